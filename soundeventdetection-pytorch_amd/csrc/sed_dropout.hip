// The keep mask of the self-attention head's dropout, written out: what the fused _drop kernels (sed_mhsa.hip, sed_layernorm.hip, sed_ffn.hip) generate
// in registers and never store.  One definition, philox.h; tests/dropout_formula.py is the same in numpy.
//   SED_DROP_ROWS:  keep[r][c],        r < n0, c < n1           (a row tensor [R][N])
//   SED_DROP_ATTN:  keep[b][g][i][j],  b < n0, g < n1, i, j < t (the attention probabilities)
// One thread per four consecutive columns / keys (one call), bytes 0 / 1.
#include "common.h"
#include "philox.h"

namespace {

__global__ __launch_bounds__(256) void dropout_mask_kernel(unsigned char* __restrict__ keep, int kind, size_t n0, int n1, int t,
                                                           DropArgs drop) {
    const bool attn = kind == SED_DROP_ATTN;
    const int N = attn ? t : n1;                       // the row length
    const int nq = (N + 3) / 4;
    const size_t rows = attn ? n0 * (size_t)n1 * (size_t)t : n0;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * (size_t)nq) return;
    const size_t row = idx / nq;
    const uint32_t q = (uint32_t)(idx % nq);
    const DropKey key(drop);
    const PhiloxWords w = attn ? drop_attn_words(key, q, (uint32_t)(row % (size_t)t), (uint32_t)(row / (size_t)t))
                               : drop_row_words(key, row, q);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if ((int)(4 * q) + j < N) keep[row * (size_t)N + 4 * q + j] = w.w[j] >= drop.thr ? 1 : 0;
}

}  // namespace

extern "C" int sed_dropout_mask(unsigned char* keep, int kind, size_t n0, int n1, int t, float p, const uint32_t* rng,
                                uint32_t stream_id, void* stream) {
    SED_REQUIRE(kind == SED_DROP_ROWS || kind == SED_DROP_ATTN, "kind must be SED_DROP_ROWS or SED_DROP_ATTN");
    SED_REQUIRE(keep != nullptr && rng != nullptr, "keep and the dropout state rng are required");
    SED_REQUIRE(n0 > 0 && n1 > 0 && (kind == SED_DROP_ROWS || t > 0), "sizes must be positive");
    DropArgs d;
    if (int rc = drop_require_args(p, rng, stream_id, &d)) return rc;
    const bool attn = kind == SED_DROP_ATTN;
    SED_REQUIRE(!attn || n0 * (size_t)n1 < ((size_t)1 << 32), "B * H must stay below 2^32");
    const size_t rows = attn ? n0 * (size_t)n1 * (size_t)t : n0;
    const size_t work = rows * (size_t)(((attn ? t : n1) + 3) / 4);
    SED_REQUIRE(cdivz(work, 256) < ((size_t)1 << 31), "too many elements");
    dropout_mask_kernel<<<(unsigned)cdivz(work, 256), 256, 0, (hipStream_t)stream>>>(keep, kind, n0, n1, t, d);
    SED_LAUNCH_CHECK();
    return 0;
}
