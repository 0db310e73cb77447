// The LayerNorm launches of the self-attention head: the residual LayerNorm behind a sub-layer (post-LN, sed_add_layernorm_*) and the
// residual add of one sub-layer with the LayerNorm in front of the next (pre-LN, sed_resid_layernorm_*).  One kernel family serves both:
// a forward, a backward over rows, the dgamma / dbeta partials and their reduction.
//
// LayerNorm: with v = x + f a the summed row (f: the factor of a, below), y = (v - mean) * rstd * gamma + beta per row, mean and the centred
// sum of squares in two passes (biased variance, rstd = 1/sqrt(var + eps)), one wave per row, each lane its columns in ascending order and
// one fixed wave reduction.  Backward with g = dy * gamma, xhat = (v - mean) * rstd:
//   dv = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)) (+ dres_in), the gradient of x;  da = f dv, the gradient of a;
//   dgamma = sum_rows dy * xhat and dbeta = sum_rows dy through per-workgroup partials (LN_ROWS_PER_WG rows each) in the workspace and a
//   fixed-order reduction over the workgroups.
// The factor: f = s m sd, multiplied in fp32 first and applied as ONE fma per element, v = fma(a, f, x): s the residual scale, m the
// dropout mask and sd = 1 / (1 - p) its scale (philox.h; generated in registers in the forward and again in the backward, never
// stored), m sd = 1 without dropout.  The plain instantiations (DROP = false) generate nothing, and an entry called with thr = 0 (p = 0)
// launches them.  Four consecutive columns sit on the four lanes of a quad and share their Philox counter: every lane makes the call of
// another column step (row kernels) or row step (partial kernel) and the words change places inside the quad with DPP quad permutes.
//
// post-LN  sed_add_layernorm_fwd / _bwd (and their _drop twins): s = 1, v is not stored -- the backward recomputes it from x, a and the
//          mask (STORED = false); dres is the gradient of x, and of a too without dropout (the _drop backward writes da = m sd dres).
// pre-LN   sed_resid_layernorm_fwd stores v as xsum (the residual stream behind the add) beside y and stats = (mean, rstd); a == NULL:
//          y = LayerNorm(x) and nothing else.  sed_resid_layernorm_bwd reads the STORED xsum (neither x nor a), adds the stream gradient
//          that has arrived, dxsum = dres_in + dv, and writes da = s m sd dxsum where it is asked for.  A thread reads an element of
//          dres_in before it writes the same element of dxsum: they may alias.
// With s = 1 fma(a, 1 * m sd, x) is the post-LN sum, and both forms take the same sums in the same order: the pre-LN forward gives the
// post-LN forward's bits, and the pre-LN backward the plain post-LN backward's on (xsum, zeros) (tests/test_gpu_preln.py).  The expressions
// are written once, in one shape, with the fused operations that matter as explicit fmaf calls; the file is compiled with
// -ffp-contract=fast, and what the compiler contracts beyond those is its own choice per instantiation (measured once: the dropout
// backward's dx and da of the two forms differ in the last place in the columns from 64 LN_MSK on, nowhere else).
#include "common.h"
#include "philox.h"
#include <math.h>
#include <type_traits>

#define LN_ROWS_PER_WG 64     // rows behind one dgamma / dbeta partial

namespace {

// each(f): f(c, s m sd) for a lane's columns lane + 64 k of one row in ascending order.  DROP = false: the stride-64 loop with the factor s.
// DROP: m sd of the columns k < LN_MSK is made once per row and kept in registers over the passes -- the four lanes of a quad own four
// consecutive columns, which share their counter, so lane L of the quad makes the call of step k0 + L and the words change places inside
// the quad (quad_word): one call per lane and four steps = 256 columns.  Columns from 64 LN_MSK on take a call each.
#define LN_MSK 8
template <bool DROP> struct LnCols {
    const DropArgs& d;
    const DropKey key;
    const float s;
    const size_t row;
    const int C, lane;
    float ms[LN_MSK];
    __device__ __forceinline__ LnCols(const DropArgs& d_, float s_, size_t row_, int C_, int lane_)
        : d(d_), key(drop_key<DROP>(d_)), s(s_), row(row_), C(C_), lane(lane_) {
        const int L = lane & 3;
#pragma unroll
        for (int k0 = 0; DROP && k0 < LN_MSK; k0 += 4) {
            if (64 * k0 < C) {                         // (uniform: every lane of the wave takes part in the permutes)
                const PhiloxWords w = drop_row_words(key, row, (uint32_t)((lane >> 2) + 16 * (k0 + L)));
                ms[k0 + 0] = drop_ms(quad_word<0>(w, L), d);
                ms[k0 + 1] = drop_ms(quad_word<1>(w, L), d);
                ms[k0 + 2] = drop_ms(quad_word<2>(w, L), d);
                ms[k0 + 3] = drop_ms(quad_word<3>(w, L), d);
            } else {
                ms[k0 + 0] = ms[k0 + 1] = ms[k0 + 2] = ms[k0 + 3] = 0.f;
            }
        }
    }
    template <typename Fn> __device__ __forceinline__ void each(Fn f) const {
        if constexpr (DROP) {
#pragma unroll
            for (int k = 0; k < LN_MSK; ++k) {
                const int c = lane + 64 * k;
                if (c < C) f(c, s * ms[k]);
            }
            for (int c = lane + 64 * LN_MSK; c < C; c += 64) f(c, s * drop_row_ms(key, d, row, c));
        } else {
            for (int c = lane; c < C; c += 64) f(c, s);
        }
    }
};

// the LayerNorm of one row: each(f) calls f(c, v) for the lane's columns of the summed row in ascending order
template <typename Each>
__device__ __forceinline__ void ln_row(Each each, const float* __restrict__ gamma, const float* __restrict__ beta,
                                       float* __restrict__ yr, float* __restrict__ stats, size_t row, int C, float eps, int lane) {
    float s = 0.f;
    each([&](int c, float v) { s += v; });
    const float mean = wave_sum(s) / (float)C;
    float ss = 0.f;
    each([&](int c, float v) { const float d = v - mean; ss = fmaf(d, d, ss); });
    const float rstd = 1.f / sqrtf(wave_sum(ss) / (float)C + eps);
    each([&](int c, float v) { yr[c] = (v - mean) * rstd * gamma[c] + beta[c]; });
    if (stats != nullptr && lane == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
}

// HAS_A = false: y = LayerNorm(x).  STORE: the pre-LN form, xsum = the summed row; else the post-LN form, nothing stored and s = 1 (a
// compile-time switch: the post-LN launches carry no branch for the store, and their sum is x + m sd a, the plain one x + a)
template <bool HAS_A, bool DROP, bool STORE>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ a, float s,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float* __restrict__ xsum, float* __restrict__ y, float* __restrict__ stats,
                                                     size_t rows, int C, float eps, DropArgs drop) {
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* __restrict__ xr = x + row * C;
    float* __restrict__ yr = y + row * C;
    if constexpr (!HAS_A) {
        ln_row([&](auto f) { for (int c = lane; c < C; c += 64) f(c, xr[c]); }, gamma, beta, yr, stats, row, C, eps, lane);
    } else {
        const float* __restrict__ ar = a + row * C;
        const LnCols<DROP> cols(drop, STORE ? s : 1.f, row, C, lane);
        auto each = [&](auto f) { cols.each([&](int c, float fa) { f(c, fmaf(ar[c], fa, xr[c])); }); };
        if constexpr (STORE) {
            float* __restrict__ sr = xsum + row * C;
            each([&](int c, float v) { sr[c] = v; });
        }
        ln_row(each, gamma, beta, yr, stats, row, C, eps, lane);
    }
}

// dx = (dres_in +) dv, da = f dx.  STORED: the pre-LN form, x is the stored sum and a is not read; else the post-LN form, the sum is
// recomputed, fma(a, f, x) with s = 1.
// dres_in and dx carry no __restrict__: they may be the same buffer
template <bool STORED, bool HAS_RES, bool HAS_DA, bool DROP>
__global__ __launch_bounds__(256) void ln_bwd_row_kernel(const float* __restrict__ dy, const float* dres_in, const float* __restrict__ x,
                                                         const float* __restrict__ a, float s, const float* __restrict__ gamma,
                                                         const float* __restrict__ stats, float* dx, float* __restrict__ da,
                                                         size_t rows, int C, DropArgs drop) {
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* __restrict__ xr = x + row * C;
    const float* __restrict__ ar = STORED ? nullptr : a + row * C;
    const float* __restrict__ gr = dy + row * C;
    const float mean = stats[2 * row], rstd = stats[2 * row + 1];
    const LnCols<DROP> cols(drop, STORED ? s : 1.f, row, C, lane);
    // f(c, g, xhat, factor of a)
    auto each = [&](auto f) {
        cols.each([&](int c, float fa) {
            const float v = STORED ? xr[c] : fmaf(ar[c], fa, xr[c]);
            f(c, gr[c] * gamma[c], (v - mean) * rstd, fa);
        });
    };
    float s1 = 0.f, s2 = 0.f;
    each([&](int c, float g, float xh, float fa) {
        s1 += g;
        s2 = fmaf(g, xh, s2);
    });
    const float m1 = wave_sum(s1) / (float)C, m2 = wave_sum(s2) / (float)C;
    each([&](int c, float g, float xh, float fa) {
        // (the add of dres_in as an explicit fma: every instantiation rounds it the same way, whatever the compiler contracts)
        const float in = (g - m1) - xh * m2;
        const float d = HAS_RES ? fmaf(rstd, in, dres_in[row * C + c]) : rstd * in;
        dx[row * C + c] = d;
        if (HAS_DA) da[row * C + c] = d * fa;
    });
}

// f(row, m sd) for each of a thread's rows r0 + ry + 4 i < r1 of column c in ascending order (live: the column exists)
template <bool DROP, typename Fn>
__device__ __forceinline__ void ln_part_rows(const DropArgs& drop, size_t r0, size_t r1, int ry, int c, bool live, Fn f) {
    if constexpr (DROP) {
        // a quad's four columns share the counter of a row: lane L of the quad makes the call of row step it0 + L and the words change
        // places inside the quad; every thread takes part in the permutes, whatever its column and rows
        const DropKey key(drop);
        const int L = threadIdx.x & 3;
        for (int it0 = 0; it0 < LN_ROWS_PER_WG / 4; it0 += 4) {
            const PhiloxWords w = drop_row_words(key, r0 + ry + 4 * (size_t)(it0 + L), (uint32_t)c >> 2);
            const float ms4[4] = {drop_ms(quad_word<0>(w, L), drop), drop_ms(quad_word<1>(w, L), drop), drop_ms(quad_word<2>(w, L), drop),
                                  drop_ms(quad_word<3>(w, L), drop)};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t row = r0 + ry + 4 * (size_t)(it0 + j);
                if (live && row < r1) f(row, ms4[j]);
            }
        }
    } else if (live) {
        for (size_t row = r0 + ry; row < r1; row += 4) f(row, 1.f);
    }
}

// partial[chunk][0][c] = sum over the chunk's rows of dy * xhat, partial[chunk][1][c] = sum of dy: 64 columns x 4 row lanes per
// workgroup, each row lane its rows (stride 4) in ascending order, then the four in a fixed order.  STORED as in the row kernel
template <bool STORED, bool DROP>
__global__ __launch_bounds__(256) void ln_bwd_part_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                          const float* __restrict__ a, const float* __restrict__ stats,
                                                          float* __restrict__ partial, size_t rows, int C, DropArgs drop) {
    __shared__ float sh[2][4][64];
    const int cl = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const size_t r0 = (size_t)blockIdx.y * LN_ROWS_PER_WG;
    const size_t r1 = r0 + LN_ROWS_PER_WG < rows ? r0 + LN_ROWS_PER_WG : rows;
    float sg = 0.f, sb = 0.f;
    ln_part_rows<DROP>(drop, r0, r1, ry, c, c < C, [&](size_t row, float ms) {
        const float g = dy[row * C + c];
        const float v = STORED ? x[row * C + c] : fmaf(a[row * C + c], ms, x[row * C + c]);
        const float xh = (v - stats[2 * row]) * stats[2 * row + 1];
        sg = fmaf(g, xh, sg);
        sb += g;
    });
    sh[0][ry][cl] = sg;
    sh[1][ry][cl] = sb;
    __syncthreads();
    if (ry == 0 && c < C) {
        partial[((size_t)blockIdx.y * 2 + 0) * C + c] = (sh[0][0][cl] + sh[0][1][cl]) + (sh[0][2][cl] + sh[0][3][cl]);
        partial[((size_t)blockIdx.y * 2 + 1) * C + c] = (sh[1][0][cl] + sh[1][1][cl]) + (sh[1][2][cl] + sh[1][3][cl]);
    }
}

__global__ __launch_bounds__(256) void ln_bwd_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, int nchunks, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float sg = 0.f, sb = 0.f;
    for (int k = 0; k < nchunks; ++k) {
        sg += partial[((size_t)k * 2 + 0) * C + c];
        sb += partial[((size_t)k * 2 + 1) * C + c];
    }
    dgamma[c] = sg;
    dbeta[c] = sb;
}

// ---- host: one launcher each way.  A run-time bool picks a template argument as in mhsa_dispatch: f(std::true_type / std::false_type)
const std::true_type T{};
const std::false_type F{};
template <typename Fn> void with_bool(bool b, Fn f) {
    if (b) f(T);
    else f(F);
}

// a NULL: y = LayerNorm(x).  xsum NULL: the post-LN entries, the sum is not stored and s is 1.  d.thr = 0: the plain instantiations.
// required: the entry's wording of which pointers it needs
int ln_fwd_launch(const float* x, const float* a, float s, const float* gamma, const float* beta, float* xsum, float* y, float* stats,
                  size_t rows, int C, float eps, const DropArgs& d, const char* required, void* stream) {
    SED_REQUIRE(rows > 0 && C > 0, "sizes must be positive");
    SED_REQUIRE(x != nullptr && gamma != nullptr && beta != nullptr && y != nullptr, required);
    SED_REQUIRE(cdivz(rows, 4) < ((size_t)1 << 31), "too many rows");
    auto go = [&](auto has_a, auto drop, auto store) {
        ln_fwd_kernel<decltype(has_a)::value, decltype(drop)::value, decltype(store)::value>
            <<<(unsigned)cdivz(rows, 4), 256, 0, (hipStream_t)stream>>>(x, a, s, gamma, beta, xsum, y, stats, rows, C, eps, d);
    };
    if (a == nullptr) go(F, F, F);
    else with_bool(d.thr != 0, [&](auto drop) { with_bool(xsum != nullptr, [&](auto store) { go(T, drop, store); }); });
    SED_LAUNCH_CHECK();
    return 0;
}

// a NULL: x is the stored sum (the pre-LN entry); else the sum is recomputed from x, a and the mask, and da is written under dropout only
// (the post-LN entries: no dres_in).  d.thr = 0: the plain instantiations
int ln_bwd_launch(const float* dy, const float* dres_in, const float* x, const float* a, float s, const float* gamma, const float* stats,
                  float* dx, float* da, float* dgamma, float* dbeta, float* workspace, size_t rows, int C, const DropArgs& d,
                  const char* required, void* stream) {
    SED_REQUIRE(rows > 0 && C > 0, "sizes must be positive");
    SED_REQUIRE(dy != nullptr && x != nullptr && gamma != nullptr && stats != nullptr && dx != nullptr && dgamma != nullptr &&
                dbeta != nullptr && workspace != nullptr, required);
    const size_t nchunks = cdivz(rows, LN_ROWS_PER_WG);
    SED_REQUIRE(nchunks <= 65535, "too many rows (the partial grid takes 65535 * 64)");
    const bool drop = da != nullptr && d.thr != 0;
    hipStream_t st = (hipStream_t)stream;
    auto row = [&](auto stored, auto res, auto has_da, auto dr) {
        ln_bwd_row_kernel<decltype(stored)::value, decltype(res)::value, decltype(has_da)::value, decltype(dr)::value>
            <<<(unsigned)cdivz(rows, 4), 256, 0, st>>>(dy, dres_in, x, a, s, gamma, stats, dx, da, rows, C, d);
    };
    auto part = [&](auto stored, auto dr) {
        ln_bwd_part_kernel<decltype(stored)::value, decltype(dr)::value>
            <<<dim3((unsigned)cdiv(C, 64), (unsigned)nchunks), 256, 0, st>>>(dy, x, a, stats, workspace, rows, C, d);
    };
    if (a == nullptr)
        with_bool(dres_in != nullptr, [&](auto res) {
            if (drop) row(T, res, T, T);
            else if (da != nullptr) row(T, res, T, F);
            else row(T, res, F, F);
        });
    else if (drop) row(F, F, T, T);
    else row(F, F, F, F);
    SED_LAUNCH_CHECK();
    if (a == nullptr) part(T, F);
    else if (drop) part(F, T);
    else part(F, F);
    SED_LAUNCH_CHECK();
    ln_bwd_reduce_kernel<<<(unsigned)cdiv(C, 256), 256, 0, st>>>(workspace, dgamma, dbeta, (int)nchunks, C);
    SED_LAUNCH_CHECK();
    return 0;
}

// the post-LN entries: a is required, s = 1, nothing is stored
int add_ln_fwd(const float* x, const float* a, const float* gamma, const float* beta, float* y, float* stats, size_t rows, int C,
               float eps, const DropArgs& d, void* stream) {
    SED_REQUIRE(a != nullptr, "x, a, gamma, beta and y are required");
    return ln_fwd_launch(x, a, 1.f, gamma, beta, nullptr, y, stats, rows, C, eps, d, "x, a, gamma, beta and y are required", stream);
}
int add_ln_bwd(const float* dy, const float* x, const float* a, const float* gamma, const float* stats, float* dres, float* da,
               float* dgamma, float* dbeta, float* workspace, size_t rows, int C, const DropArgs& d, void* stream) {
    SED_REQUIRE(a != nullptr, "every pointer is required");
    return ln_bwd_launch(dy, nullptr, x, a, 1.f, gamma, stats, dres, da, dgamma, dbeta, workspace, rows, C, d, "every pointer is required",
                         stream);
}

// the scale and dropout arguments of an entry whose added tensor is present: s finite, p in [0, 1), rng required only for p > 0
int resid_scale_args(float s, float p, const uint32_t* rng, uint32_t stream_id, DropArgs* d) {
    SED_REQUIRE(isfinite(s), "the residual scale s must be finite");
    if (int rc = drop_require_args(p, rng, stream_id, d)) return rc;
    SED_REQUIRE(p == 0.f || rng != nullptr, "the dropout state rng is required for p > 0");
    return 0;
}
}  // namespace

extern "C" int sed_add_layernorm_fwd(const float* x, const float* a, const float* gamma, const float* beta, float* y, float* stats,
                                     size_t rows, int C, float eps, void* stream) {
    return add_ln_fwd(x, a, gamma, beta, y, stats, rows, C, eps, DropArgs{}, stream);
}

// the dropout twins: p in [0, 1) and the state (required whatever p is), then the plain entry's checks
extern "C" int sed_add_layernorm_fwd_drop(const float* x, const float* a, const float* gamma, const float* beta, float* y, float* stats,
                                          size_t rows, int C, float eps, float p, const uint32_t* rng, uint32_t stream_id, void* stream) {
    SED_REQUIRE(rng != nullptr, "the dropout state rng is required");
    DropArgs d;
    if (int rc = drop_require_args(p, rng, stream_id, &d)) return rc;
    return add_ln_fwd(x, a, gamma, beta, y, stats, rows, C, eps, d, stream);
}

extern "C" size_t sed_add_layernorm_bwd_ws_floats(size_t rows, int C) {
    if (rows == 0 || C <= 0) return 0;
    return cdivz(rows, LN_ROWS_PER_WG) * 2 * (size_t)C;
}

extern "C" int sed_add_layernorm_bwd(const float* dy, const float* x, const float* a, const float* gamma, const float* stats,
                                     float* dres, float* dgamma, float* dbeta, float* workspace, size_t rows, int C, void* stream) {
    return add_ln_bwd(dy, x, a, gamma, stats, dres, nullptr, dgamma, dbeta, workspace, rows, C, DropArgs{}, stream);
}

extern "C" int sed_add_layernorm_bwd_drop(const float* dy, const float* x, const float* a, const float* gamma, const float* stats,
                                          float* dres, float* da, float* dgamma, float* dbeta, float* workspace, size_t rows, int C,
                                          float p, const uint32_t* rng, uint32_t stream_id, void* stream) {
    SED_REQUIRE(rng != nullptr, "the dropout state rng is required");
    DropArgs d;
    if (int rc = drop_require_args(p, rng, stream_id, &d)) return rc;
    SED_REQUIRE(da != nullptr, "da is required");
    if (int rc = add_ln_bwd(dy, x, a, gamma, stats, dres, da, dgamma, dbeta, workspace, rows, C, d, stream)) return rc;
    if (d.thr == 0) {                                  // the plain kernels ran: da = dres
        const hipError_t e = hipMemcpyAsync(da, dres, rows * (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
        SED_REQUIRE(e == hipSuccess, "the copy of dres into da failed");
    }
    return 0;
}

extern "C" int sed_resid_layernorm_fwd(const float* x, const float* a, float s, const float* gamma, const float* beta, float* xsum,
                                       float* y, float* stats, size_t rows, int C, float eps, float p, const uint32_t* rng,
                                       uint32_t stream_id, void* stream) {
    DropArgs d{};
    if (a != nullptr) {
        SED_REQUIRE(xsum != nullptr, "xsum is required with a");
        if (int rc = resid_scale_args(s, p, rng, stream_id, &d)) return rc;
    }
    return ln_fwd_launch(x, a, s, gamma, beta, xsum, y, stats, rows, C, eps, d, "x, gamma, beta and y are required", stream);
}

extern "C" size_t sed_resid_layernorm_bwd_ws_floats(size_t rows, int C) { return sed_add_layernorm_bwd_ws_floats(rows, C); }

extern "C" int sed_resid_layernorm_bwd(const float* dy, const float* dres_in, const float* xsum, const float* gamma, const float* stats,
                                       float s, float* dxsum, float* da, float* dgamma, float* dbeta, float* workspace, size_t rows,
                                       int C, float p, const uint32_t* rng, uint32_t stream_id, void* stream) {
    DropArgs d{};
    if (da != nullptr)
        if (int rc = resid_scale_args(s, p, rng, stream_id, &d)) return rc;
    return ln_bwd_launch(dy, dres_in, xsum, nullptr, s, gamma, stats, dxsum, da, dgamma, dbeta, workspace, rows, C, d,
                         "every pointer but dres_in and da is required", stream);
}
