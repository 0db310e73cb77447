// Self-attention temporal head: the multi-head attention core (forward and backward, flash form, on the matrix pipe).  The projections
// around the core are sed_gemm_nt / sed_gemm_tn launches (sed_gru.hip), the LayerNorms around the sub-layers sed_layernorm.hip.
//
// Core, for one clip b and head g (dh = 32 or 64 columns [g*dh, (g+1)*dh) of each third of a qkv row), scale = 1/sqrt(dh):
//   s_ij  = scale * sum_c q_ic k_jc                      i, j over the t frames of the SAME clip, no mask
//   lse_i = max_j s_ij + ln sum_j exp(s_ij - max_j s_ij)
//   p_ij  = exp(s_ij - lse_i),   ctx_ic = sum_j p_ij v_jc
// backward, with D_i = sum_c dctx_ic ctx_ic (per head):
//   dv_jc = sum_i p_ij dctx_ic          dp_ij = sum_c dctx_ic v_jc          ds_ij = p_ij (dp_ij - D_i)
//   dq_ic = scale sum_j ds_ij k_jc      dk_jc = scale sum_i ds_ij q_ic
// (tests/mhsa_formula.py is the same in float64 numpy.)
//
// Forward: a workgroup is four waves, each wave owns 32 queries of one (clip, head) and walks the keys in tiles of 32; the t x t
// scores never reach memory.  The wave computes S^T = K Q^T (32x32 MFMA, key in the accumulator registers, query on the lane), so
// a lane holds 16 scores of ONE query and the other half-wave's lane the other 16: the running maximum and sum are per-lane fp32
// scalars plus one exchange with lane ^ 32, and the probabilities are already the B operand of O^T = V^T P^T (an accumulator tile as
// the next MFMA's operand: P never passes through LDS).  O^T has the query on the lane too, so the rescale by
// exp(m_old - m_new) and the final 1/sum are per-lane scalars.  ctx = O / sum, lse = m + ln(sum).
// Where the operands come from: the bf16 forward stages each K / V tile once per workgroup in LDS, rounded to bf16 (mhsa_fwd_lds_kernel
// below: 0.079 -> 0.063 ms at B 32, t 750, 4 heads of 32 against every wave loading and converting the tiles itself).  The fp32
// forward and the three backward kernels load their operands straight from global memory into registers (a clip's q, k, v of one head
// are 3 t dh floats and stay in L2), the next tile's rows while the current tile is computed; their four waves share nothing.
// Backward: sed_mhsa_bwd is three launches, all in a fixed order (no atomics, the same bits on every run):
//   1. D_i per (clip, head, frame) into the workspace;
//   2. waves that own 32 KEYS loop over the query tiles: S = Q K^T and dP = dctx V^T with the key on the lane, P and dS rebuilt in
//      registers and fed as B operands to dV^T += dctx^T P and dK^T += Q^T dS;
//   3. waves that own 32 QUERIES loop over the key tiles: S^T and dP^T with the query on the lane (lse_i and D_i are lane scalars),
//      dQ^T += K^T dS^T.
// S is recomputed in both passes; dqkv is overwritten, every element of its B*t rows.
//
// dtype: SED_BF16 -- q, k, v (and dctx in the backward) are rounded to bf16 (nearest even) as MFMA operands of
// v_mfma_f32_32x32x16_bf16, and so are the probabilities as the operand of P V (backward: P for dV, dS for dK and dQ); the scores,
// the maximum, the sum, lse, D, P and dS themselves, every accumulator and every stored tensor are fp32.  The sum that normalises
// ctx is taken over the fp32 probabilities.  SED_F32 -- the same dataflow on v_mfma_f32_32x32x2_f32 (exact fp32 products).
//
// Ragged tiles: any t >= 1.  Loads of rows past the clip are clamped to its last row (always real data of the same clip), their
// scores are set to -inf (p = 0) or their p / dS to 0, and no row past t is stored: nothing outside the B*t rows is read or written.
// Addressing: 64-bit clip base + 32-bit offsets inside a clip: t * 3C * 4 bytes must stay below 2^31, and B*H*ceil(t/128) below 2^31
// workgroups.  qkv, ctx, dctx, dqkv must be 16-byte aligned (rows are read and written with 16-byte accesses).
//
// Dropout (the DROP instantiations behind sed_mhsa_fwd_drop / sed_mhsa_bwd_drop; masks m and scale s = 1 / (1 - p) from philox.h,
// generated in registers in the forward and again in the backward, never stored):
//   core       lse_i and p_ij as above, over all keys (no renormalisation);  p~_ij = m_ij s p_ij,  ctx_ic = sum_j p~_ij v_jc.  In the
//              running form exp(s_ij - m_run) is multiplied by m_ij s in fp32 for the P V operand only (SED_BF16: the operand is
//              bf16(p m s)); the normalising sum is still taken over the undropped fp32 probabilities.
//              dv_jc = sum_i p~_ij dctx_ic,  dp_ij = m_ij s sum_c dctx_ic v_jc,  ds_ij = p_ij (dp_ij - D_i);  D_i = sum_c dctx_ic ctx_ic
//              holds with the dropped ctx, so launch 1 is unchanged.
// A lane of the forward and of the dQ pass holds four consecutive keys of one query in registers 4 n ... 4 n + 3: one Philox call per
// four scores.  Where four consecutive keys sit on the four lanes of a quad (the dK / dV pass) the quad shares the counter: every lane
// makes the call of another query and the words change places inside the quad with DPP quad permutes (quad_word, philox.h).  The plain instantiations (DROP = false) are the code they were; a twin called with thr = 0
// (p = 0) launches the plain instantiation.
//
// Local window (the WIN instantiations behind sed_mhsa_fwd_win / sed_mhsa_bwd_win; left, right >= 0, the same for every head): key j
// takes part for query i iff i - left <= j <= i + right.  lse_i, p_ij and ctx_i run over the in-window keys only, p_ij = 0 outside; in the
// backward ds_ij = 0 outside, and dv, dq, dk, D_i are built from those.  The diagonal is always inside: no row is empty.  Dropout composes
// (p~_ij = m_ij s p_ij with p over the window; the counters are indexed by the absolute (b H + g, i, j, step), the same cells dropped).
//   tiles      mhsa_win_range, one __host__ __device__ helper for the kernels and for sed_mhsa_win_tiles: a wave that owns queries
//              [q0, q0 + 31] walks the key tiles that meet [q0 - left, q0 + 31 + right] and [0, t); a wave that owns keys [k0, k0 + 31]
//              (the dK / dV pass) the query tiles that meet [k0 - right, k0 + 31 + left].  The prefetch a tile ahead starts at the first
//              visited tile.  mhsa_fwd_lds_kernel stages the union of its four waves' ranges (loop bounds and `more` the same in every
//              thread: the barrier is uniform); a wave computes on the tiles of its own range and stages and waits on the others.
//   mask       inside a visited tile, by select: forward score -inf; backward p = dS = 0 without taking exp(s - lse) of an out-of-window
//              cell (lse covers the window only, so that exponential can overflow).
//   maximum    a query's first visited tiles can lie wholly outside its window (left = 3: queries 32 ... 63 start at key tile 0, where
//              query 40 has no key); while its running maximum is -inf the reference point of the tile is 0, so alpha and every
//              probability are exp(-inf) = 0 instead of exp(-inf + inf).
// The host clamps left and right to t - 1 (nothing overflows; a side that reaches the clip's end from every query is unbounded); both
// sides unbounded launches the WIN = false instantiation, plain or DROP, which is the code it was.  Ragged tiles, clamped loads, the 2^31
// limits, no atomics, a fixed order and the same bits on every run as above.
//
// Relative-position bias (the REL instantiations behind sed_mhsa_fwd_rel / sed_mhsa_bwd_rel, always with WIN = true: both sides unbounded is
// a valid window; rel[H][2t - 1] fp32, one row per head, index d + t - 1 for the distance d = j - i, key minus query):
//   s_ij = scale * sum_c q_ic k_jc + rel[g][(j - i) + t - 1]         lse, p, p~, ctx, D, dv, dp, ds, dq, dk as above with this s
//   drel[g][d + t - 1] = sum_b sum_{(i, j) in the window, j - i = d} ds_ij                  (no scale: it enters dq and dk only)
//   stage      a wave keeps the slice of its head's row that its walk can reach in LDS of its own (rel_stage below), 256 walked rows at a
//              time; the forward and the dQ pass read slot (key - chunk start) + 31 - (lane & 31), the dK / dV pass the mirrored slice
//   backward   the exponent is written scale s - (lse - rel): the shape of the other instantiations, so a zero table gives their bits
//   drel       the dQ pass holds dS of a tile with the key in the register and the query on the lane: lane X gathers diagonal
//              X = key row - query lane + 31 of the tile from the two half-waves (32 lane reads, fixed order), stores the 32 diagonals no
//              later tile meets into the wave's workspace row and carries the other 31 down 32 lanes; mhsa_rel_reduce_kernel sums the rows
//              over waves and clips in fp64 in a fixed order and rounds once.  Masked cells are exact zeros (select), no exp is taken there.
// sed_relpos_expand: rel[g][x] = w[g][map[x]] (bit copy); sed_relpos_fold: dw[g][n] = sum_{x: map[x] = n} drel[g][x], fp64, ascending x,
// rounded once, 0 for an empty bucket.  The bucket map is the host's (sed_relpos_map_check); the hot kernels never see it.
#include "common.h"
#include "philox.h"
#include <math.h>
#include <type_traits>

#define MHSA_QT 32            // queries (or keys) a wave owns
#define MHSA_WAVES 4          // waves per workgroup, each with its own tile

namespace {

// row of the 32x32 accumulator that register i of lane half h holds
__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// ---- the fragments of one row-major row (dh head columns) as the operand of a product summed over the columns -----------------
// bf16: k-step s (16 columns) takes columns 16 s + 8 h + j in element j;  fp32: k-step kk (2 columns) takes column h * dh/2 + kk
// (both operands of a product use the same map, so the order of the k index inside the sum is free)
template <typename T, int DH> struct RowFrag;
template <int DH> struct RowFrag<bf16_t, DH> {
    static constexpr int N = DH / 16;
    bf16x8 f[N];
    __device__ __forceinline__ void load(const float* __restrict__ row, int h) {
#pragma unroll
        for (int s = 0; s < N; ++s) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(row + 16 * s + 8 * h);
            const f32x4 b = *reinterpret_cast<const f32x4*>(row + 16 * s + 8 * h + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { f[s][j] = (bf16_t)a[j]; f[s][4 + j] = (bf16_t)b[j]; }
        }
    }
};
template <int DH> struct RowFrag<float, DH> {
    static constexpr int N = DH / 2;
    float f[N];
    __device__ __forceinline__ void load(const float* __restrict__ row, int h) {
#pragma unroll
        for (int s = 0; s < N / 4; ++s) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(row + h * N + 4 * s);
#pragma unroll
            for (int j = 0; j < 4; ++j) f[4 * s + j] = a[j];
        }
    }
};

// acc[row of A][row of B] = sum_c A[.][c] B[.][c]: A's row index lands in the accumulator registers, B's on the lane
template <typename T, int DH>
__device__ __forceinline__ f32x16 mm_rows(const RowFrag<T, DH>& a, const RowFrag<T, DH>& b) {
    f32x16 acc = {};
#pragma unroll
    for (int s = 0; s < RowFrag<T, DH>::N; ++s) acc = mfma(a.f[s], b.f[s], acc);
    return acc;
}

// One column of a 32-row tile as the A operand of the product below: a[i] = M[row0 + acc_row(i, h)][c], col pointing at column c =
// this lane's (lane & 31) of row 0 of the clip; rows >= t are read from row t - 1 (their x is 0).  Kept apart from the product so that
// a kernel can issue these loads a tile ahead, or at the top of the tile, and the wave does not sit out their latency between MFMAs.
__device__ __forceinline__ void load_col(float (&a)[16], const float* __restrict__ col, int ld, int row0, int t, int h) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        int row = row0 + acc_row(i, h);
        row = row < t ? row : t - 1;
        a[i] = col[row * ld];
    }
}
// acc[c][lane] += sum_rows a[row] * x[row][lane], x an accumulator tile (row in the registers)
template <typename T> struct MmAx;
template <> struct MmAx<bf16_t> {
    static __device__ __forceinline__ void run(f32x16& acc, const float (&a)[16], const f32x16& x) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 af, b;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                af[j] = (bf16_t)a[8 * s + j];
                b[j] = (bf16_t)x[8 * s + j];
            }
            acc = mfma(af, b, acc);
        }
    }
};
template <> struct MmAx<float> {
    static __device__ __forceinline__ void run(f32x16& acc, const float (&a)[16], const f32x16& x) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float af = a[i], b = x[i];
            acc = mfma(af, b, acc);
        }
    }
};

__device__ __forceinline__ float xor32(float v) { return __shfl_xor(v, 32, 64); }

struct MhsaParams {
    const float* qkv;
    const float* ctx;
    const float* dctx;
    const float* lse;
    float* out;          // ctx (forward) / dqkv (backward)
    float* lse_out;
    float* D;            // workspace [B][H][t]
    int t, H, ntile;     // ntile = ceil(t / 128) workgroups per (clip, head)
    float scale;
    DropArgs drop;       // the DROP instantiations only
    int wl, wr;          // the WIN instantiations only: left and right, clamped to t - 1 by the host
    const float* rel;    // the REL instantiations only: the per-distance table [H][2t - 1]
    float* relws;        // dQ pass: per-wave diagonal partials [B][H][ntile * MHSA_WAVES][relspan]
    int relspan;
};

// A thread's place in a core launch: workgroup blockIdx.x is tile `tile` (128 rows) of clip b and head g, its wave `wave` owns the 32 rows
// from row0 (queries, or keys in the dK / dV pass); r = the lane's row or column inside a 32 x 32 tile, h = its half-wave
template <int DH> struct WaveTile {
    int lane, wave, r, h, bh, tile, b, g, C, ld, row0;
    __device__ __forceinline__ explicit WaveTile(const MhsaParams& p)
        : lane(threadIdx.x & 63), wave(threadIdx.x >> 6), r(lane & 31), h(lane >> 5), bh(blockIdx.x / p.ntile), tile(blockIdx.x % p.ntile),
          b(bh / p.H), g(bh % p.H), C(p.H * DH), ld(3 * C), row0((tile * MHSA_WAVES + wave) * MHSA_QT) {}
};

// ---- the local window: the tiles a wave walks --------------------------------------------------------------------------------------
// A wave (span 32) or a workgroup (span 128) that owns rows [a0, a0 + span - 1], a0 < t, of one index walks the tiles of 32 of the
// OTHER index that intersect [a0 - before, a0 + span - 1 + after] with [0, t): tile starts lo, lo + 32, ... < hi.  Queries own keys
// with (before, after) = (left, right), keys own queries with (right, left).  Rows past t widen nothing: the last real row t - 1
// already reaches t - 1 + after >= t - 1.  before, after <= t - 1 (the host clamps them), so nothing here overflows.
struct TileRange { int lo, hi; };
__host__ __device__ inline TileRange mhsa_win_range(int a0, int span, int t, int before, int after) {
    const int first = a0 - before > 0 ? a0 - before : 0;
    const int last = a0 + span - 1 + after < t - 1 ? a0 + span - 1 + after : t - 1;
    return {first & ~(MHSA_QT - 1), last + 1};
}
// key j takes part for query i (both inside the clip is the caller's business)
__device__ __forceinline__ bool in_window(int i, int j, int wl, int wr) { return j >= i - wl && j <= i + wr; }

// ---- the relative-position bias: a wave's slice of its head's table in LDS -----------------------------------------------------------
// A wave that owns 32 rows of one index and walks tiles of the other meets, over REL_CHUNK walked rows (8 tiles), REL_CHUNK + 62
// distances in a row: it stages them once per chunk with five coalesced loads per lane in its own REL_PITCH floats (5 KiB per
// workgroup whatever t is; the whole walk of t = 750 would be 17 KiB and no faster: measured), slot x = (walked row - chunk
// start) + 31 - (lane & 31), and a cell reads slot x + (its row inside the tile).  Queries own keys: slot x holds
// rel[(kc - q0 - 31 + x) + t - 1] (dir +1); keys own queries: rel[(k0 + 31 - qc - x) + t - 1] (dir -1).  Slots whose distance lies
// outside [-(t - 1), t - 1] belong to rows past the clip only (masked cells) and are read from the clamped end.  The slice is private to
// the wave: no workgroup barrier, only the wave's own program order.
#define REL_CHUNK 256
#define REL_PITCH (REL_CHUNK + 64)
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void rel_stage(float* relw, const float* __restrict__ rel_g, int base, int dir, int n, int t, int lane) {
    wave_lds_order();
    for (int x = lane; x < n; x += 64) {
        int idx = base + dir * x;
        idx = idx < 0 ? 0 : idx > 2 * t - 2 ? 2 * t - 2 : idx;
        relw[x] = rel_g[idx];
    }
    wave_lds_order();
}
// slots a chunk that starts at walked row c0 of a walk that ends at hi needs
__device__ __forceinline__ int rel_slots(int c0, int hi) {
    const int rows = ((hi - c0 + MHSA_QT - 1) & ~(MHSA_QT - 1)) < REL_CHUNK ? ((hi - c0 + MHSA_QT - 1) & ~(MHSA_QT - 1)) : REL_CHUNK;
    return rows + 31;
}
// A wave's slice over its walk from row lo: the slice (REL only: the other instantiations hold no LDS for it) and the start c0 of the
// staged chunk.  tile() at the top of the tile at walked row x0 restages where a chunk starts (own0: the wave's first own row, hi: the
// walk's end, dir as above); at() is the bias of the cell in register i of the tile at x0.
template <bool REL> struct RelWalk {
    float* relw = nullptr;
    int lo, c0;
    __device__ __forceinline__ RelWalk(int wave, int lo_) : lo(lo_), c0(lo_) {
        if constexpr (REL) {
            __shared__ float relsm[MHSA_WAVES * REL_PITCH];
            relw = relsm + wave * REL_PITCH;
        }
    }
    __device__ __forceinline__ void tile(const MhsaParams& p, int g, int own0, int x0, int hi, int dir, int lane) {
        if constexpr (REL) {
            if (((x0 - lo) & (REL_CHUNK - 1)) == 0) {
                c0 = x0;
                rel_stage(relw, p.rel + (size_t)g * (2 * p.t - 1), dir * (c0 - own0 - 31) + p.t - 1, dir, rel_slots(c0, hi), p.t, lane);
            }
        }
    }
    __device__ __forceinline__ float at(int x0, int i, int h, int r) const { return relw[(x0 - c0) + acc_row(i, h) + 31 - r]; }
};

// store the transposed 32 x 32 tile o (column c = acc_row(i, h) in the registers, row on the lane) times f into row `dst` (head columns)
__device__ __forceinline__ void store_tile_t(float* __restrict__ dst, const f32x16& o, float f, int h) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = o[4 * g + j] * f;
        *reinterpret_cast<f32x4*>(dst + 8 * g + 4 * h) = v;
    }
}

// ---- dropout on the probabilities (philox.h): m_ij s per score of a 32 x 32 tile ------------------------------------------------------
// query on the lane (the forward and the dQ pass): registers 4 n ... 4 n + 3 are four consecutive keys k0 + 8 n + 4 h + (0 ... 3) of
// query i, so one call gives the four words of a register group
__device__ __forceinline__ void drop_factors_t(float (&ms)[16], const DropArgs& d, int k0, int i, int bh, int h) {
    const DropKey key(d);
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const PhiloxWords w = drop_attn_words(key, (uint32_t)(k0 >> 2) + 2 * n + h, (uint32_t)i, (uint32_t)bh);
#pragma unroll
        for (int j = 0; j < 4; ++j) ms[4 * n + j] = drop_ms(w.w[j], d);
    }
}
__device__ __forceinline__ void drop_scores_t(f32x16& s, const DropArgs& d, int k0, int i, int bh, int h) {
    float ms[16];
    drop_factors_t(ms, d, k0, i, bh, h);
#pragma unroll
    for (int n = 0; n < 16; ++n) s[n] *= ms[n];
}

// One tile of the forward's running softmax, both forward kernels': s holds the products of the keys k0 + acc_row(i, h) with the lane's
// query w.row0 + w.r and leaves as the P V operand, exp(s - m_run) (DROP: times m s); m and l are the query's running maximum and sum
// (of the undropped probabilities).  Returns alpha = exp(m_old - m_new), what the query's O so far is rescaled by.
template <bool DROP, bool WIN, bool REL, int DH>
__device__ __forceinline__ float softmax_tile(f32x16& s, float& m, float& l, const MhsaParams& p, const WaveTile<DH>& w, int k0,
                                              const RelWalk<REL>& rw) {
    const int t = p.t, q0 = w.row0, r = w.r, h = w.h;
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int j = k0 + acc_row(i, h);
        if constexpr (REL)
            s[i] = j < t && in_window(q0 + r, j, p.wl, p.wr) ? s[i] * p.scale + rw.at(k0, i, h, r) : -INFINITY;
        else
            s[i] = j < t && (!WIN || in_window(q0 + r, j, p.wl, p.wr)) ? s[i] * p.scale : -INFINITY;
        mx = fmaxf(mx, s[i]);
    }
    mx = fmaxf(mx, xor32(mx));
    // plain: finite from the first tile on (key k0 is always inside the clip).  WIN: a query's first visited tiles can lie wholly
    // left of its window (left = 3, queries 32 ... 63 start at key tile 0, where query 40 has no key): the maximum is still -inf
    // there, and the reference point 0 makes alpha and every probability exp(-inf) = 0 instead of exp(-inf + inf)
    const float mx2 = fmaxf(m, mx);
    const float mn = WIN && mx2 == -INFINITY ? 0.f : mx2;
    const float alpha = expf(m - mn);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { s[i] = expf(s[i] - mn); sum += s[i]; }
    sum += xor32(sum);
    l = l * alpha + sum;
    m = WIN ? mx2 : mn;
    if (DROP) drop_scores_t(s, p.drop, k0, q0 + r, w.bh, h);
    return alpha;
}
// key on the lane (the dK / dV pass): registers 4 n ... 4 n + 3 are four consecutive queries q0 + 8 n + 4 h + (0 ... 3) of key j = k0 + r,
// and the four lanes of a quad share j >> 2: lane L of the quad makes the call of query q0 + 8 n + 4 h + L, and lane j & 3 takes word
// j & 3 of each of the quad's four calls (quad permutes; every lane of the wave is live here)
__device__ __forceinline__ void drop_factors_k(float (&ms)[16], const DropArgs& d, int j, int q0, int bh, int h) {
    const DropKey key(d);
    const int L = j & 3;                               // (k0 is a multiple of 32: j & 3 is the lane's place in its quad)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const PhiloxWords w = drop_attn_words(key, (uint32_t)j >> 2, (uint32_t)(q0 + 8 * n + 4 * h + L), (uint32_t)bh);
        ms[4 * n + 0] = drop_ms(quad_word<0>(w, L), d);
        ms[4 * n + 1] = drop_ms(quad_word<1>(w, L), d);
        ms[4 * n + 2] = drop_ms(quad_word<2>(w, L), d);
        ms[4 * n + 3] = drop_ms(quad_word<3>(w, L), d);
    }
}

template <typename T, int DH, bool DROP, bool WIN, bool REL = false>
__global__ __launch_bounds__(64 * MHSA_WAVES) void mhsa_fwd_kernel(MhsaParams p) {
    static_assert(WIN || !REL, "REL is instantiated with WIN only");
    const WaveTile<DH> w(p);
    const int t = p.t, q0 = w.row0, r = w.r, h = w.h, C = w.C, ld = w.ld;
    if (q0 >= t) return;                               // (no barrier in this kernel)
    const float* __restrict__ base = p.qkv + (size_t)w.b * t * ld + w.g * DH;
    const int qr = q0 + r < t ? q0 + r : t - 1;
    RowFrag<T, DH> qf;
    qf.load(base + qr * ld, h);
    f32x16 o[DH / 32];
#pragma unroll
    for (int cb = 0; cb < DH / 32; ++cb) o[cb] = (f32x16){};
    float m = -INFINITY, l = 0.f;
    // the next tile's K rows and V columns are loaded while this tile is computed (registers, no LDS)
    RowFrag<T, DH> kn;
    float vn[DH / 32][16];
    const TileRange kt = WIN ? mhsa_win_range(q0, MHSA_QT, t, p.wl, p.wr) : TileRange{0, t};
    kn.load(base + C + (kt.lo + r < t ? kt.lo + r : t - 1) * ld, h);
#pragma unroll
    for (int cb = 0; cb < DH / 32; ++cb) load_col(vn[cb], base + 2 * C + cb * 32 + r, ld, kt.lo, t, h);
    RelWalk<REL> rw(w.wave, kt.lo);
    for (int k0 = kt.lo; k0 < kt.hi; k0 += 32) {
        rw.tile(p, w.g, q0, k0, kt.hi, 1, w.lane);
        const RowFrag<T, DH> kf = kn;
        float va[DH / 32][16];
#pragma unroll
        for (int cb = 0; cb < DH / 32; ++cb)
#pragma unroll
            for (int i = 0; i < 16; ++i) va[cb][i] = vn[cb][i];
        if (k0 + 32 < kt.hi) {
            const int kr = k0 + 32 + r < t ? k0 + 32 + r : t - 1;
            kn.load(base + C + kr * ld, h);
#pragma unroll
            for (int cb = 0; cb < DH / 32; ++cb) load_col(vn[cb], base + 2 * C + cb * 32 + r, ld, k0 + 32, t, h);
        }
        f32x16 s = mm_rows<T, DH>(kf, qf);             // s[key][query]
        const float alpha = softmax_tile<DROP, WIN, REL>(s, m, l, p, w, k0, rw);
#pragma unroll
        for (int cb = 0; cb < DH / 32; ++cb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) o[cb][i] *= alpha;
            MmAx<T>::run(o[cb], va[cb], s);
        }
    }
    if (q0 + r < t) {
        const float inv = 1.f / l;
        float* __restrict__ dst = p.out + ((size_t)w.b * t + q0 + r) * C + w.g * DH;
#pragma unroll
        for (int cb = 0; cb < DH / 32; ++cb) store_tile_t(dst + cb * 32, o[cb], inv, h);
        if (p.lse_out != nullptr && h == 0) p.lse_out[(size_t)w.bh * t + q0 + r] = m + logf(l);
    }
}

// The bf16 forward with the K / V tiles staged ONCE per workgroup: the 256 threads load a tile of 32 keys with whole-row 16-byte loads
// (the next tile's while this one is computed), round it to bf16 and write K row-major (pitch dh + 8: conflict-free 16-byte reads of the
// A fragments) and V transposed (Vt[c][key], pitch 36: a lane's eight keys of a k-step are two 8-byte reads) into one of two LDS
// buffers, one barrier per tile.  Same values, same MFMA order and so the same bits as the register-fed kernel above, which the fp32
// mode keeps; waves whose 32 queries lie past the clip take part in the staging and the barriers only.
template <int DH, bool DROP, bool WIN, bool REL = false>
__global__ __launch_bounds__(64 * MHSA_WAVES) void mhsa_fwd_lds_kernel(MhsaParams p) {
    static_assert(WIN || !REL, "REL is instantiated with WIN only");
    constexpr int KP = DH + 8, VP = 36, NL = DH / 32, RQ = DH / 4;       // NL 16-byte loads of K and of V per thread and tile
    __shared__ __attribute__((aligned(16))) bf16_t ks[2][32 * KP];
    __shared__ __attribute__((aligned(16))) bf16_t vt[2][DH * VP];
    const WaveTile<DH> w(p);
    const int tid = threadIdx.x, t = p.t, q0 = w.row0, r = w.r, h = w.h, C = w.C, ld = w.ld;
    const bool active = q0 < t;
    const float* __restrict__ base = p.qkv + (size_t)w.b * t * ld + w.g * DH;
    const int qr = q0 + r < t ? q0 + r : t - 1;
    RowFrag<bf16_t, DH> qf;
    qf.load(base + qr * ld, h);
    f32x4 kreg[NL], vreg[NL];
    auto gload = [&](int k0) {
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int idx = tid + 256 * n, row = idx / RQ, c4 = (idx % RQ) * 4;
            const int rr = k0 + row < t ? k0 + row : t - 1;
            kreg[n] = *reinterpret_cast<const f32x4*>(base + C + rr * ld + c4);
            vreg[n] = *reinterpret_cast<const f32x4*>(base + 2 * C + rr * ld + c4);
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int idx = tid + 256 * n, row = idx / RQ, c4 = (idx % RQ) * 4;
            bf16x4 kb;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                kb[i] = (bf16_t)kreg[n][i];
                vt[buf][(c4 + i) * VP + row] = (bf16_t)vreg[n][i];
            }
            *reinterpret_cast<bf16x4*>(&ks[buf][row * KP + c4]) = kb;
        }
    };
    f32x16 o[NL];
#pragma unroll
    for (int cb = 0; cb < NL; ++cb) o[cb] = (f32x16){};
    float m = -INFINITY, l = 0.f;
    // WIN: the workgroup stages the union of its waves' ranges (the range of its 128 queries: wg, the same in every thread); a wave
    // computes on the tiles of its own range (mine) and only stages and waits on the others
    const TileRange wg = WIN ? mhsa_win_range(w.tile * MHSA_WAVES * MHSA_QT, MHSA_WAVES * MHSA_QT, t, p.wl, p.wr) : TileRange{0, t};
    const TileRange mine = WIN && active ? mhsa_win_range(q0, MHSA_QT, t, p.wl, p.wr) : TileRange{0, t};
    gload(wg.lo);
    lstore(0);
    __syncthreads();
    RelWalk<REL> rw(w.wave, mine.lo);                  // (the wave's own walk)
    for (int k0 = wg.lo, it = 0; k0 < wg.hi; k0 += 32, ++it) {
        const int cur = it & 1;
        const bool more = k0 + 32 < wg.hi;             // (the same in every thread: the barrier below is uniform)
        if (more) gload(k0 + 32);
        if (active && (!WIN || (k0 >= mine.lo && k0 < mine.hi))) {
            rw.tile(p, w.g, q0, k0, mine.hi, 1, w.lane);
            RowFrag<bf16_t, DH> kf;
#pragma unroll
            for (int s = 0; s < DH / 16; ++s) kf.f[s] = *reinterpret_cast<const bf16x8*>(&ks[cur][r * KP + 16 * s + 8 * h]);
            f32x16 s = mm_rows<bf16_t, DH>(kf, qf);    // s[key][query]
            const float alpha = softmax_tile<DROP, WIN, REL>(s, m, l, p, w, k0, rw);
#pragma unroll
            for (int cb = 0; cb < NL; ++cb) {
#pragma unroll
                for (int i = 0; i < 16; ++i) o[cb][i] *= alpha;
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const bf16_t* vrow = &vt[cur][(cb * 32 + r) * VP + 16 * s2 + 4 * h];
                    const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vrow), hi = *reinterpret_cast<const bf16x4*>(vrow + 8);
                    bf16x8 af, pb;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { af[j] = lo[j]; af[4 + j] = hi[j]; }
#pragma unroll
                    for (int j = 0; j < 8; ++j) pb[j] = (bf16_t)s[8 * s2 + j];
                    o[cb] = mfma(af, pb, o[cb]);
                }
            }
        }
        if (more) lstore(cur ^ 1);
        __syncthreads();
    }
    if (active && q0 + r < t) {
        const float inv = 1.f / l;
        float* __restrict__ dst = p.out + ((size_t)w.b * t + q0 + r) * C + w.g * DH;
#pragma unroll
        for (int cb = 0; cb < NL; ++cb) store_tile_t(dst + cb * 32, o[cb], inv, h);
        if (p.lse_out != nullptr && h == 0) p.lse_out[(size_t)w.bh * t + q0 + r] = m + logf(l);
    }
}

// D[b][g][i] = sum_c dctx[b*t+i][g*dh + c] * ctx[..]: one thread per (row, head), columns ascending
__global__ __launch_bounds__(256) void mhsa_rowdot_kernel(MhsaParams p, int B, int dh) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n = (size_t)B * p.t * p.H;
    if (idx >= n) return;
    const size_t row = idx / p.H;
    const int g = (int)(idx % p.H);
    const size_t b = row / p.t, i = row % p.t;
    const float* __restrict__ x = p.dctx + row * (size_t)(p.H * dh) + g * dh;
    const float* __restrict__ y = p.ctx + row * (size_t)(p.H * dh) + g * dh;
    float acc = 0.f;
    for (int c = 0; c < dh; c += 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + c), bb = *reinterpret_cast<const f32x4*>(y + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = fmaf(a[j], bb[j], acc);
    }
    p.D[(b * p.H + g) * p.t + i] = acc;
}

// pass 2 of the backward: the wave owns 32 keys (on the lane) and loops over the query tiles -> dK, dV
template <typename T, int DH, bool DROP, bool WIN, bool REL = false>
__global__ __launch_bounds__(64 * MHSA_WAVES) void mhsa_bwd_kv_kernel(MhsaParams p) {
    static_assert(WIN || !REL, "REL is instantiated with WIN only");
    const WaveTile<DH> w(p);
    const int t = p.t, k0 = w.row0, r = w.r, h = w.h, C = w.C, ld = w.ld;
    if (k0 >= t) return;
    const float* __restrict__ base = p.qkv + (size_t)w.b * t * ld + w.g * DH;
    const float* __restrict__ dbase = p.dctx + (size_t)w.b * t * C + w.g * DH;
    const float* __restrict__ lse = p.lse + (size_t)w.bh * t;
    const float* __restrict__ D = p.D + (size_t)w.bh * t;
    const int kr = k0 + r < t ? k0 + r : t - 1;
    RowFrag<T, DH> kf, vf;
    kf.load(base + C + kr * ld, h);
    vf.load(base + 2 * C + kr * ld, h);
    f32x16 dk[DH / 32], dv[DH / 32];
#pragma unroll
    for (int cb = 0; cb < DH / 32; ++cb) { dk[cb] = (f32x16){}; dv[cb] = (f32x16){}; }
    // the next tile's Q / dctx rows, lse and D are loaded while this tile is computed; this tile's Q / dctx columns at its top
    RowFrag<T, DH> qn, dn;
    float ln[16], Dn[16];
    auto load_rows = [&](int q0) {
        const int qr = q0 + r < t ? q0 + r : t - 1;
        qn.load(base + qr * ld, h);
        dn.load(dbase + qr * C, h);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int q = q0 + acc_row(i, h);
            const int qc = q < t ? q : t - 1;
            ln[i] = lse[qc];
            Dn[i] = D[qc];
        }
    };
    const TileRange qt = WIN ? mhsa_win_range(k0, MHSA_QT, t, p.wr, p.wl) : TileRange{0, t};
    // WIN: p and dS of a cell outside the window (or the clip) are 0 by select; exp(s - lse) is not taken there (lse covers the window
    // only, so it can overflow)
    auto live = [&](int q) { return q < t && (!WIN || (k0 + r < t && in_window(q, k0 + r, p.wl, p.wr))); };
    load_rows(qt.lo);
    RelWalk<REL> rw(w.wave, qt.lo);
    // what the scaled product of cell (query q0 + acc_row(i, h), key k0 + r) is reduced by under the exponential: lse_i, REL: lse_i - rel
    // (the expression keeps the shape scale * s - c of the other instantiations: a zero table gives their bits whatever is contracted)
    auto under = [&](float l, int q0, int i) {
        if constexpr (REL) return l - rw.at(q0, i, h, r);
        else return l;
    };
    for (int q0 = qt.lo; q0 < qt.hi; q0 += 32) {
        rw.tile(p, w.g, k0, q0, qt.hi, -1, w.lane);
        const RowFrag<T, DH> qf = qn, df = dn;
        float lc[16], Dc[16], qa[DH / 32][16], da[DH / 32][16];
#pragma unroll
        for (int i = 0; i < 16; ++i) { lc[i] = ln[i]; Dc[i] = Dn[i]; }
#pragma unroll
        for (int cb = 0; cb < DH / 32; ++cb) {
            load_col(da[cb], dbase + cb * 32 + r, C, q0, t, h);
            load_col(qa[cb], base + cb * 32 + r, ld, q0, t, h);
        }
        if (q0 + 32 < qt.hi) load_rows(q0 + 32);
        f32x16 s = mm_rows<T, DH>(qf, kf);             // s[query][key]
        f32x16 dp = mm_rows<T, DH>(df, vf);
        float ms[16];
        if constexpr (DROP) drop_factors_k(ms, p.drop, k0 + r, q0, w.bh, h);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const bool in = live(q0 + acc_row(i, h));
            const float pr = in ? expf(s[i] * p.scale - under(lc[i], q0, i)) : 0.f;
            if constexpr (DROP) {
                s[i] = pr * ms[i];                       // p~ for dV
                dp[i] = !WIN || in ? pr * (dp[i] * ms[i] - Dc[i]) : 0.f;
            } else {
                s[i] = pr;
                dp[i] = !WIN || in ? pr * (dp[i] - Dc[i]) : 0.f;
            }
        }
#pragma unroll
        for (int cb = 0; cb < DH / 32; ++cb) {
            MmAx<T>::run(dv[cb], da[cb], s);
            MmAx<T>::run(dk[cb], qa[cb], dp);
        }
    }
    if (k0 + r < t) {
        float* __restrict__ dst = p.out + ((size_t)w.b * t + k0 + r) * ld + w.g * DH;
#pragma unroll
        for (int cb = 0; cb < DH / 32; ++cb) {
            store_tile_t(dst + C + cb * 32, dk[cb], p.scale, h);
            store_tile_t(dst + 2 * C + cb * 32, dv[cb], 1.f, h);
        }
    }
}

// pass 3: the wave owns 32 queries (on the lane) and loops over the key tiles -> dQ
template <typename T, int DH, bool DROP, bool WIN, bool REL = false>
__global__ __launch_bounds__(64 * MHSA_WAVES) void mhsa_bwd_q_kernel(MhsaParams p) {
    static_assert(WIN || !REL, "REL is instantiated with WIN only");
    const WaveTile<DH> w(p);
    const int t = p.t, q0 = w.row0, lane = w.lane, r = w.r, h = w.h, C = w.C, ld = w.ld;
    if (q0 >= t) return;
    const float* __restrict__ base = p.qkv + (size_t)w.b * t * ld + w.g * DH;
    const float* __restrict__ dbase = p.dctx + (size_t)w.b * t * C + w.g * DH;
    const int qr = q0 + r < t ? q0 + r : t - 1;
    const float lse = p.lse[(size_t)w.bh * t + qr], Dq = p.D[(size_t)w.bh * t + qr];
    RowFrag<T, DH> qf, df;
    qf.load(base + qr * ld, h);
    df.load(dbase + qr * C, h);
    f32x16 dq[DH / 32];
#pragma unroll
    for (int cb = 0; cb < DH / 32; ++cb) dq[cb] = (f32x16){};
    // the next tile's K / V rows are loaded while this tile is computed; this tile's K columns at its top
    RowFrag<T, DH> kn, vn;
    auto load_rows = [&](int k0) {
        const int kr = k0 + r < t ? k0 + r : t - 1;
        kn.load(base + C + kr * ld, h);
        vn.load(base + 2 * C + kr * ld, h);
    };
    const TileRange kt = WIN ? mhsa_win_range(q0, MHSA_QT, t, p.wl, p.wr) : TileRange{0, t};
    load_rows(kt.lo);
    RelWalk<REL> rw(w.wave, kt.lo);
    // REL: the wave's partial of drel.  Slot x of its workspace row is distance (kt.lo - q0 - 31) + x; a tile at k0 meets slots
    // (k0 - kt.lo) + 0 ... 62, lane X of `carry` holding slot (k0 - kt.lo) + X: the lower 32 are complete after this tile and are
    // stored, the upper 31 move down to meet the next tile; the row ends with the last tile's upper half.
    float carry = 0.f;
    float* __restrict__ wsrow = nullptr;
    if constexpr (REL) wsrow = p.relws + ((size_t)blockIdx.x * MHSA_WAVES + w.wave) * p.relspan;
    for (int k0 = kt.lo; k0 < kt.hi; k0 += 32) {
        rw.tile(p, w.g, q0, k0, kt.hi, 1, lane);
        const RowFrag<T, DH> kf = kn, vf = vn;
        float ka[DH / 32][16];
#pragma unroll
        for (int cb = 0; cb < DH / 32; ++cb) load_col(ka[cb], base + C + cb * 32 + r, ld, k0, t, h);
        if (k0 + 32 < kt.hi) load_rows(k0 + 32);
        f32x16 s = mm_rows<T, DH>(kf, qf);             // s[key][query]
        f32x16 dp = mm_rows<T, DH>(vf, df);
        if (DROP) {
            float ms[16];
            drop_factors_t(ms, p.drop, k0, q0 + r, w.bh, h);
#pragma unroll
            for (int i = 0; i < 16; ++i) dp[i] *= ms[i];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int j = k0 + acc_row(i, h);
            const bool in = j < t && (!WIN || (q0 + r < t && in_window(q0 + r, j, p.wl, p.wr)));   // (select: see mhsa_bwd_kv_kernel)
            float lr = lse;                             // REL: lse - rel, the expression's shape kept (see mhsa_bwd_kv_kernel)
            if constexpr (REL) lr = lse - rw.at(k0, i, h, r);
            const float pr = in ? expf(s[i] * p.scale - lr) : 0.f;
            dp[i] = !WIN || in ? pr * (dp[i] - Dq) : 0.f;
        }
        if constexpr (REL) {
            // the tile's 63 diagonal sums of dS, diagonal X = (key row) - (query lane) + 31 on lane X: register i holds key rows
            // b and b + 4 (the two half-waves), so lane X takes it from lane b + 31 - X of the lower and b + 35 - X of the upper
            // half where those exist; 32 reads in a fixed order, no two lanes ever add into one place
            float v = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int bi = (i & 3) + 8 * (i >> 2);
                const int r0 = bi + 31 - lane, r1 = bi + 35 - lane;
                const float a0 = __shfl(dp[i], r0 & 31, 64), a1 = __shfl(dp[i], 32 + (r1 & 31), 64);
                v += r0 >= 0 && r0 < 32 ? a0 : 0.f;
                v += r1 >= 0 && r1 < 32 ? a1 : 0.f;
            }
            const float up = __shfl(carry, (lane + 32) & 63, 64);
            carry = lane < 32 ? v + up : v;
            if (lane < 32) wsrow[(k0 - kt.lo) + lane] = carry;
        }
#pragma unroll
        for (int cb = 0; cb < DH / 32; ++cb) MmAx<T>::run(dq[cb], ka[cb], dp);
    }
    if constexpr (REL) {
        if (lane >= 32) wsrow[((kt.hi - kt.lo + MHSA_QT - 1) & ~(MHSA_QT - 1)) + lane - 32] = carry;
    }
    if (q0 + r < t) {
        float* __restrict__ dst = p.out + ((size_t)w.b * t + q0 + r) * ld + w.g * DH;
#pragma unroll
        for (int cb = 0; cb < DH / 32; ++cb) store_tile_t(dst + cb * 32, dq[cb], p.scale, h);
    }
}

// ---- relative-position bias: the workspace rows of the dQ pass and their reduction ---------------------------------------------------
// floats of a wave's row: 32 per visited tile and 32 for the last tile's upper half, the largest over the waves of a clip
inline int rel_span(int t, int wl, int wr) {
    int span = 0;
    for (int q0 = 0; q0 < t; q0 += MHSA_QT) {
        const TileRange kt = mhsa_win_range(q0, MHSA_QT, t, wl, wr);
        const int n = ((kt.hi - kt.lo + MHSA_QT - 1) & ~(MHSA_QT - 1)) + MHSA_QT;
        span = n > span ? n : span;
    }
    return span;
}

// drel[g][d + t - 1] = sum over the clips and the waves of their partials of distance d, in fp64: 64 distances x REL_RED_LANES clip lanes
// per workgroup, each clip lane its clips (stride REL_RED_LANES) and their waves in ascending order, then the lanes in a fixed tree,
// rounded once
#define REL_RED_LANES 16
__global__ __launch_bounds__(64 * REL_RED_LANES) void mhsa_rel_reduce_kernel(const float* __restrict__ ws, float* __restrict__ drel, int B, int t, int H,
                                                              int ntile, int relspan, int wl, int wr) {
    __shared__ double sh[REL_RED_LANES][64];
    const int cl = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int di = blockIdx.x * 64 + cl, g = blockIdx.y, d = di - (t - 1);
    double s = 0.0;
    if (di < 2 * t - 1)
        for (int b = ry; b < B; b += REL_RED_LANES)
            for (int w = 0; w * MHSA_QT < t; ++w) {
                const int q0 = w * MHSA_QT;
                const TileRange kt = mhsa_win_range(q0, MHSA_QT, t, wl, wr);
                const int slot = d - (kt.lo - q0 - 31);
                const int n = ((kt.hi - kt.lo + MHSA_QT - 1) & ~(MHSA_QT - 1)) + MHSA_QT;
                if (slot >= 0 && slot < n) s += (double)ws[(((size_t)b * H + g) * ((size_t)ntile * MHSA_WAVES) + w) * relspan + slot];
            }
    sh[ry][cl] = s;
    __syncthreads();
#pragma unroll
    for (int n = REL_RED_LANES / 2; n >= 1; n >>= 1) {          // lane ry += lane ry + n: the same tree on every run
        if (ry < n) sh[ry][cl] += sh[ry + n][cl];
        __syncthreads();
    }
    if (ry == 0 && di < 2 * t - 1) drel[(size_t)g * (2 * t - 1) + di] = (float)sh[0][cl];
}

// rel[g][x] = w[g][map[x]], x = d + t - 1 (a bit copy; the map was checked on the host: sed_relpos_map_check)
__global__ __launch_bounds__(256) void relpos_expand_kernel(const float* __restrict__ w, const int* __restrict__ map, float* __restrict__ rel,
                                                            int nb, int n) {
    const int x = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
    if (x >= n) return;
    int m = map[x];
    m = m < 0 ? 0 : m >= nb ? nb - 1 : m;              // (never taken for a checked map: no read outside w whatever the map holds)
    rel[(size_t)g * n + x] = w[(size_t)g * nb + m];
}

// dw[g][b] = sum over the distances x with map[x] = b of drel[g][x], in fp64, ascending x, rounded once; 0 for an empty bucket
__global__ __launch_bounds__(256) void relpos_fold_kernel(const float* __restrict__ drel, const int* __restrict__ map, float* __restrict__ dw,
                                                          int nb, int n) {
    // the workgroup stages 1024 distances at a time in LDS (coalesced loads, the tail padded with bucket -1); every thread scans them for
    // its bucket in ascending order, 16 at a time through 16-byte LDS reads issued together
    __shared__ __attribute__((aligned(16))) int ms[1024];
    __shared__ __attribute__((aligned(16))) float ds[1024];
    const int b = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
    double s = 0.0;
    for (int x0 = 0; x0 < n; x0 += 1024) {
        for (int x = threadIdx.x; x < 1024; x += 256) {
            const bool in = x0 + x < n;
            ms[x] = in ? map[x0 + x] : -1;
            ds[x] = in ? drel[(size_t)g * n + x0 + x] : 0.f;
        }
        __syncthreads();
        const int m = n - x0 < 1024 ? n - x0 : 1024;
        for (int x = 0; x < m; x += 16) {
            int4 mm[4];
            f32x4 dd[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { mm[k] = *reinterpret_cast<const int4*>(&ms[x + 4 * k]); dd[k] = *reinterpret_cast<const f32x4*>(&ds[x + 4 * k]); }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s += mm[k].x == b ? (double)dd[k][0] : 0.0;
                s += mm[k].y == b ? (double)dd[k][1] : 0.0;
                s += mm[k].z == b ? (double)dd[k][2] : 0.0;
                s += mm[k].w == b ? (double)dd[k][3] : 0.0;
            }
        }
        __syncthreads();
    }
    if (b < nb) dw[(size_t)g * nb + b] = (float)s;
}

int mhsa_check(int dtype, int B, int t, int H, int dh, long long* nblocks, int* ntile) {
    SED_REQUIRE(dtype == SED_F32 || dtype == SED_BF16, "dtype must be SED_F32 or SED_BF16");
    SED_REQUIRE(B > 0 && t > 0 && H > 0, "sizes must be positive");
    SED_REQUIRE(dh == 32 || dh == 64, "head width must be 32 or 64");
    SED_REQUIRE((long long)t * 3 * H * dh * 4 < (1ll << 31), "a clip's qkv rows must stay below 2 GiB (32-bit offsets inside a clip)");
    *ntile = cdiv(t, MHSA_QT * MHSA_WAVES);
    *nblocks = (long long)B * H * *ntile;
    SED_REQUIRE(*nblocks < (1ll << 31), "too many workgroups");
    return 0;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// ---- the options of a core launch: dropout, window and table, as every entry hands them to the two launchers ------------------------
// drop.thr = 0 (p below 2^-33: every cell kept, s = 1 exactly) is no dropout by definition and takes the DROP = false instantiation, so
// p = 0 gives the plain entry's bits whatever the compiler contracts where.  win: a bounded side, or a table (both sides unbounded is a
// valid window for the REL kernels: every tile is visited and the select never masks); without either the launch is the WIN = false
// instantiation, plain or DROP.
struct MhsaOpts {
    DropArgs drop;
    bool win;
    int wl, wr;          // the sides, clamped to t - 1
    const float* rel;
    float* drel;
};

// a side clamped to t - 1: one that reaches the clip's end from every query is unbounded
inline int mhsa_win_side(int side, int t) {
    const int cap = t > 0 ? t - 1 : 0;
    return side < cap ? side : cap;
}

// p = 0: no dropout, rng may be NULL
int mhsa_opts(MhsaOpts* o, int t, int left, int right, float p, const uint32_t* rng, uint32_t stream_id, const float* rel, float* drel) {
    SED_REQUIRE(left >= 0 && right >= 0, "the window sides left and right must be >= 0");
    if (int rc = drop_require_args(p, rng, stream_id, &o->drop)) return rc;
    SED_REQUIRE(o->drop.thr == 0 || rng != nullptr, "the dropout state rng is required when p > 0");
    o->wl = mhsa_win_side(left, t);
    o->wr = mhsa_win_side(right, t);
    const int cap = mhsa_win_side(SED_WIN_UNBOUNDED, t);
    o->win = rel != nullptr || o->wl != cap || o->wr != cap;
    o->rel = rel;
    o->drel = drel;
    return 0;
}

// f(MhsaKernel<T, DH, DROP, WIN, REL>{}) for the instantiation of (dtype, dh) and the options; REL comes with WIN only
template <typename T_, int DH, bool DROP, bool WIN, bool REL> struct MhsaKernel {
    using T = T_;
    static constexpr int dh = DH;
    static constexpr bool drop = DROP, win = WIN, rel = REL;
};
template <typename F> void mhsa_dispatch(int dtype, int dh, const MhsaOpts& o, F f) {
    auto by_size = [&](auto drop, auto win, auto rel) {
        constexpr bool D = decltype(drop)::value, W = decltype(win)::value, R = decltype(rel)::value;
        if (dtype == SED_BF16) {
            if (dh == 32) f(MhsaKernel<bf16_t, 32, D, W, R>{});
            else f(MhsaKernel<bf16_t, 64, D, W, R>{});
        } else {
            if (dh == 32) f(MhsaKernel<float, 32, D, W, R>{});
            else f(MhsaKernel<float, 64, D, W, R>{});
        }
    };
    auto by_drop = [&](auto win, auto rel) {
        if (o.drop.thr != 0) by_size(std::true_type{}, win, rel);
        else by_size(std::false_type{}, win, rel);
    };
    if (o.rel != nullptr) by_drop(std::true_type{}, std::true_type{});
    else if (o.win) by_drop(std::true_type{}, std::false_type{});
    else by_drop(std::false_type{}, std::false_type{});
}

int mhsa_fwd_launch(int dtype, const float* qkv, float* ctx, float* lse, int B, int t, int H, int dh, const MhsaOpts& o, void* stream) {
    long long nb; int ntile;
    if (int rc = mhsa_check(dtype, B, t, H, dh, &nb, &ntile)) return rc;
    SED_REQUIRE(qkv != nullptr && ctx != nullptr, "qkv and ctx are required");
    SED_REQUIRE(aligned16(qkv) && aligned16(ctx), "qkv and ctx must be 16-byte aligned");
    MhsaParams p = {};
    p.qkv = qkv; p.out = ctx; p.lse_out = lse; p.t = t; p.H = H; p.ntile = ntile; p.scale = 1.f / sqrtf((float)dh);
    p.drop = o.drop;
    p.wl = o.wl; p.wr = o.wr;
    p.rel = o.rel;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nb), block(64 * MHSA_WAVES);
    mhsa_dispatch(dtype, dh, o, [&](auto k) {
        using K = decltype(k);
        if constexpr (std::is_same_v<typename K::T, bf16_t>) mhsa_fwd_lds_kernel<K::dh, K::drop, K::win, K::rel><<<grid, block, 0, st>>>(p);
        else mhsa_fwd_kernel<float, K::dh, K::drop, K::win, K::rel><<<grid, block, 0, st>>>(p);
    });
    SED_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" int sed_mhsa_fwd(int dtype, const float* qkv, float* ctx, float* lse, int B, int t, int H, int dh, void* stream) {
    return mhsa_fwd_launch(dtype, qkv, ctx, lse, B, t, H, dh, MhsaOpts{}, stream);
}

// the dropout twins: p in [0, 1) and the state (required whatever p is), then the plain entry's checks
extern "C" int sed_mhsa_fwd_drop(int dtype, const float* qkv, float* ctx, float* lse, int B, int t, int H, int dh, float p,
                                 const uint32_t* rng, uint32_t stream_id, void* stream) {
    SED_REQUIRE(rng != nullptr, "the dropout state rng is required");
    MhsaOpts o;
    if (int rc = mhsa_opts(&o, t, SED_WIN_UNBOUNDED, SED_WIN_UNBOUNDED, p, rng, stream_id, nullptr, nullptr)) return rc;
    return mhsa_fwd_launch(dtype, qkv, ctx, lse, B, t, H, dh, o, stream);
}

// the windowed entry: one for plain and dropout; both sides unbounded is the attention above and launches its instantiation
extern "C" int sed_mhsa_fwd_win(int dtype, const float* qkv, float* ctx, float* lse, int B, int t, int H, int dh, int left, int right,
                                float p, const uint32_t* rng, uint32_t stream_id, void* stream) {
    MhsaOpts o;
    if (int rc = mhsa_opts(&o, t, left, right, p, rng, stream_id, nullptr, nullptr)) return rc;
    return mhsa_fwd_launch(dtype, qkv, ctx, lse, B, t, H, dh, o, stream);
}

// tiles of 32 x 32 per (clip, head) on which a wave of the pass issues MFMAs: the sum of mhsa_win_range over the waves
extern "C" long long sed_mhsa_win_tiles(int t, int left, int right, int pass) {
    if (t <= 0 || left < 0 || right < 0 || pass < 0 || pass > 2) return -1;
    const int wl = mhsa_win_side(left, t), wr = mhsa_win_side(right, t);
    long long n = 0;
    for (int a0 = 0; a0 < t; a0 += MHSA_QT) {
        const TileRange rg = pass == 1 ? mhsa_win_range(a0, MHSA_QT, t, wr, wl) : mhsa_win_range(a0, MHSA_QT, t, wl, wr);
        n += (rg.hi - rg.lo + MHSA_QT - 1) / MHSA_QT;
    }
    return n;
}

extern "C" size_t sed_mhsa_bwd_ws_floats(int B, int t, int H, int dh) {
    (void)dh;
    if (B <= 0 || t <= 0 || H <= 0) return 0;
    return (size_t)B * t * H;
}

namespace {
int mhsa_bwd_launch(int dtype, const float* qkv, const float* ctx, const float* dctx, const float* lse, float* dqkv,
                    float* workspace, int B, int t, int H, int dh, const MhsaOpts& o, void* stream) {
    long long nb; int ntile;
    if (int rc = mhsa_check(dtype, B, t, H, dh, &nb, &ntile)) return rc;
    SED_REQUIRE(qkv != nullptr && ctx != nullptr && dctx != nullptr && lse != nullptr && dqkv != nullptr && workspace != nullptr,
                "qkv, ctx, dctx, lse, dqkv and the workspace are required");
    SED_REQUIRE(aligned16(qkv) && aligned16(ctx) && aligned16(dctx) && aligned16(dqkv), "qkv, ctx, dctx and dqkv must be 16-byte aligned");
    MhsaParams p = {};
    p.qkv = qkv; p.ctx = ctx; p.dctx = dctx; p.lse = lse; p.out = dqkv; p.D = workspace;
    p.t = t; p.H = H; p.ntile = ntile; p.scale = 1.f / sqrtf((float)dh);
    p.drop = o.drop;
    p.wl = o.wl; p.wr = o.wr;
    if (o.rel != nullptr) {
        p.rel = o.rel;
        p.relws = workspace + (size_t)B * t * H;
        p.relspan = rel_span(t, o.wl, o.wr);
    }
    hipStream_t st = (hipStream_t)stream;
    mhsa_rowdot_kernel<<<(unsigned)cdivz((size_t)B * t * H, 256), 256, 0, st>>>(p, B, dh);
    SED_LAUNCH_CHECK();
    const dim3 grid((unsigned)nb), block(64 * MHSA_WAVES);
    mhsa_dispatch(dtype, dh, o, [&](auto k) {
        using K = decltype(k);
        mhsa_bwd_kv_kernel<typename K::T, K::dh, K::drop, K::win, K::rel><<<grid, block, 0, st>>>(p);
        mhsa_bwd_q_kernel<typename K::T, K::dh, K::drop, K::win, K::rel><<<grid, block, 0, st>>>(p);
    });
    SED_LAUNCH_CHECK();
    if (o.rel != nullptr) {
        mhsa_rel_reduce_kernel<<<dim3((unsigned)cdiv(2 * t - 1, 64), (unsigned)H), 64 * REL_RED_LANES, 0, st>>>(p.relws, o.drel, B, t, H, ntile, p.relspan, o.wl, o.wr);
        SED_LAUNCH_CHECK();
    }
    return 0;
}
}  // namespace

extern "C" int sed_mhsa_bwd(int dtype, const float* qkv, const float* ctx, const float* dctx, const float* lse, float* dqkv,
                            float* workspace, int B, int t, int H, int dh, void* stream) {
    return mhsa_bwd_launch(dtype, qkv, ctx, dctx, lse, dqkv, workspace, B, t, H, dh, MhsaOpts{}, stream);
}

extern "C" int sed_mhsa_bwd_drop(int dtype, const float* qkv, const float* ctx, const float* dctx, const float* lse, float* dqkv,
                                 float* workspace, int B, int t, int H, int dh, float p, const uint32_t* rng, uint32_t stream_id,
                                 void* stream) {
    SED_REQUIRE(rng != nullptr, "the dropout state rng is required");
    MhsaOpts o;
    if (int rc = mhsa_opts(&o, t, SED_WIN_UNBOUNDED, SED_WIN_UNBOUNDED, p, rng, stream_id, nullptr, nullptr)) return rc;
    return mhsa_bwd_launch(dtype, qkv, ctx, dctx, lse, dqkv, workspace, B, t, H, dh, o, stream);
}

extern "C" int sed_mhsa_bwd_win(int dtype, const float* qkv, const float* ctx, const float* dctx, const float* lse, float* dqkv,
                                float* workspace, int B, int t, int H, int dh, int left, int right, float p, const uint32_t* rng,
                                uint32_t stream_id, void* stream) {
    MhsaOpts o;
    if (int rc = mhsa_opts(&o, t, left, right, p, rng, stream_id, nullptr, nullptr)) return rc;
    return mhsa_bwd_launch(dtype, qkv, ctx, dctx, lse, dqkv, workspace, B, t, H, dh, o, stream);
}

// ---- the relative-position entries: the windowed entries' arguments and the per-distance table(s).  Always the WIN = true kernels,
// DROP by thr as above
extern "C" int sed_mhsa_fwd_rel(int dtype, const float* qkv, float* ctx, float* lse, int B, int t, int H, int dh, int left, int right,
                                float p, const uint32_t* rng, uint32_t stream_id, const float* rel, void* stream) {
    MhsaOpts o;
    if (int rc = mhsa_opts(&o, t, left, right, p, rng, stream_id, rel, nullptr)) return rc;
    SED_REQUIRE(rel != nullptr, "the distance table rel is required");
    SED_REQUIRE(aligned4(rel), "rel must be 4-byte aligned");
    return mhsa_fwd_launch(dtype, qkv, ctx, lse, B, t, H, dh, o, stream);
}

extern "C" size_t sed_mhsa_bwd_rel_ws_floats(int B, int t, int H, int dh, int left, int right) {
    long long nb; int ntile;
    if (left < 0 || right < 0 || mhsa_check(SED_F32, B, t, H, dh, &nb, &ntile) != 0) return 0;
    return (size_t)B * t * H + (size_t)nb * MHSA_WAVES * rel_span(t, mhsa_win_side(left, t), mhsa_win_side(right, t));
}

extern "C" int sed_mhsa_bwd_rel(int dtype, const float* qkv, const float* ctx, const float* dctx, const float* lse, float* dqkv,
                                float* workspace, int B, int t, int H, int dh, int left, int right, float p, const uint32_t* rng,
                                uint32_t stream_id, const float* rel, float* drel, void* stream) {
    MhsaOpts o;
    if (int rc = mhsa_opts(&o, t, left, right, p, rng, stream_id, rel, drel)) return rc;
    SED_REQUIRE(rel != nullptr && drel != nullptr, "the distance tables rel and drel are required");
    SED_REQUIRE(aligned4(rel) && aligned4(drel), "rel and drel must be 4-byte aligned");
    return mhsa_bwd_launch(dtype, qkv, ctx, dctx, lse, dqkv, workspace, B, t, H, dh, o, stream);
}

#define SED_RELPOS_MAX_BUCKETS 4096
extern "C" int sed_relpos_map_check(const int* map_host, int nb, int t) {
    SED_REQUIRE(map_host != nullptr, "the bucket map is required");
    SED_REQUIRE(nb >= 1 && nb <= SED_RELPOS_MAX_BUCKETS, "the bucket count must lie in [1, 4096]");
    SED_REQUIRE(t >= 1 && t < (1 << 30), "t must lie in [1, 2^30)");
    for (int x = 0; x < 2 * t - 1; ++x) SED_REQUIRE(map_host[x] >= 0 && map_host[x] < nb, "a bucket map entry lies outside [0, nb)");
    return 0;
}

namespace {
int relpos_check(const void* a, const void* map, const void* b, int H, int nb, int t) {
    SED_REQUIRE(a != nullptr && map != nullptr && b != nullptr, "the table, the map and the output are required");
    SED_REQUIRE(aligned4(a) && aligned4(map) && aligned4(b), "the table, the map and the output must be 4-byte aligned");
    SED_REQUIRE(H >= 1 && H <= 65535, "H must lie in [1, 65535]");
    SED_REQUIRE(nb >= 1 && nb <= SED_RELPOS_MAX_BUCKETS, "the bucket count must lie in [1, 4096]");
    SED_REQUIRE(t >= 1 && t < (1 << 30), "t must lie in [1, 2^30)");
    return 0;
}
}  // namespace

extern "C" int sed_relpos_expand(const float* w, const int* map, float* rel, int H, int nb, int t, void* stream) {
    if (int rc = relpos_check(w, map, rel, H, nb, t)) return rc;
    const int n = 2 * t - 1;
    relpos_expand_kernel<<<dim3((unsigned)cdiv(n, 256), (unsigned)H), 256, 0, (hipStream_t)stream>>>(w, map, rel, nb, n);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_relpos_fold(const float* drel, const int* map, float* dw, int H, int nb, int t, void* stream) {
    if (int rc = relpos_check(drel, map, dw, H, nb, t)) return rc;
    relpos_fold_kernel<<<dim3((unsigned)cdiv(nb, 256), (unsigned)H), 256, 0, (hipStream_t)stream>>>(drel, map, dw, nb, 2 * t - 1);
    SED_LAUNCH_CHECK();
    return 0;
}
