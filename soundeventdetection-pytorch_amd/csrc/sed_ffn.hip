// Self-attention temporal head: the position-wise feed-forward sub-layer of an encoder layer, both products and the activation in
// ONE launch on the matrix pipe, and the elementwise activation backward.  (The rest of the backward is sed_gemm_nt / sed_gemm_tn /
// sed_transpose_shift launches, sed_gru.hip.)
//
//   u = x . w1^T + b1          x [R][C], w1 [D][C], b1 [D]        (the pre-activation, [R][D])
//   a = act(u)                 ReLU: max(u, 0);  GELU (erf form): 0.5 u (1 + erf(u / sqrt 2)) = 0.5 u erfc(-u / sqrt 2)
//   y = a . w2^T + b2          w2 [C][D], b2 [C]                  ([R][C])
// backward of the activation:  du = da act'(u);  ReLU: act' = 1 for u > 0, else 0;  GELU: Phi(u) + u phi(u)
// (tests/ffn_formula.py is the same in float64 numpy.)
//
// Forward: a workgroup is four waves and owns 32 rows; it stages its x tile ONCE in LDS as the MFMA operand image (bf16 in bf16 mode)
// and walks the hidden index in steps of 128.  Within a step wave w computes the 32-hidden x 32-row tile u^T = w1 x^T of hidden units
// [d0 + 32 w, d0 + 32 w + 32) (32x32 MFMA: hidden unit in the accumulator registers, row on the lane, as sed_mhsa.hip has S^T), adds b1,
// stores u (training form only: four consecutive hidden units of a row are one 16-byte store), applies the activation and writes the
// operand image of a to LDS.  After ONE barrier (the a tile is double-buffered) every wave accumulates the 32-column output tiles it owns
// (tile j belongs to wave j % 4: C / 128 rounded up tiles, at most four = 64 accumulator registers at C = 512) over the step's hidden
// units: y^T = w2 a^T with the output column in the registers and the row on the lane again.  The [R][D] hidden tensor reaches global
// memory only as u, and only when asked for; y has the same bits either way (the same instructions in the same order).
// The weights come straight from global memory (they are 2 C D floats and live in L2), the next 32 columns' fragment while the
// current one is multiplied: no packing launch.
//
// dtype: SED_BF16 -- x, w1, w2 and a are rounded to bf16 (nearest even) as operands of v_mfma_f32_32x32x16_bf16; both accumulations,
// the bias adds, the activation, u and y are fp32.  SED_F32 -- the same dataflow on v_mfma_f32_32x32x2_f32 (exact products).
// No atomics, every sum in a fixed order: the same bits on every run.
//
// Ragged last tile: loads of rows past R are clamped to row R - 1 (real data), their results are never stored.
//
// Dropout (the DROP instantiations behind sed_ffn_fwd_drop / sed_ffn_act_bwd_drop; mask m of element (row, hidden unit) and scale
// s = 1 / (1 - p) from philox.h, generated in registers):  a = m s act(u) before it becomes the operand of the second product, u stored
// undropped;  backward  a = m s act(u) (for dw2),  du = da m s act'(u).  A register group of the forward and a 16-byte access of the
// backward are four consecutive hidden units of one row: one Philox call each.  thr = 0 (p = 0) launches the plain instantiation.
#include "common.h"
#include "philox.h"
#include <math.h>

#define FFN_ROWS 32           // rows a workgroup owns
#define FFN_WAVES 4
#define FFN_DSTEP 128         // hidden units per step: 32 per wave
#define FFN_MAX_C 512
#define FFN_MAX_D 4096

namespace {

// row of the 32x32 accumulator that register i of lane half h holds
__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

template <int ACT> __device__ __forceinline__ float act_fwd(float u) {
    if (ACT == SED_ACT_RELU) return u > 0.f ? u : 0.f;
    return 0.5f * u * erfcf(-u * 0.70710678118654752f);        // 1 + erf(z) = erfc(-z): no cancellation for u << 0
}
template <int ACT> __device__ __forceinline__ float act_grad(float u) {
    if (ACT == SED_ACT_RELU) return u > 0.f ? 1.f : 0.f;
    return fmaf(u * 0.3989422804014327f, expf(-0.5f * u * u), 0.5f * erfcf(-u * 0.70710678118654752f));
}

// ---- 32 consecutive columns of one row as the operand of a product summed over the columns -------------------------------------------
// bf16: two k-steps of 16, step s takes columns 16 s + 8 h + j in element j;  fp32: sixteen k-steps of 2, step 4 q + j takes column
// 8 q + 4 h + j (both operands of a product use the same map, so the order of the columns inside the sum is free)
template <typename T> struct Frag;
template <> struct Frag<bf16_t> {
    bf16x8 f[2];
    __device__ __forceinline__ void from_f32(const float* __restrict__ p, int h) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(p + 16 * s + 8 * h);
            const f32x4 b = *reinterpret_cast<const f32x4*>(p + 16 * s + 8 * h + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { f[s][j] = (bf16_t)a[j]; f[s][4 + j] = (bf16_t)b[j]; }
        }
    }
    __device__ __forceinline__ void from_image(const bf16_t* p, int h) {
#pragma unroll
        for (int s = 0; s < 2; ++s) f[s] = *reinterpret_cast<const bf16x8*>(p + 16 * s + 8 * h);
    }
};
template <> struct Frag<float> {
    float f[16];
    __device__ __forceinline__ void from_f32(const float* __restrict__ p, int h) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(p + 8 * q + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; ++j) f[4 * q + j] = a[j];
        }
    }
    __device__ __forceinline__ void from_image(const float* p, int h) { from_f32(p, h); }
};
// acc[row of A][row of B] += sum over the 32 columns: A's row index lands in the accumulator registers, B's on the lane
__device__ __forceinline__ f32x16 mm32(const Frag<bf16_t>& a, const Frag<bf16_t>& b, f32x16 acc) {
#pragma unroll
    for (int s = 0; s < 2; ++s) acc = mfma(a.f[s], b.f[s], acc);
    return acc;
}
__device__ __forceinline__ f32x16 mm32(const Frag<float>& a, const Frag<float>& b, f32x16 acc) {
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = mfma(a.f[s], b.f[s], acc);
    return acc;
}

// four consecutive values of the operand image
__device__ __forceinline__ void put4(bf16_t* dst, const f32x4& v) {
    bf16x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (bf16_t)v[j];
    *reinterpret_cast<bf16x4*>(dst) = o;
}
__device__ __forceinline__ void put4(float* dst, const f32x4& v) { *reinterpret_cast<f32x4*>(dst) = v; }

struct FfnParams {
    const float* x;
    const float* w1;
    const float* b1;
    const float* w2;
    const float* b2;
    float* y;
    float* u;
    size_t R;
    int C, D;
    DropArgs drop;       // the DROP instantiations only
};

template <typename T> constexpr int ffn_pad() { return 16 / (int)sizeof(T); }       // 16 bytes: the 16-byte fragment reads of the 32 rows spread over the banks
template <typename T> static inline size_t ffn_lds_bytes(int C) {
    return ((size_t)2 * FFN_ROWS * (FFN_DSTEP + ffn_pad<T>()) + (size_t)FFN_ROWS * (C + ffn_pad<T>())) * sizeof(T);
}

// TPW: output tiles (32 columns each) per wave = ceil(C / 128)
// DROP: a = m s act(u) with the mask of element (row, hidden unit) (philox.h: a register group is four consecutive hidden units of one
// row, one call); u is stored undropped
template <typename T, int ACT, int TPW, bool DROP>
__global__ __launch_bounds__(64 * FFN_WAVES) void ffn_fwd_kernel(FfnParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int AP = FFN_DSTEP + ffn_pad<T>();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int C = p.C, D = p.D, XP = C + ffn_pad<T>(), NT = C / 32;
    const size_t row0 = (size_t)blockIdx.x * FFN_ROWS;
    T* as = reinterpret_cast<T*>(smem);                            // [2][32][AP]
    T* xs = as + 2 * FFN_ROWS * AP;                                // [32][XP]
    // the x tile, once: whole rows with 16-byte loads, rows past R from row R - 1
    const int q4 = C / 4;
    for (int idx = tid; idx < FFN_ROWS * q4; idx += 64 * FFN_WAVES) {
        const int row = idx / q4, c4 = (idx % q4) * 4;
        const size_t gr = row0 + row < p.R ? row0 + row : p.R - 1;
        put4(xs + row * XP + c4, *reinterpret_cast<const f32x4*>(p.x + gr * C + c4));
    }
    __syncthreads();
    const bool live = row0 + r < p.R;
    const DropKey key = drop_key<DROP>(p.drop);
    f32x16 acc[TPW];
#pragma unroll
    for (int tt = 0; tt < TPW; ++tt) acc[tt] = (f32x16){};
    for (int d0 = 0, it = 0; d0 < D; d0 += FFN_DSTEP, ++it) {
        T* ab = as + (it & 1) * FFN_ROWS * AP;
        const int dw = d0 + 32 * wave;                             // this wave's hidden units (the same in every lane of the wave)
        if (dw < D) {
            const float* __restrict__ w1r = p.w1 + (size_t)(dw + r) * C;
            const T* xr = xs + r * XP;
            f32x16 ut = {};
            Frag<T> wn;
            wn.from_f32(w1r, h);
            for (int c = 0; c < C; c += 32) {
                const Frag<T> wc = wn;
                if (c + 32 < C) wn.from_f32(w1r + c + 32, h);
                Frag<T> xb;
                xb.from_image(xr + c, h);
                ut = mm32(wc, xb, ut);                             // ut[hidden][row]
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int hl = 32 * wave + 8 * g + 4 * h;          // four consecutive hidden units, inside the step
                f32x4 uv, av;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    uv[j] = ut[4 * g + j] + p.b1[d0 + hl + j];
                    av[j] = act_fwd<ACT>(uv[j]);
                }
                if (DROP) {
                    const PhiloxWords w = drop_row_words(key, row0 + r, (uint32_t)(d0 + hl) >> 2);
#pragma unroll
                    for (int j = 0; j < 4; ++j) av[j] *= drop_ms(w.w[j], p.drop);
                }
                if (p.u != nullptr && live) *reinterpret_cast<f32x4*>(p.u + (row0 + r) * D + d0 + hl) = uv;
                put4(ab + r * AP + hl, av);
            }
        }
        __syncthreads();                                           // (uniform: every wave passes every step's barrier)
        const int nch = (D - d0) / 32 < 4 ? (D - d0) / 32 : 4;     // 32-wide chunks of hidden units this step holds
        for (int k = 0; k < nch; ++k) {
            Frag<T> af;
            af.from_image(ab + r * AP + 32 * k, h);
            Frag<T> wf[TPW];
#pragma unroll
            for (int tt = 0; tt < TPW; ++tt) {
                const int tile = wave + FFN_WAVES * tt;
                if (tile < NT) wf[tt].from_f32(p.w2 + (size_t)(32 * tile + r) * D + d0 + 32 * k, h);
            }
#pragma unroll
            for (int tt = 0; tt < TPW; ++tt) {
                const int tile = wave + FFN_WAVES * tt;
                if (tile < NT) acc[tt] = mm32(wf[tt], af, acc[tt]);   // acc[column][row]
            }
        }
    }
    if (live) {
#pragma unroll
        for (int tt = 0; tt < TPW; ++tt) {
            const int tile = wave + FFN_WAVES * tt;
            if (tile < NT) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int col = 32 * tile + 8 * g + 4 * h;
                    f32x4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = acc[tt][4 * g + j] + p.b2[col + j];
                    *reinterpret_cast<f32x4*>(p.y + (row0 + r) * C + col) = v;
                }
            }
        }
    }
}

// a = act(u), du = da * act'(u): every element read before it is written (a may be u, du may be da)
// DROP (the tensors are [R][D], D a multiple of 4, so n % 4 = 0 and four consecutive elements share a row and a call):
// a = m s act(u), du = da m s act'(u)
template <int ACT, bool VEC, bool DROP>
__global__ __launch_bounds__(256) void ffn_act_bwd_kernel(const float* u, const float* da, float* a, float* du, size_t n, int D, DropArgs drop) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const DropKey key = drop_key<DROP>(drop);
    if (VEC) {
        const size_t n4 = n / 4;
        if (i < n4) {
            const f32x4 uv = reinterpret_cast<const f32x4*>(u)[i], dv = reinterpret_cast<const f32x4*>(da)[i];
            f32x4 av, gv;
#pragma unroll
            for (int j = 0; j < 4; ++j) { av[j] = act_fwd<ACT>(uv[j]); gv[j] = dv[j] * act_grad<ACT>(uv[j]); }
            if (DROP) {
                const size_t e = 4 * i;
                const PhiloxWords w = drop_row_words(key, e / (size_t)D, (uint32_t)(e % (size_t)D) >> 2);
#pragma unroll
                for (int j = 0; j < 4; ++j) { const float ms = drop_ms(w.w[j], drop); av[j] *= ms; gv[j] *= ms; }
            }
            reinterpret_cast<f32x4*>(a)[i] = av;
            reinterpret_cast<f32x4*>(du)[i] = gv;
        } else if (i - n4 < n % 4) {                               // the tail, one element per thread
            const size_t e = 4 * n4 + (i - n4);
            const float uv = u[e], dv = da[e];
            a[e] = act_fwd<ACT>(uv);
            du[e] = dv * act_grad<ACT>(uv);
        }
    } else if (i < n) {
        const float uv = u[i], dv = da[i];
        if (DROP) {
            const float ms = drop_row_ms(key, drop, i / (size_t)D, (int)(i % (size_t)D));
            a[i] = act_fwd<ACT>(uv) * ms;
            du[i] = dv * act_grad<ACT>(uv) * ms;
        } else {
            a[i] = act_fwd<ACT>(uv);
            du[i] = dv * act_grad<ACT>(uv);
        }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// [a, a + bytes) and [b, b + bytes) share a byte without being the same range
inline bool partial_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x != y && x < y + bytes && y < x + bytes;
}
inline bool any_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

template <typename T, int ACT, int TPW, bool DROP>
int ffn_launch(const FfnParams& p, hipStream_t st) {
    const size_t lds = ffn_lds_bytes<T>(p.C);
    if (lds > 48 * 1024)
        if (int rc = sed_set_max_lds<ffn_fwd_kernel<T, ACT, TPW, DROP>>(lds)) return rc;
    ffn_fwd_kernel<T, ACT, TPW, DROP><<<(unsigned)cdivz(p.R, FFN_ROWS), 64 * FFN_WAVES, lds, st>>>(p);
    return 0;
}
template <typename T, int ACT, bool DROP>
int ffn_launch_tpw(const FfnParams& p, hipStream_t st) {
    switch (cdiv(p.C / 32, FFN_WAVES)) {
        case 1: return ffn_launch<T, ACT, 1, DROP>(p, st);
        case 2: return ffn_launch<T, ACT, 2, DROP>(p, st);
        case 3: return ffn_launch<T, ACT, 3, DROP>(p, st);
        default: return ffn_launch<T, ACT, 4, DROP>(p, st);
    }
}

template <bool DROP>
int ffn_fwd_entry(int dtype, int act, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                  float* y, float* u, size_t R, int C, int D, const DropArgs& drop, void* stream) {
    SED_REQUIRE(dtype == SED_F32 || dtype == SED_BF16, "dtype must be SED_F32 or SED_BF16");
    SED_REQUIRE(act == SED_ACT_RELU || act == SED_ACT_GELU, "act must be SED_ACT_RELU or SED_ACT_GELU");
    SED_REQUIRE(R > 0 && cdivz(R, FFN_ROWS) < ((size_t)1 << 31), "R must be positive (and below 2^31 tiles of 32 rows)");
    SED_REQUIRE(C > 0 && C % 32 == 0 && C <= FFN_MAX_C, "C must be a multiple of 32, at most 512");
    SED_REQUIRE(D > 0 && D % 32 == 0 && D <= FFN_MAX_D, "D must be a multiple of 32, at most 4096");
    SED_REQUIRE(x != nullptr && w1 != nullptr && b1 != nullptr && w2 != nullptr && b2 != nullptr && y != nullptr,
                "x, w1, b1, w2, b2 and y are required");
    SED_REQUIRE(aligned16(x) && aligned16(w1) && aligned16(w2) && aligned16(y) && aligned16(u), "x, w1, w2, y and u must be 16-byte aligned");
    FfnParams p = {x, w1, b1, w2, b2, y, u, R, C, D, drop};
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (dtype == SED_BF16)
        rc = act == SED_ACT_RELU ? ffn_launch_tpw<bf16_t, SED_ACT_RELU, DROP>(p, st) : ffn_launch_tpw<bf16_t, SED_ACT_GELU, DROP>(p, st);
    else
        rc = act == SED_ACT_RELU ? ffn_launch_tpw<float, SED_ACT_RELU, DROP>(p, st) : ffn_launch_tpw<float, SED_ACT_GELU, DROP>(p, st);
    if (rc) return rc;
    SED_LAUNCH_CHECK();
    return 0;
}

template <bool DROP>
int ffn_act_bwd_entry(int act, const float* u, const float* da, float* a, float* du, size_t n, int D, const DropArgs& drop, void* stream) {
    SED_REQUIRE(act == SED_ACT_RELU || act == SED_ACT_GELU, "act must be SED_ACT_RELU or SED_ACT_GELU");
    SED_REQUIRE(n > 0 && n < ((size_t)1 << 38), "n must be positive (and below 2^38)");
    SED_REQUIRE(u != nullptr && da != nullptr && a != nullptr && du != nullptr, "every pointer is required");
    const size_t bytes = n * sizeof(float);
    SED_REQUIRE(!partial_overlap(a, u, bytes) && !partial_overlap(du, da, bytes), "a may be u and du may be da, exactly: no partial overlap");
    SED_REQUIRE(!any_overlap(a, da, bytes) && !any_overlap(du, u, bytes) && !any_overlap(a, du, bytes),
                "a overlaps da or du, or du overlaps u");
    hipStream_t st = (hipStream_t)stream;
    const bool vec = aligned16(u) && aligned16(da) && aligned16(a) && aligned16(du) && n >= 4;
    if (vec) {
        const unsigned grid = (unsigned)cdivz(n / 4 + n % 4, 256);
        if (act == SED_ACT_RELU) ffn_act_bwd_kernel<SED_ACT_RELU, true, DROP><<<grid, 256, 0, st>>>(u, da, a, du, n, D, drop);
        else ffn_act_bwd_kernel<SED_ACT_GELU, true, DROP><<<grid, 256, 0, st>>>(u, da, a, du, n, D, drop);
    } else {
        const unsigned grid = (unsigned)cdivz(n, 256);
        if (act == SED_ACT_RELU) ffn_act_bwd_kernel<SED_ACT_RELU, false, DROP><<<grid, 256, 0, st>>>(u, da, a, du, n, D, drop);
        else ffn_act_bwd_kernel<SED_ACT_GELU, false, DROP><<<grid, 256, 0, st>>>(u, da, a, du, n, D, drop);
    }
    SED_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int sed_ffn_fwd(int dtype, int act, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                           float* y, float* u, size_t R, int C, int D, void* stream) {
    return ffn_fwd_entry<false>(dtype, act, x, w1, b1, w2, b2, y, u, R, C, D, DropArgs{}, stream);
}

extern "C" int sed_ffn_act_bwd(int act, const float* u, const float* da, float* a, float* du, size_t n, void* stream) {
    return ffn_act_bwd_entry<false>(act, u, da, a, du, n, 4, DropArgs{}, stream);
}

// the dropout twins (philox.h): the plain entry's checks, then p in [0, 1) and the state
extern "C" int sed_ffn_fwd_drop(int dtype, int act, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                                float* y, float* u, size_t R, int C, int D, float p, const uint32_t* rng, uint32_t stream_id,
                                void* stream) {
    SED_REQUIRE(rng != nullptr, "the dropout state rng is required");
    DropArgs d;
    if (int rc = drop_require_args(p, rng, stream_id, &d)) return rc;
    if (d.thr == 0) return ffn_fwd_entry<false>(dtype, act, x, w1, b1, w2, b2, y, u, R, C, D, d, stream);      // (no dropout: sed_mhsa.hip)
    return ffn_fwd_entry<true>(dtype, act, x, w1, b1, w2, b2, y, u, R, C, D, d, stream);
}

// u, da, a, du are [R][D]; D a multiple of 4
extern "C" int sed_ffn_act_bwd_drop(int act, const float* u, const float* da, float* a, float* du, size_t R, int D, float p,
                                    const uint32_t* rng, uint32_t stream_id, void* stream) {
    SED_REQUIRE(rng != nullptr, "the dropout state rng is required");
    DropArgs d;
    if (int rc = drop_require_args(p, rng, stream_id, &d)) return rc;
    SED_REQUIRE(R > 0 && D > 0 && D % 4 == 0, "R and D must be positive, D a multiple of 4");
    SED_REQUIRE(R < ((size_t)1 << 38) / (size_t)D, "R * D must stay below 2^38");
    if (d.thr == 0) return ffn_act_bwd_entry<false>(act, u, da, a, du, R * (size_t)D, D, d, stream);
    return ffn_act_bwd_entry<true>(act, u, da, a, du, R * (size_t)D, D, d, stream);
}
