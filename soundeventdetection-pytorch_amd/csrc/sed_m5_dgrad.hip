// M5's first layer, data gradient: the transposed convolution of Conv1d(1, 64, kernel 79, stride 4, padding 39) of
// /root/reference/models/waveform_models.py:15-24 (conv_block1.0), i.e. what autograd puts into x.grad of the raw waveform:
//   dx[b][l] = sum_c sum_t dz[b][t][c] * w[c][l + 39 - 4t]          (0 <= l + 39 - 4t < 79, 0 <= t < L1)
// It is the forward's GEMM transposed, on the matrix pipe,
//   D[tap][t] = sum_c w[c][tap] * dz[t][c]                          A = w^T (80 x 64, taps padded to 96), B = dz^T (64 x positions)
// followed by an overlap-add dx[4t + tap - 39] += D[tap][t].  The overlap-add is a GATHER in a fixed order (no float atomics, the
// same bits on every run): D goes to LDS as [tap][position]; with tap = 4q + p the sample o = 4m + p of the tile's window is
// sum_{q = 0..19} D[4q + p][m - q], twenty reads of consecutive addresses across the lanes.
// Tile seams: a tile OWNS 4*TO = 416 consecutive samples of one frame and contracts the PT = TO + 2*HALO = 128 positions that can
// reach them (a sample takes positions (l - 39)/4 .. (l + 39)/4: 10 on each side of the owned range; HALO = 12 keeps the tile on a
// MaxPool window boundary).  The halo positions are recomputed by the neighbouring tile (23 % more MFMAs and, mostly from L2, loads)
// instead of a second launch that sums seam partials.  Every sample 0 <= l < L belongs to exactly one tile and is stored by it.
//   bf16: v_mfma_f32_32x32x16_bf16, dz either read (materialised form) or rebuilt on load from the pooled gradient dy, the stored z
//         and the BatchNorm coefficients exactly as m5_conv1_wgrad_mfma_kernel<POOLG> does (dz is never written);
//   fp32: v_mfma_f32_32x32x2_f32 (exact fp32 products and accumulation) on the materialised dz of sed_bn_bwd_apply.
#include "conv_common.h"

namespace {

constexpr int K1 = 79, K1P = 80, S1 = 4, P1 = 39, C1 = 64;
constexpr int PT = 128;                       // positions contracted per tile
constexpr int HALO = 12;                      // recomputed positions on each side (>= 10; a multiple of 4: pooling windows)
constexpr int TO = PT - 2 * HALO;             // positions whose 4 samples the tile owns
constexpr int OUT = S1 * TO;                  // owned samples: l = 4*TO*j + e, e in [0, OUT)
constexpr int O0 = S1 * HALO + P1;            // window index o = l + 39 - 4*tp0 of the first owned sample (tp0 = TO*j - HALO)
constexpr int NQ = K1P / S1;                  // taps per stride phase
// phase p of the owned window: o = 4m + p with m in [m0(p), m0(p) + TO); its gather reads positions m - 19 .. m of the tile
constexpr int m0_of(int p) { return (O0 - p + S1 - 1) / S1; }
static_assert(HALO % 4 == 0 && 4 * HALO >= P1, "halo");
static_assert(m0_of(3) - (NQ - 1) >= 0 && m0_of(0) + TO - 1 < PT, "every gathered position lies inside the tile");

template <typename T> struct R8;              // 8 consecutive stored elements, raw
template <> struct R8<bf16_t> {
    bf16x8 v;
    __device__ __forceinline__ void load(const bf16_t* p) { v = *reinterpret_cast<const bf16x8*>(p); }
    __device__ __forceinline__ float get(int i) const { return (float)v[i]; }
};
template <> struct R8<float> {
    f32x4 a, b;
    __device__ __forceinline__ void load(const float* p) {
        a = *reinterpret_cast<const f32x4*>(p);
        b = *reinterpret_cast<const f32x4*>(p + 4);
    }
    __device__ __forceinline__ float get(int i) const { return i < 4 ? a[i] : b[i - 4]; }
};

// POOLG (bf16): g = the pooled dy [B/8][L1/4][8][64]; dz = ca*G + cb*z + cc with G = dy at the first arg-max of relu(scale*z + shift)
// over each window of 4 when that maximum is > 0 (sed_maxpool4_relu_bwd), rebuilt on load.  !POOLG: g = dz itself [B/8][L1][8][64].
template <typename T, bool POOLG>
__global__ __launch_bounds__(256) void m5_conv1_dgrad_kernel(const T* __restrict__ g, const T* __restrict__ zsrc,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             const float* __restrict__ ca, const float* __restrict__ cb,
                                                             const float* __restrict__ cc, const float* __restrict__ w,
                                                             float* __restrict__ dx, int B, int L, int L1, int tiles) {
    constexpr bool BF = sizeof(T) == 2;
    static_assert(BF || !POOLG, "the rebuilt-on-load form is the bf16 one");
    // staging row pitch: 64 channels + 16 B.  The B fragment is one ds_read_b128 per lane with lane = row: the 16 rows of a lane
    // group then start on 16 different multiples of 4 banks (bf16: 36 words per row, fp32: 68)
    constexpr int PITCH = C1 + 16 / (int)sizeof(T);
    constexpr int NK = C1 / EL<T>::KSTEP;                             // MFMA k-steps over the 64 channels (bf16 4, fp32 32)
    __shared__ __attribute__((aligned(16))) float buf[K1P * PT];      // the dz tile [position][PITCH] of T, then D [tap][position]
    __shared__ float ov[OUT];                                         // the owned samples, for whole-line stores
    static_assert(PT * PITCH * sizeof(T) <= sizeof(float) * K1P * PT, "the dz tile fits under the D image");
    T* stg = reinterpret_cast<T*>(buf);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, hh = lane >> 5;
    // A fragments for the whole kernel: row = tap 32*tt + r (taps >= 79: zero rows); the lane's channels of k-step ks are
    // 16*ks + 8*hh + j (bf16) or the single channel 32*hh + ks (fp32: the two k of an instruction are channels ks and 32 + ks, so that
    // the B side is 32 consecutive floats per lane)
    typename EL<T>::frag_t wa[3][NK];
#pragma unroll
    for (int tt = 0; tt < 3; ++tt) {
        const int tap = 32 * tt + r;
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) {
            if constexpr (BF) {
#pragma unroll
                for (int j = 0; j < 8; ++j) wa[tt][ks][j] = (bf16_t)(tap < K1 ? w[(16 * ks + 8 * hh + j) * K1 + tap] : 0.f);
            } else {
                wa[tt][ks] = tap < K1 ? w[(32 * hh + ks) * K1 + tap] : 0.f;
            }
        }
    }
    const int c8 = tid & 7;                   // dz production: this thread's 8 channels
    float a8[8], b8[8], k8[8], sc8[8], sh8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        a8[e] = POOLG ? ca[c8 * 8 + e] : 0.f; b8[e] = POOLG ? cb[c8 * 8 + e] : 0.f; k8[e] = POOLG ? cc[c8 * 8 + e] : 0.f;
        sc8[e] = POOLG ? scale[c8 * 8 + e] : 0.f; sh8[e] = POOLG ? shift[c8 * 8 + e] : 0.f;
    }
    const int Ho = L1 >> 2;                   // pooled length (floor)
    // operands of the NEXT tile are fetched into registers while this tile computes
    constexpr int NIT = PT * 8 / 256;
    static_assert(NIT == 4, "a thread owns one pooling window of 4 steps");
    R8<T> gn[POOLG ? 1 : NIT], zn[POOLG ? NIT : 1];
    auto fetch = [&](int tile) {
        const bool live = tile < B * tiles;
        const int b = live ? tile / tiles : 0, tp0 = live ? (tile - b * tiles) * TO - HALO : 0;
#pragma unroll
        for (int u = 0; u < NIT; ++u) {
            const int row = POOLG ? 4 * (tid >> 3) + u : (tid >> 3) + 32 * u, t = tp0 + row;
            const bool ok = live && t >= 0 && t < L1;
            const size_t o = ok ? (((size_t)(b >> 3) * L1 + t) * 8 + (b & 7)) * C1 + c8 * 8 : 0;     // (dead rows re-read element 0 and are zeroed below)
            if constexpr (POOLG) zn[u].load(zsrc + o);
            else gn[u].load(g + o);
        }
        if constexpr (POOLG) {
            const int ho = (tp0 >> 2) + (tid >> 3);          // (tp0 is a multiple of 4, also when negative)
            const bool ok = live && ho >= 0 && ho < Ho;
            const size_t o = ok ? (((size_t)(b >> 3) * Ho + ho) * 8 + (b & 7)) * C1 + c8 * 8 : 0;
            gn[0].load(g + o);
        }
    };
    fetch(blockIdx.x);
    for (int tile = blockIdx.x; tile < B * tiles; tile += gridDim.x) {
        const int b = tile / tiles, jt = tile - b * tiles, tp0 = jt * TO - HALO;
        __syncthreads();                      // the previous tile's gather has read D (which the dz tile overlays)
        if constexpr (POOLG) {
            const int ho = (tp0 >> 2) + (tid >> 3);
            const bool win_ok = ho >= 0 && ho < Ho;
            float best[8];
            int am[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { best[e] = fmaxf(0.f, fmaf(zn[0].get(e), sc8[e], sh8[e])); am[e] = 0; }
#pragma unroll
            for (int i = 1; i < 4; ++i)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float a = fmaxf(0.f, fmaf(zn[i].get(e), sc8[e], sh8[e]));
                    if (a > best[e]) { best[e] = a; am[e] = i; }      // strict: ties keep the first (torch max_pool1d)
                }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 4 * (tid >> 3) + i, t = tp0 + row;
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float gg = (win_ok && am[e] == i && best[e] > 0.f) ? gn[0].get(e) : 0.f;
                    v[e] = (t >= 0 && t < L1) ? fmaf(a8[e], gg, fmaf(b8[e], zn[i].get(e), k8[e])) : 0.f;
                }
                store8<T>(stg + row * PITCH + c8 * 8, v);
            }
        } else {
#pragma unroll
            for (int u = 0; u < NIT; ++u) {
                const int row = (tid >> 3) + 32 * u, t = tp0 + row;
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = (t >= 0 && t < L1) ? gn[u].get(e) : 0.f;
                store8<T>(stg + row * PITCH + c8 * 8, v);
            }
        }
        __syncthreads();
        fetch(tile + gridDim.x);
        // wave wv: positions 32*wv .. + 31 (lane = position), all 96 tap rows
        f32x16 acc[3];
#pragma unroll
        for (int tt = 0; tt < 3; ++tt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[tt][i] = 0.f;
        const T* prow = stg + (32 * wv + r) * PITCH;
        if constexpr (BF) {
#pragma unroll
            for (int ks = 0; ks < NK; ++ks) {
                const bf16x8 bf = *reinterpret_cast<const bf16x8*>(prow + 16 * ks + 8 * hh);
#pragma unroll
                for (int tt = 0; tt < 3; ++tt) acc[tt] = mfma(wa[tt][ks], bf, acc[tt]);       // D[tap][position]
            }
        } else {
#pragma unroll
            for (int k4 = 0; k4 < NK / 4; ++k4) {
                const f32x4 bv = *reinterpret_cast<const f32x4*>(prow + 32 * hh + 4 * k4);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int tt = 0; tt < 3; ++tt) acc[tt] = mfma(wa[tt][4 * k4 + j], bv[j], acc[tt]);
            }
        }
        __syncthreads();                      // every wave has read its rows of the dz tile: D may overwrite it
        // register i of tile tt = tap 32*tt + (i&3) + 8*(i>>2) + 4*hh, lane = position: 32 consecutive words per store group
#pragma unroll
        for (int tt = 0; tt < 3; ++tt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int tap0 = 32 * tt + (i & 3) + 8 * (i >> 2);         // (+ 4*hh <= tap0 + 4)
                if (tap0 + 4 < K1P) buf[(tap0 + 4 * hh) * PT + 32 * wv + r] = acc[tt][i];
            }
        __syncthreads();
        // gather: sample o = 4m + p of the window <- sum over q of D[4q + p][m - q], q ascending (tap 79 is a zero row)
#pragma unroll
        for (int u = 0; u < (OUT + 255) / 256; ++u) {
            const int idx = tid + 256 * u;
            if (idx < OUT) {
                const int p = idx / TO, m = idx - p * TO + (O0 - p + S1 - 1) / S1;
                const float* dp = buf + p * PT + m;
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < NQ; ++q) s += dp[q * (S1 * PT - 1)];
                ov[S1 * m + p - O0] = s;
            }
        }
        __syncthreads();
        float* __restrict__ dxb = dx + (size_t)b * L;
        const int l0 = jt * OUT;
#pragma unroll
        for (int u = 0; u < (OUT + 255) / 256; ++u) {
            const int e = tid + 256 * u;
            if (e < OUT && l0 + e < L) dxb[l0 + e] = ov[e];
        }
    }
}

}  // namespace

extern "C" int sed_m5_conv1_len(int L);

static int m5_dgrad_grid(int B, int tiles) {
    const long long n = (long long)B * tiles;
    return (int)(n < 768 ? n : 768);          // 3 resident 256-thread workgroups per CU (LDS: 42.6 KB each)
}

extern "C" int sed_m5_conv1_dgrad(int dtype, const void* dz, const float* w, float* dx, int B, int L, void* stream) {
    SED_REQUIRE(dtype == SED_BF16 || dtype == SED_F32, "covered: bf16, fp32");
    SED_REQUIRE(B > 0 && B % 8 == 0, "the interleaved layout needs a batch that is a multiple of 8");
    SED_REQUIRE(L >= K1 - 2 * P1, "frame too short");
    SED_REQUIRE(dz && w && dx, "operands");
    const int L1 = sed_m5_conv1_len(L), tiles = cdiv(L, OUT);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == SED_BF16)
        m5_conv1_dgrad_kernel<bf16_t, false><<<m5_dgrad_grid(B, tiles), 256, 0, st>>>((const bf16_t*)dz, nullptr, nullptr, nullptr, nullptr,
                                                                                     nullptr, nullptr, w, dx, B, L, L1, tiles);
    else
        m5_conv1_dgrad_kernel<float, false><<<m5_dgrad_grid(B, tiles), 256, 0, st>>>((const float*)dz, nullptr, nullptr, nullptr, nullptr,
                                                                                    nullptr, nullptr, w, dx, B, L, L1, tiles);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_m5_conv1_dgrad_fused_pool(int dtype, const void* dy, const void* zsrc, const float* scale, const float* shift,
                                             const float* ca, const float* cb, const float* cc, const float* w, float* dx, int B,
                                             int L, void* stream) {
    SED_REQUIRE(dtype == SED_BF16, "covered: bf16 (fp32 takes the materialised dz: sed_m5_conv1_dgrad)");
    SED_REQUIRE(B > 0 && B % 8 == 0, "the interleaved layout needs a batch that is a multiple of 8");
    SED_REQUIRE(L >= K1 - 2 * P1, "frame too short");
    SED_REQUIRE(dy && zsrc && scale && shift && ca && cb && cc && w && dx, "operands");
    const int L1 = sed_m5_conv1_len(L), tiles = cdiv(L, OUT);
    SED_REQUIRE(L1 >= 4, "frame too short for MaxPool1d(4)");
    m5_conv1_dgrad_kernel<bf16_t, true><<<m5_dgrad_grid(B, tiles), 256, 0, (hipStream_t)stream>>>(
        (const bf16_t*)dy, (const bf16_t*)zsrc, scale, shift, ca, cb, cc, w, dx, B, L, L1, tiles);
    SED_LAUNCH_CHECK();
    return 0;
}
