// Input gradient of the Cin = 1 first layer, and the C1 form of the eval-mode (running-statistics) BatchNorm backward.
//
// Reference: autograd through the first ConvBlock, models/spectogram_models.py:153-160 of the reference:
//   dz1 = ca*g1 + cb*z1 + cc                     (BN1 backward; g1 = gradient at BN1's output)
//   dx[b][h][w] = sum_{c, tap} w1[c][tap] * dz1[b][h - dh][w - dw][c]      (conv1's data gradient onto its one channel)
// One 256-thread workgroup per 8 x 64 output tile.  Phase 1 reads the tile's (8+2) x (64+2) halo of g1 / z1 once and reduces every
// source pixel's channels to its nine per-tap partials s[tap] = sum_c w1[c][tap] * dz1[c] (fp32 FMA, LDS).  Phase 2 is the 3x3
// shift-add of those partials.  z1 is read, or recomputed from the z-scored input (C1 mode keeps no z1 in memory).  Outside the image
// dz1 = 0: cc never leaks into the zero padding.
#include "common.h"

namespace {

constexpr int DX_TH = 8, DX_TW = 64, DX_NT = 256;
constexpr int DX_SR = DX_TH + 2, DX_SC = DX_TW + 2, DX_SN = DX_SR * DX_SC;     // dz1 halo tile
constexpr int DX_XR = DX_TH + 4, DX_XC = DX_TW + 4, DX_XN = DX_XR * DX_XC;     // input tile of the z1 recompute

template <typename T, bool RECOMP>
__global__ __launch_bounds__(DX_NT) void c1_dgrad_kernel(const T* __restrict__ g, const T* __restrict__ z, const float* __restrict__ x,
                                                         const float* __restrict__ fmean, const float* __restrict__ fstd,
                                                         const float* __restrict__ w1, const float* __restrict__ ca,
                                                         const float* __restrict__ cb, const float* __restrict__ cc,
                                                         float* __restrict__ dx, int H, int W, int Cout, int Coutp, int tilesW) {
    __shared__ float sp[9][DX_SN];
    __shared__ float sx[RECOMP ? DX_XN : 1];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int th = blockIdx.x / tilesW, tw = blockIdx.x - th * tilesW;
    const int h0 = th * DX_TH, w0 = tw * DX_TW;
    if constexpr (RECOMP) {
        // z-scored input, zero outside the image (the reference pads the normalised features)
        for (int i = tid; i < DX_XN; i += DX_NT) {
            const int r = i / DX_XC, c = i - r * DX_XC;
            const int h = h0 - 2 + r, w = w0 - 2 + c;
            float v = 0.f;
            if (h >= 0 && h < H && w >= 0 && w < W) {
                v = x[((size_t)b * H + h) * W + w];
                if (fmean) v = (v - fmean[w]) / fstd[w];
            }
            sx[i] = v;
        }
        __syncthreads();
    }
    for (int i = tid; i < DX_SN; i += DX_NT) {
        const int r = i / DX_SC, c = i - r * DX_SC;
        const int h = h0 - 1 + r, w = w0 - 1 + c;
        float acc[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[t] = 0.f;
        if (h >= 0 && h < H && w >= 0 && w < W) {
            const size_t px = (((size_t)b * H + h) * W + w) * Coutp;
            float xv[9];
            if constexpr (RECOMP) {
#pragma unroll
                for (int t = 0; t < 9; ++t) xv[t] = sx[(r + t / 3) * DX_XC + c + t % 3];
            }
            for (int c0 = 0; c0 < Cout; c0 += 8) {
                float gv[8], zv[8];
                load8<T>(g + px + c0, gv);
                if constexpr (!RECOMP) load8<T>(z + px + c0, zv);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int ch = c0 + e;
                    if (ch < Cout) {
                        const float* wc = w1 + ch * 9;
                        float zc;
                        if constexpr (RECOMP) {
                            zc = 0.f;
#pragma unroll
                            for (int t = 0; t < 9; ++t) zc = fmaf(wc[t], xv[t], zc);
                        } else {
                            zc = zv[e];
                        }
                        const float d = ca[ch] * gv[e] + cb[ch] * zc + cc[ch];
#pragma unroll
                        for (int t = 0; t < 9; ++t) acc[t] = fmaf(wc[t], d, acc[t]);
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) sp[t][i] = acc[t];
    }
    __syncthreads();
    for (int i = tid; i < DX_TH * DX_TW; i += DX_NT) {
        const int r = i / DX_TW, c = i - r * DX_TW;
        const int h = h0 + r, w = w0 + c;
        if (h >= H || w >= W) continue;
        // tap (kh, kw) of output pixel (h, w) reads the partial of source pixel (h - kh + 1, w - kw + 1)
        float v = 0.f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) v += sp[kh * 3 + kw][(r - kh + 2) * DX_SC + (c - kw + 2)];
        if (fstd) v = v / fstd[w];
        dx[((size_t)b * H + h) * W + w] = v;
    }
}

}  // namespace

extern "C" int sed_conv3x3_c1_dgrad(int dtype, const void* g, const void* z, const float* x, const float* fmean, const float* fstd,
                                    const float* w1, const float* ca, const float* cb, const float* cc, float* dx, int B, int H, int W,
                                    int Cout, int Coutp, void* stream) {
    SED_REQUIRE(dtype == SED_BF16 || dtype == SED_F32, "dtype must be SED_BF16 or SED_F32");
    SED_REQUIRE(g && w1 && ca && cb && cc && dx && (z || x), "operands");
    SED_REQUIRE((fmean == nullptr) == (fstd == nullptr), "mean/std must both be given or both NULL");
    SED_REQUIRE(B > 0 && H > 0 && W > 0 && W <= SED_ANYW_MAX_W && B <= 65535, "shape");
    SED_REQUIRE(Cout > 0 && Cout <= Coutp && Coutp % 32 == 0, "channels");
    const int tilesW = cdiv(W, DX_TW);
    const long long tiles = (long long)cdiv(H, DX_TH) * tilesW;
    SED_REQUIRE(tiles < (1LL << 31), "shape");
    const dim3 grid((unsigned)tiles, B);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == SED_BF16) {
        const bf16_t* gp = reinterpret_cast<const bf16_t*>(g);
        const bf16_t* zp = reinterpret_cast<const bf16_t*>(z);
        if (z) c1_dgrad_kernel<bf16_t, false><<<grid, DX_NT, 0, st>>>(gp, zp, x, fmean, fstd, w1, ca, cb, cc, dx, H, W, Cout, Coutp, tilesW);
        else   c1_dgrad_kernel<bf16_t, true><<<grid, DX_NT, 0, st>>>(gp, zp, x, fmean, fstd, w1, ca, cb, cc, dx, H, W, Cout, Coutp, tilesW);
    } else {
        const float* gp = reinterpret_cast<const float*>(g);
        const float* zp = reinterpret_cast<const float*>(z);
        if (z) c1_dgrad_kernel<float, false><<<grid, DX_NT, 0, st>>>(gp, zp, x, fmean, fstd, w1, ca, cb, cc, dx, H, W, Cout, Coutp, tilesW);
        else   c1_dgrad_kernel<float, true><<<grid, DX_NT, 0, st>>>(gp, zp, x, fmean, fstd, w1, ca, cb, cc, dx, H, W, Cout, Coutp, tilesW);
    }
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_bn_eval_bwd_finalize_c1(const float* partial, int nparts, const float* a_sum, const float* w1, const float* gamma,
                                           const float* mean, const float* invstd, float* dgamma, float* dbeta, float* ca, float* cb,
                                           float* cc, int C, int Cp, void* stream) {
    SED_REQUIRE(partial && nparts > 0 && a_sum && w1 && C > 0 && C <= Cp, "operands");
    launch_bn_eval_bwd_finalize(partial, nparts, a_sum, w1, gamma, mean, invstd, dgamma, dbeta, ca, cb, cc, C, Cp, (hipStream_t)stream);
    SED_LAUNCH_CHECK();
    return 0;
}
