// The Cin = 1 first layer (conv1 of block 0) for gfx950: direct forward, weight gradient, Gram statistics, the BatchNorm finalizers
// that work from them, and the "C1 mode" entry points of conv2, which rebuild conv1's output on load instead of reading it.
//
// Replaces conv1 / bn1 of the first ConvBlock, forward and autograd backward (models/spectogram_models.py:132-135,142,155 of the
// reference), and in C1 mode the conv2 calls of that block (:137-140,156).  The C1-mode kernels themselves are in sed_conv_pc.hip,
// sed_wgrad.hip, sed_dgrad_c1.hip and sed_bwd_fused_c1.hip; conv1's input gradient is in sed_c1_dx.hip.
#include "conv_common.h"

// =================================================================================================
// first layer (Cin = 1): direct, bandwidth bound
// =================================================================================================
// A workgroup walks bands of C1_TR rows grid-stride; per band the C1_TR + 2 input lines are staged in LDS
// (z-scored on the way in, zero padded) behind ONE barrier pair, then thread (w, cg) produces 8 output
// channels of pixel w in each row of the band.  All index math is 32-bit and per band.
constexpr int C1_TR = 8;

template <typename T>
__global__ __launch_bounds__(256) void conv_c1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                          const float* __restrict__ stdv, const float* __restrict__ w,
                                                          T* __restrict__ z, float* __restrict__ partial, int B,
                                                          int H, int W, int Cout, int Coutp, int G, int PPB) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* wsm = reinterpret_cast<float*>(smem);          // [9][Coutp]
    float* xrow = wsm + 9 * Coutp;                        // [C1_TR + 2][W+2]
    float* red = xrow + (C1_TR + 2) * (W + 2);            // [PPB][2][Coutp]
    const int tid = threadIdx.x;
    for (int i = tid; i < 9 * Coutp; i += blockDim.x) {
        const int tap = i / Coutp, c = i % Coutp;
        wsm[i] = c < Cout ? w[c * 9 + tap] : 0.f;
    }
    __syncthreads();
    const int cg = tid % G, pl = tid / G;                 // fixed channel group per thread
    float wr[9][8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) wr[t][e] = wsm[t * Coutp + cg * 8 + e];
    float S[8], Q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { S[e] = 0.f; Q[e] = 0.f; }
    const int WP2 = W + 2;
    const int bands = (H + C1_TR - 1) / C1_TR;
    for (int band = blockIdx.x; band < B * bands; band += gridDim.x) {
        const int b = band / bands, h0 = (band - b * bands) * C1_TR;
        __syncthreads();
        for (int i = tid; i < (C1_TR + 2) * WP2; i += blockDim.x) {
            const int rr = i / WP2, cc = i - rr * WP2;
            const int hy = h0 + rr - 1, wx = cc - 1;
            float v = 0.f;
            if (hy >= 0 && hy < H && wx >= 0 && wx < W) {
                v = x[((size_t)b * H + hy) * W + wx];
                if (mean) v = (v - mean[wx]) / stdv[wx];
            }
            xrow[i] = v;
        }
        __syncthreads();
        if (pl < PPB) {
            for (int wq = pl; wq < W; wq += PPB) {
                // sliding 3x3 window down the band: three new inputs per row
                float x0[3], x1[3], x2[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) { x0[j] = xrow[wq + j]; x1[j] = xrow[WP2 + wq + j]; }
#pragma unroll
                for (int r = 0; r < C1_TR; ++r) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) x2[j] = xrow[(r + 2) * WP2 + wq + j];
                    if (h0 + r < H) {
                        float a[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) a[e] = 0.f;
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) a[e] = fmaf(x0[j], wr[j][e], a[e]);
                        }
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) a[e] = fmaf(x1[j], wr[3 + j][e], a[e]);
                        }
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) a[e] = fmaf(x2[j], wr[6 + j][e], a[e]);
                        }
#pragma unroll
                        for (int e = 0; e < 8; ++e) { S[e] += a[e]; Q[e] = fmaf(a[e], a[e], Q[e]); }
                        store8<T>(z + (((size_t)b * H + h0 + r) * W + wq) * Coutp + cg * 8, a);
                    }
#pragma unroll
                    for (int j = 0; j < 3; ++j) { x0[j] = x1[j]; x1[j] = x2[j]; }
                }
            }
        }
    }
    if (partial) {
        __syncthreads();
        if (pl < PPB) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                red[(pl * 2 + 0) * Coutp + cg * 8 + e] = S[e];
                red[(pl * 2 + 1) * Coutp + cg * 8 + e] = Q[e];
            }
        }
        __syncthreads();
        for (int i = tid; i < 2 * Coutp; i += blockDim.x) {
            float t = 0.f;
            for (int q = 0; q < PPB; ++q) t += red[q * 2 * Coutp + i];
            partial[(size_t)blockIdx.x * 2 * Coutp + i] = t;
        }
    }
}

// With zsrc != NULL the layer's dz is produced on load: dz = ca*g + cb*z + cc (g = `dz` argument = output of
// the data-gradient epilogue, z = the layer's pre-BN output); nothing is written back -- block 0 has no
// data gradient, so its dz1 never needs to exist in memory.
// NPF: staged input values per thread, (C1_TR + 2) * (W + 2) <= NPF * 256 (4: W <= 100; 11: W <= SED_ANYW_MAX_W; c1_npf)
template <typename T, bool FUSED, int NPF>
__global__ __launch_bounds__(256) void conv_c1_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                            const float* __restrict__ stdv, const T* __restrict__ dz,
                                                            const T* __restrict__ zsrc, const float* __restrict__ ca,
                                                            const float* __restrict__ cb, const float* __restrict__ cc,
                                                            float* __restrict__ partial, int B, int H, int W,
                                                            int Coutp, int G, int PPB) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* xrow = reinterpret_cast<float*>(smem);         // [C1_TR + 2][W+2]
    float* red = xrow + (C1_TR + 2) * (W + 2);            // [PPB][Coutp] per tap
    const int tid = threadIdx.x;
    const int cg = tid % G, pl = tid / G;
    const int WP2 = W + 2;
    float acc[9][8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[t][e] = 0.f;
    float a8[8], b8[8], c8[8];
    if (FUSED) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { a8[e] = ca[cg * 8 + e]; b8[e] = cb[cg * 8 + e]; c8[e] = cc[cg * 8 + e]; }
    }
    const int bands = (H + C1_TR - 1) / C1_TR;
    // the band's input lines are fetched one band ahead into registers (the load -> LDS -> barrier -> compute chain of the
    // first version exposed a full memory latency per band: 31 bands x ~2.5 us per workgroup)
    const int nstage = (C1_TR + 2) * WP2;
    float pf[NPF];
    auto fetch = [&](int band) {
        const int b = band / bands, h0 = (band - b * bands) * C1_TR;
#pragma unroll
        for (int u = 0; u < NPF; ++u) {
            const int i = tid + u * 256;
            const int rr = i / WP2, cc2 = i - rr * WP2;
            const int hy = h0 + rr - 1, wx = cc2 - 1;
            float v = 0.f;
            if (i < nstage && band < B * bands && hy >= 0 && hy < H && wx >= 0 && wx < W) {
                v = x[((size_t)b * H + hy) * W + wx];
                if (mean) v = (v - mean[wx]) / stdv[wx];
            }
            pf[u] = v;
        }
    };
    // (host-checked: (C1_TR + 2) * (W + 2) <= NPF * 256)
    fetch(blockIdx.x);
    for (int band = blockIdx.x; band < B * bands; band += gridDim.x) {
        const int b = band / bands, h0 = (band - b * bands) * C1_TR;
        (void)b;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NPF; ++u)
            if (tid + u * 256 < nstage) xrow[tid + u * 256] = pf[u];
        __syncthreads();
        fetch(band + gridDim.x);
        if (pl < PPB) {
            for (int wq = pl; wq < W; wq += PPB) {
                float x0[3], x1[3], x2[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) { x0[j] = xrow[wq + j]; x1[j] = xrow[WP2 + wq + j]; }
                // the band's loads first (independent addresses), then the math
                float d[C1_TR][8], zz[FUSED ? C1_TR : 1][8];
#pragma unroll
                for (int r = 0; r < C1_TR; ++r) {
                    const int h = (h0 + r < H) ? h0 + r : H - 1;       // clamped: the row is skipped below
                    const size_t off = (((size_t)b * H + h) * W + wq) * Coutp + cg * 8;
                    load8<T>(dz + off, d[r]);
                    if (FUSED) load8<T>(zsrc + off, zz[FUSED ? r : 0]);
                }
#pragma unroll
                for (int r = 0; r < C1_TR; ++r) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) x2[j] = xrow[(r + 2) * WP2 + wq + j];
                    if (h0 + r < H) {
                        if (FUSED) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) d[r][e] = fmaf(a8[e], d[r][e], fmaf(b8[e], zz[FUSED ? r : 0][e], c8[e]));
                        }
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                acc[j][e] = fmaf(x0[j], d[r][e], acc[j][e]);
                                acc[3 + j][e] = fmaf(x1[j], d[r][e], acc[3 + j][e]);
                                acc[6 + j][e] = fmaf(x2[j], d[r][e], acc[6 + j][e]);
                            }
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 3; ++j) { x0[j] = x1[j]; x1[j] = x2[j]; }
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        __syncthreads();
        if (pl < PPB) {
#pragma unroll
            for (int e = 0; e < 8; ++e) red[pl * Coutp + cg * 8 + e] = acc[t][e];
        }
        __syncthreads();
        for (int i = tid; i < Coutp; i += blockDim.x) {
            float sacc = 0.f;
            for (int q = 0; q < PPB; ++q) sacc += red[q * Coutp + i];
            partial[((size_t)blockIdx.x * 9 + t) * Coutp + i] = sacc;
        }
    }
}

// -------------------------------------------------------------------------------------------------
// First-layer weight gradient without the layer's pre-BN output.  With dz1 = ca*g + cb*z1 + cc and
// z1[c] = sum_j w1[c][j]*xp[j] (xp = the 3x3 patch of the z-scored, zero-padded input),
//     dW1[c][k] = sum_px dz1[c]*xp[k] = ca[c]*A[c][k] + cb[c]*sum_j w1[c][j]*G[j][k] + cc[c]*sx[k]
// where A = sum_px g[c]*xp[k] is the plain first-layer weight gradient of g, and G[j][k] = sum_px xp[j]*xp[k],
// sx[k] = sum_px xp[k] depend on the input alone: z1 is never read (and is exact instead of bf16-rounded).
// conv_c1_gram_kernel: partial[block][54] = 45 products (j <= k, row-major upper triangle) then the 9 sums.
// -------------------------------------------------------------------------------------------------
template <int SIT>      // items per thread: (C1_TR + 2) * (W + 2) <= SIT * 256 (c1_npf)
__global__ __launch_bounds__(256) void conv_c1_gram_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                           const float* __restrict__ stdv, float* __restrict__ partial,
                                                           int B, int H, int W) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* xrow = reinterpret_cast<float*>(smem);         // [C1_TR + 2][W+2]
    float* red = xrow + (C1_TR + 2) * (W + 2);            // [4][54]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int WP2 = W + 2;
    float acc[54];
#pragma unroll
    for (int i = 0; i < 54; ++i) acc[i] = 0.f;
    const int bands = (H + C1_TR - 1) / C1_TR;
    // a thread's staging items are the same (row, column) of every band: index arithmetic and the z-score constants are hoisted out of
    // the band loop (they were more than half of the kernel's instructions); z-score as (v - mean) * (1 / std), the form of the
    // convolution kernels' input copy (conv_common.h / sed_conv_pc.hip)
    int srow[SIT], scol[SIT];
    float smu[SIT], sinv[SIT];
#pragma unroll
    for (int u = 0; u < SIT; ++u) {
        const int i = tid + u * 256;
        const int rr = i / WP2, cc2 = i - rr * WP2;
        const bool ok = i < (C1_TR + 2) * WP2 && cc2 >= 1 && cc2 <= W;
        srow[u] = i < (C1_TR + 2) * WP2 ? rr - 1 : (1 << 28);      // past the staged lines: never inside an image
        scol[u] = ok ? cc2 - 1 : -1;
        smu[u] = (ok && mean) ? mean[cc2 - 1] : 0.f;
        sinv[u] = (ok && mean) ? 1.0f / stdv[cc2 - 1] : 1.f;
    }
    const int npix = C1_TR * W;
    // the next band's lines are fetched into registers while this band's products run (the kernel was bound by one exposed memory
    // latency per band)
    float nraw[SIT];
    unsigned nvalid = 0;
    auto fetch = [&](int band) {
        nvalid = 0;
        if (band >= B * bands) return;
        const int b = band / bands, h0 = (band - b * bands) * C1_TR;
#pragma unroll
        for (int u = 0; u < SIT; ++u) {
            const int hy = h0 + srow[u];
            const bool ok = hy >= 0 && hy < H && scol[u] >= 0;
            nraw[u] = ok ? x[((size_t)b * H + hy) * W + scol[u]] : 0.f;
            nvalid |= ok ? (1u << u) : 0u;
        }
    };
    fetch(blockIdx.x);
    for (int band = blockIdx.x; band < B * bands; band += gridDim.x) {
        const int b = band / bands, h0 = (band - b * bands) * C1_TR;
        (void)b;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < SIT; ++u) {
            const int i = tid + u * 256;
            if (i >= (C1_TR + 2) * WP2) break;
            xrow[i] = ((nvalid >> u) & 1u) ? (nraw[u] - smu[u]) * sinv[u] : 0.f;
        }
        fetch(band + gridDim.x);
        __syncthreads();
        for (int pix = tid; pix < npix; pix += blockDim.x) {
            const int r = pix / W, wq = pix - r * W;
            if (h0 + r >= H) continue;
            float xp[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) xp[t] = xrow[(r + t / 3) * WP2 + wq + t % 3];
#pragma unroll
            for (int j = 0; j < 9; ++j)
#pragma unroll
                for (int k = j; k < 9; ++k) {
                    constexpr int dummy = 0; (void)dummy;
                    const int o = j * 9 - j * (j - 1) / 2 + (k - j);      // constant after unrolling (a running index went to scratch)
                    acc[o] = fmaf(xp[j], xp[k], acc[o]);
                }
#pragma unroll
            for (int k = 0; k < 9; ++k) acc[45 + k] += xp[k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 54; ++i) {
        const float t = wave_sum(acc[i]);
        if (lane == 0) red[wave * 54 + i] = t;
    }
    __syncthreads();
    if (tid < 54) partial[(size_t)blockIdx.x * 54 + tid] = red[tid] + red[54 + tid] + red[108 + tid] + red[162 + tid];
}

// BatchNorm statistics of z1 = conv1(x_norm) from the Gram statistics of the input patches:
//   sum z1[c] = sum_k w[c][k]*sx[k],  sum z1[c]^2 = sum_jk w[c][j]*w[c][k]*G[j][k]   (same outputs as bn_train_finalize)
__global__ __launch_bounds__(1024) void bn_train_finalize_c1_kernel(const float* __restrict__ gram, int nparts, double count,
                                                                    const float* __restrict__ w, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, float* __restrict__ rmean,
                                                                    float* __restrict__ rvar, float momentum, float eps,
                                                                    float* __restrict__ scale, float* __restrict__ shift,
                                                                    float* __restrict__ mean_o, float* __restrict__ invstd_o, int C,
                                                                    int Cp, double* __restrict__ gsum_out = nullptr) {
    __shared__ double G[54];
    __shared__ double Gp[16][64];
    const int tid = threadIdx.x;
    {
        const int v = tid & 63, g = tid >> 6;
        double s = 0.0;
        if (v < 54) {       // eight independent loads in flight, summed in the same fixed order as a plain loop
            int i = g;
            for (; i + 16 * 7 < nparts; i += 16 * 8) {
                float t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) t[u] = gram[(size_t)(i + 16 * u) * 54 + v];
#pragma unroll
                for (int u = 0; u < 8; ++u) s += (double)t[u];
            }
            for (; i < nparts; i += 16) s += (double)gram[(size_t)i * 54 + v];
        }
        Gp[g][v] = s;
    }
    __syncthreads();
    if (tid < 54) {
        double s = 0.0;
        for (int g = 0; g < 16; ++g) s += Gp[g][tid];
        G[tid] = s;
        if (gsum_out != nullptr) gsum_out[tid] = s;       // the reduced Gram statistics, kept for the backward's tail kernel (sed_c1_bwd_tail)
    }
    __syncthreads();
    for (int c = tid; c < Cp; c += blockDim.x) {
        if (c >= C) { scale[c] = 0.f; shift[c] = 0.f; mean_o[c] = 0.f; invstd_o[c] = 0.f; continue; }
        double s1 = 0.0, s2 = 0.0;
        for (int j = 0; j < 9; ++j) {
            s1 += (double)w[c * 9 + j] * G[45 + j];
            for (int k2 = 0; k2 < 9; ++k2) {
                const int a = j < k2 ? j : k2, b2 = j < k2 ? k2 : j;
                s2 += (double)w[c * 9 + j] * (double)w[c * 9 + k2] * G[a * 9 - a * (a - 1) / 2 + (b2 - a)];
            }
        }
        const double mean = s1 / count;
        double var = s2 / count - mean * mean;
        if (var < 0.0) var = 0.0;
        const float invstd = (float)(1.0 / sqrt(var + (double)eps));
        const float sc = gamma[c] * invstd;
        scale[c] = sc;
        shift[c] = beta[c] - (float)mean * sc;
        mean_o[c] = (float)mean;
        invstd_o[c] = invstd;
        if (rmean) {
            const double unbiased = count > 1.0 ? var * (count / (count - 1.0)) : var;
            rmean[c] = (1.f - momentum) * rmean[c] + momentum * (float)mean;
            rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)unbiased;
        }
    }
}

// BatchNorm-1 backward coefficients in C1 mode: sum g from the data-gradient epilogue, sum g*z1 = sum_k w1[c][k]*A[k][c]
// with A = the plain first-layer weight gradient of g (z1 itself is never read)
__global__ __launch_bounds__(256) void bn_bwd_finalize_c1_kernel(const float* __restrict__ partial, int nparts, double count,
                                                                 const float* __restrict__ A, const float* __restrict__ w,
                                                                 const float* __restrict__ gamma, const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta, float* __restrict__ ca,
                                                                 float* __restrict__ cb, float* __restrict__ cc, int C, int Cp) {
    __shared__ double sm[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < nparts; i += 256) s += (double)partial[((size_t)i * 2 + 0) * Cp + c];
    sm[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sm[tid] += sm[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        if (c >= C) { ca[c] = 0.f; cb[c] = 0.f; cc[c] = 0.f; return; }
        const double sg = sm[0];
        double sgz = 0.0;
        for (int k2 = 0; k2 < 9; ++k2) sgz += (double)w[c * 9 + k2] * (double)A[k2 * Cp + c];
        const double g = gamma[c], is = invstd[c], mu = mean[c];
        const double q = is * (sgz - mu * sg);              // sum g * xhat
        dbeta[c] = (float)sg;
        dgamma[c] = (float)q;
        const double mg = sg / count, mgx = q / count;
        ca[c] = (float)(g * is);
        cb[c] = (float)(-g * is * is * mgx);
        cc[c] = (float)(-g * is * (mg - mu * is * mgx));
    }
}

__global__ __launch_bounds__(1024) void conv_c1_wgrad_combine_kernel(const float* __restrict__ A, const float* __restrict__ gram,
                                                                    int nparts, const float* __restrict__ w,
                                                                    const float* __restrict__ ca, const float* __restrict__ cb,
                                                                    const float* __restrict__ cc, float* __restrict__ dw,
                                                                    int Cout, int Coutp, float* __restrict__ dw_torch = nullptr) {
    __shared__ double G[54];
    __shared__ double Gp[16][64];
    const int tid = threadIdx.x;
    {   // thread (value v, group g of 16): every 16th partial row, then a fixed-order 16-way sum
        const int v = tid & 63, g = tid >> 6;
        double s = 0.0;
        if (v < 54) {       // eight independent loads in flight, summed in the same fixed order as a plain loop
            int i = g;
            for (; i + 16 * 7 < nparts; i += 16 * 8) {
                float t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) t[u] = gram[(size_t)(i + 16 * u) * 54 + v];
#pragma unroll
                for (int u = 0; u < 8; ++u) s += (double)t[u];
            }
            for (; i < nparts; i += 16) s += (double)gram[(size_t)i * 54 + v];
        }
        Gp[g][v] = s;
    }
    __syncthreads();
    if (tid < 54) {
        double s = 0.0;
        for (int g = 0; g < 16; ++g) s += Gp[g][tid];
        G[tid] = s;
    }
    __syncthreads();
    for (int idx = tid; idx < 9 * Coutp; idx += blockDim.x) {
        const int k = idx / Coutp, c = idx - k * Coutp;
        float out = 0.f;
        if (c < Cout) {
            double wg = 0.0;
            for (int j = 0; j < 9; ++j) {
                const int a = j < k ? j : k, b2 = j < k ? k : j;          // symmetric: G[a][b2], a <= b2
                wg += (double)w[c * 9 + j] * G[a * 9 - a * (a - 1) / 2 + (b2 - a)];
            }
            out = (float)((double)ca[c] * (double)A[idx] + (double)cb[c] * wg + (double)cc[c] * G[45 + k]);
        }
        dw[idx] = out;
        if (dw_torch != nullptr && c < Cout) dw_torch[c * 9 + k] = out;      // torch layout [Cout][1][3][3]
    }
}

// Block 0's conv1 backward tail in ONE launch (round 5; C1 mode with the fused data gradient, no SyncBN): the three dependent
// one-workgroup-scale kernels sed_sum_partials ([A; sum g] partial rows) -> sed_bn_bwd_finalize_c1 -> sed_conv3x3_c1_wgrad_combine
// (which reduced the forward's Gram partial rows a second time: up to 2048 x 54 floats through one CU) took ~22 us of dependent
// launches per step.  Here: the [A; sum g] rows are summed (fixed order, double), BatchNorm-1's backward coefficients follow, and
// dW1 = ca*A + cb*(w1.G) + cc*sx takes the Gram statistics ALREADY REDUCED by the forward's sed_bn_train_finalize_c1_g (54 doubles).
// Same formulas, same rounding points as the three kernels (a10, ca / cb / cc are rounded to fp32 where they were stored).
__global__ __launch_bounds__(1024) void c1_bwd_tail_kernel(const float* __restrict__ a_part, int a_nparts, const double* __restrict__ gsum,
                                                           double count, const float* __restrict__ w, const float* __restrict__ gamma,
                                                           const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ ca,
                                                           float* __restrict__ cb, float* __restrict__ cc, float* __restrict__ a10_out,
                                                           float* __restrict__ dw, int Cout, float* __restrict__ dw_torch) {
    constexpr int Cp = 32, NV = 10 * Cp, NG = 3;
    __shared__ double As[NG][NV];
    __shared__ float a10[NV];
    __shared__ float coef[3][Cp];
    __shared__ double G[54];
    const int tid = threadIdx.x;
    if (tid < 54) G[tid] = gsum[tid];
    if (tid < NG * NV) {        // thread (value v, group g): rows g, g + 3, ..., eight loads in flight, one fixed order
        const int v = tid % NV, g = tid / NV;
        double s = 0.0;
        int i = g;
        for (; i + NG * 7 < a_nparts; i += NG * 8) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = a_part[(size_t)(i + NG * u) * NV + v];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += (double)t[u];
        }
        for (; i < a_nparts; i += NG) s += (double)a_part[(size_t)i * NV + v];
        As[g][v] = s;
    }
    __syncthreads();
    if (tid < NV) {
        const float t = (float)(As[0][tid] + As[1][tid] + As[2][tid]);
        a10[tid] = t;
        a10_out[tid] = t;
    }
    __syncthreads();
    if (tid < Cp) {             // BatchNorm-1 backward (bn_bwd_finalize_c1_kernel): sum g = row 9, sum g*z1 = w1 . A
        const int c = tid;
        float fa = 0.f, fb = 0.f, fc = 0.f;
        if (c < Cout) {
            const double sg = (double)a10[9 * Cp + c];
            double sgz = 0.0;
            for (int k2 = 0; k2 < 9; ++k2) sgz += (double)w[c * 9 + k2] * (double)a10[k2 * Cp + c];
            const double g = gamma[c], is = invstd[c], mu = mean[c];
            const double q = is * (sgz - mu * sg);
            dbeta[c] = (float)sg;
            dgamma[c] = (float)q;
            const double mg = sg / count, mgx = q / count;
            fa = (float)(g * is);
            fb = (float)(-g * is * is * mgx);
            fc = (float)(-g * is * (mg - mu * is * mgx));
        }
        ca[c] = fa; cb[c] = fb; cc[c] = fc;
        coef[0][c] = fa; coef[1][c] = fb; coef[2][c] = fc;
    }
    __syncthreads();
    for (int idx = tid; idx < 9 * Cp; idx += blockDim.x) {      // conv_c1_wgrad_combine_kernel
        const int k = idx / Cp, c = idx - k * Cp;
        float out = 0.f;
        if (c < Cout) {
            double wg = 0.0;
            for (int j = 0; j < 9; ++j) {
                const int a = j < k ? j : k, b2 = j < k ? k : j;
                wg += (double)w[c * 9 + j] * G[a * 9 - a * (a - 1) / 2 + (b2 - a)];
            }
            out = (float)((double)coef[0][c] * (double)a10[idx] + (double)coef[1][c] * wg + (double)coef[2][c] * G[45 + k]);
        }
        dw[idx] = out;
        if (dw_torch != nullptr && c < Cout) dw_torch[c * 9 + k] = out;
    }
}

// =================================================================================================
// host launchers (C ABI)
// =================================================================================================

extern "C" int sed_conv_c1_nparts(int B, int H, int W) {
    (void)W;
    // 768 = 3 resident 256-thread workgroups on each of the 256 CUs: one full round, no 1/3-occupancy tail
    const long long rows = (long long)B * H;
    return (int)(rows < 768 ? rows : 768);
}

static void c1_geometry(int Coutp, int* G, int* PPB, int* threads) {
    *G = Coutp / 8;
    *PPB = 256 / *G;
    if (*PPB < 1) *PPB = 1;
    *threads = 256;
}

extern "C" int sed_conv3x3_c1_fwd(int dtype, const float* x, const float* mean, const float* stdv, const float* w,
                                  void* z, float* stats_partial, int B, int H, int W, int Cout, int Coutp,
                                  void* stream) {
    SED_REQUIRE(Coutp % 32 == 0 && Coutp <= 2048 && Cout <= Coutp, "Coutp must be a multiple of 32, <= 2048");
    SED_REQUIRE((mean == nullptr) == (stdv == nullptr), "mean/std must both be given or both NULL");
    int G, PPB, threads;
    c1_geometry(Coutp, &G, &PPB, &threads);
    const int grid = sed_conv_c1_nparts(B, H, W);
    const size_t lds = ((size_t)9 * Coutp + (C1_TR + 2) * (size_t)(W + 2) + (size_t)PPB * 2 * Coutp) * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == SED_BF16)
        conv_c1_fwd_kernel<bf16_t><<<grid, threads, lds, st>>>(x, mean, stdv, w, (bf16_t*)z, stats_partial, B, H, W, Cout, Coutp, G, PPB);
    else if (dtype == SED_F32)
        conv_c1_fwd_kernel<float><<<grid, threads, lds, st>>>(x, mean, stdv, w, (float*)z, stats_partial, B, H, W, Cout, Coutp, G, PPB);
    else
        SED_REQUIRE(false, "bad dtype");
    SED_LAUNCH_CHECK();
    return 0;
}

static int c1_wgrad_common(int dtype, const float* x, const float* mean, const float* stdv, const void* dz,
                           const void* zsrc, const float* ca, const float* cb, const float* cc, float* dw_partial, int B,
                           int H, int W, int Coutp, void* stream);

// staged values per thread of the first-layer kernels that hold a band of C1_TR + 2 input lines: 4 up to W = 100 (the specialised
// widths), 11 up to SED_ANYW_MAX_W; 0 = W not covered
static int c1_npf(int W) {
    const int n = (C1_TR + 2) * (W + 2);
    return W < 1 ? 0 : n <= 4 * 256 ? 4 : n <= 11 * 256 ? 11 : 0;
}

extern "C" int sed_conv3x3_c1_wgrad(int dtype, const float* x, const float* mean, const float* stdv, const void* dz,
                                    float* dw_partial, int B, int H, int W, int Coutp, void* stream) {
    return c1_wgrad_common(dtype, x, mean, stdv, dz, nullptr, nullptr, nullptr, nullptr, dw_partial, B, H, W, Coutp, stream);
}

extern "C" int sed_conv3x3_c1_wgrad_fused(int dtype, const float* x, const float* mean, const float* stdv,
                                          const void* g, const void* zsrc, const float* ca, const float* cb,
                                          const float* cc, float* dw_partial, int B, int H, int W, int Coutp,
                                          void* stream) {
    SED_REQUIRE(g && zsrc && ca && cb && cc, "fused dz operands");
    return c1_wgrad_common(dtype, x, mean, stdv, g, zsrc, ca, cb, cc, dw_partial, B, H, W, Coutp, stream);
}

static int c1_wgrad_common(int dtype, const float* x, const float* mean, const float* stdv, const void* dz,
                           const void* zsrc, const float* ca, const float* cb, const float* cc, float* dw_partial, int B,
                           int H, int W, int Coutp, void* stream) {
    SED_REQUIRE(Coutp % 32 == 0 && Coutp <= 2048, "Coutp must be a multiple of 32, <= 2048");
    int G, PPB, threads;
    c1_geometry(Coutp, &G, &PPB, &threads);
    const int grid = sed_conv_c1_nparts(B, H, W);
    const size_t lds = ((C1_TR + 2) * (size_t)(W + 2) + (size_t)PPB * Coutp) * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    const int npf = c1_npf(W);
    SED_REQUIRE(npf > 0, "W must be in [1, SED_ANYW_MAX_W]");
#define SED_C1W(N_)                                                                                                                         \
    if (dtype == SED_BF16)                                                                                                                  \
        if (zsrc) conv_c1_wgrad_kernel<bf16_t, true, N_><<<grid, threads, lds, st>>>(x, mean, stdv, (const bf16_t*)dz, (const bf16_t*)zsrc, ca, cb, cc, dw_partial, B, H, W, Coutp, G, PPB); \
        else conv_c1_wgrad_kernel<bf16_t, false, N_><<<grid, threads, lds, st>>>(x, mean, stdv, (const bf16_t*)dz, nullptr, ca, cb, cc, dw_partial, B, H, W, Coutp, G, PPB); \
    else if (dtype == SED_F32)                                                                                                              \
        if (zsrc) conv_c1_wgrad_kernel<float, true, N_><<<grid, threads, lds, st>>>(x, mean, stdv, (const float*)dz, (const float*)zsrc, ca, cb, cc, dw_partial, B, H, W, Coutp, G, PPB); \
        else conv_c1_wgrad_kernel<float, false, N_><<<grid, threads, lds, st>>>(x, mean, stdv, (const float*)dz, nullptr, ca, cb, cc, dw_partial, B, H, W, Coutp, G, PPB); \
    else                                                                                                                                    \
        SED_REQUIRE(false, "bad dtype");
    if (npf == 4) { SED_C1W(4) } else { SED_C1W(11) }
#undef SED_C1W
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_conv_c1_gram_nparts(int B, int H, int W) {
    (void)W;
    // 2048 = 8 resident 256-thread workgroups per CU: the kernel has ~500 cycles of arithmetic per band behind a full
    // memory latency, only more resident workgroups hide it (768 workgroups: 83 us)
    const long long bands = (long long)B * ((H + C1_TR - 1) / C1_TR);
    return (int)(bands < 2048 ? (bands < 1 ? 1 : bands) : 2048);
}

extern "C" int sed_conv3x3_c1_gram(const float* x, const float* mean, const float* stdv, float* gram_partial, int B, int H,
                                   int W, void* stream) {
    SED_REQUIRE((mean == nullptr) == (stdv == nullptr), "mean/std must both be given or both NULL");
    const int npf = c1_npf(W);
    SED_REQUIRE(npf > 0, "W must be in [1, SED_ANYW_MAX_W] (one band of input lines is staged by 256 threads)");
    const int grid = sed_conv_c1_gram_nparts(B, H, W); // every row of gram_partial is written (the combine reads nparts rows)
    const size_t lds = ((C1_TR + 2) * (size_t)(W + 2) + 4 * 54) * sizeof(float);
    if (npf == 4) conv_c1_gram_kernel<4><<<grid, 256, lds, (hipStream_t)stream>>>(x, mean, stdv, gram_partial, B, H, W);
    else conv_c1_gram_kernel<11><<<grid, 256, lds, (hipStream_t)stream>>>(x, mean, stdv, gram_partial, B, H, W);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_conv3x3_c1_wgrad_combine(const float* a_sum, const float* gram_partial, int nparts, const float* w,
                                            const float* ca, const float* cb, const float* cc, float* dwpack, int Cout,
                                            int Coutp, void* stream) {
    SED_REQUIRE(a_sum && gram_partial && w && ca && cb && cc && dwpack && nparts > 0, "operands");
    conv_c1_wgrad_combine_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(a_sum, gram_partial, nparts, w, ca, cb, cc, dwpack, Cout, Coutp);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_conv3x3_c1_wgrad_combine_u(const float* a_sum, const float* gram_partial, int nparts, const float* w,
                                              const float* ca, const float* cb, const float* cc, float* dwpack, int Cout,
                                              int Coutp, float* dw, void* stream) {
    SED_REQUIRE(a_sum && gram_partial && w && ca && cb && cc && dwpack && dw && nparts > 0, "operands");
    conv_c1_wgrad_combine_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(a_sum, gram_partial, nparts, w, ca, cb, cc, dwpack, Cout, Coutp, dw);
    SED_LAUNCH_CHECK();
    return 0;
}

// ---- "C1 mode" entry points: the first ConvBlock without conv1's output in memory (bf16, W = 64, 32 channels) ----
extern "C" int sed_bn_train_finalize_c1(const float* gram_partial, int nparts, double count, const float* w1, const float* gamma,
                                        const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                                        float* scale, float* shift, float* mean, float* invstd, int C, int Cp, void* stream) {
    SED_REQUIRE(nparts > 0 && count > 0 && C <= Cp, "bad sizes");
    SED_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "running stats must both be given or both NULL");
    bn_train_finalize_c1_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(gram_partial, nparts, count, w1, gamma, beta, running_mean,
                                                                     running_var, momentum, eps, scale, shift, mean, invstd, C, Cp);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_bn_train_finalize_c1_g(const float* gram_partial, int nparts, double count, const float* w1, const float* gamma,
                                          const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                                          float* scale, float* shift, float* mean, float* invstd, int C, int Cp, double* gram_sum,
                                          void* stream) {
    SED_REQUIRE(nparts > 0 && count > 0 && C <= Cp && gram_sum, "bad sizes / operands");
    SED_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "running stats must both be given or both NULL");
    bn_train_finalize_c1_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(gram_partial, nparts, count, w1, gamma, beta, running_mean,
                                                                     running_var, momentum, eps, scale, shift, mean, invstd, C, Cp, gram_sum);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_c1_bwd_tail(const float* a_partial, int a_nparts, const double* gram_sum, double count, const float* w1,
                               const float* gamma, const float* mean, const float* invstd, float* dgamma, float* dbeta, float* ca,
                               float* cb, float* cc, float* a_sum, float* dwpack, int Cout, int Coutp, float* dw, void* stream) {
    SED_REQUIRE(a_partial && gram_sum && w1 && gamma && mean && invstd && dgamma && dbeta && ca && cb && cc && a_sum && dwpack &&
                a_nparts > 0 && count > 0, "operands");
    SED_REQUIRE(Coutp == 32 && Cout > 0 && Cout <= 32, "covered: 32 (padded) conv1 channels");
    c1_bwd_tail_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(a_partial, a_nparts, gram_sum, count, w1, gamma, mean, invstd, dgamma, dbeta,
                                                            ca, cb, cc, a_sum, dwpack, Cout, dw);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_c1_mode_supported(int dtype, int W, int C1, int Cout2) {
    return dtype == SED_BF16 && W == 64 && C1 == 32 && Cout2 == 32;
}

static int c1_conv_common(ConvParams& p, int W, void* stream) {
    p.dbg = sed_dbg_env();
    p.wres = 0;
    p.nparts = sed_conv_nparts(p.B, p.H, W);
    const int rc = launch_conv_pc(p, W, (hipStream_t)stream);
    if (rc < 0) { sed_set_error("C1 mode: shape not covered (needs bf16, W = 64, 32 conv1 channels)"); return 1; }
    if (rc) return rc;
    hipError_t e_ = hipGetLastError();
    if (e_ != hipSuccess) { sed_set_error(std::string("C1 mode launch failed: ") + hipGetErrorString(e_)); return 2; }
    return 0;
}

extern "C" int sed_conv3x3_fwd_c1(int dtype, int epi, const float* x1, const float* fmean, const float* fstd, const float* w1,
                                  const float* pro_scale, const float* pro_shift, const void* wpack, void* z, float* partial,
                                  void* relu_mask, int B, int H, int W, int Coutp, void* stream) {
    SED_REQUIRE(dtype == SED_BF16 && x1 && w1 && pro_scale && pro_shift && wpack && z, "operands");
    SED_REQUIRE((fmean == nullptr) == (fstd == nullptr), "mean/std must both be given or both NULL");
    SED_REQUIRE(epi == SED_EPI_STORE || (epi == SED_EPI_STATS && partial), "epilogue");
    ConvParams p = {};
    p.x = nullptr; p.pro_scale = pro_scale; p.pro_shift = pro_shift; p.wpack = wpack; p.z = z; p.partial = partial;
    p.B = B; p.H = H; p.Cinp = 32; p.Coutp = Coutp; p.pro = SED_PRO_C1; p.epi = epi;
    p.c1_x = x1; p.c1_mean = fmean; p.c1_std = fstd; p.c1_w = w1; p.c1_mask = relu_mask;
    return c1_conv_common(p, W, stream);
}

extern "C" int sed_conv3x3_dgrad_c1(int dtype, const void* dz, const void* wpack_t, void* g, const void* relu_mask, float* partial,
                                    int B, int H, int W, int Cinp, void* stream) {
    SED_REQUIRE(dtype == SED_BF16 && dz && wpack_t && g && relu_mask && partial, "operands");
    ConvParams p = {};
    p.x = dz; p.wpack = wpack_t; p.z = g; p.partial = partial;
    p.B = B; p.H = H; p.Cinp = Cinp; p.Coutp = 32; p.pro = SED_PRO_NONE; p.epi = SED_EPI_RELUBWD_C1;
    p.c1_mask = const_cast<void*>(relu_mask);
    return c1_conv_common(p, W, stream);
}

static int wgrad_fused_c1_impl(int dtype, const float* x1, const float* fmean, const float* fstd, const float* w1,
                               const float* pro_scale, const float* pro_shift, const void* gsrc, const void* zsrc,
                               const float* scale, const float* shift, const float* ca, const float* cb,
                               const float* cc, int pool, void* dz_out, float* dwpack, float* workspace, int B, int H,
                               int W, int Coutp, void* stream, float* dw, int Cout, int Cin) {
    SED_REQUIRE(dtype == SED_BF16 && x1 && w1 && pro_scale && pro_shift && gsrc && zsrc && scale && shift && ca && cb && cc &&
                dwpack, "operands");
    Wgrad2Params p = {};
    p.x = nullptr; p.pro_scale = pro_scale; p.pro_shift = pro_shift; p.dz = gsrc; p.zsrc = zsrc; p.scale = scale; p.shift = shift;
    p.ca = ca; p.cb = cb; p.cc = cc; p.dz_out = dz_out; p.ws = workspace;
    p.B = B; p.H = H; p.Cinp = 32; p.Coutp = Coutp; p.pro = SED_PRO_C1; p.pool = pool < 1 ? 1 : pool;
    p.c1_x = x1; p.c1_mean = fmean; p.c1_std = fstd; p.c1_w = w1;
    p.dbg = sed_dbg_env();
    const int rc = launch_wgrad3(DZ_POOL, p, W, (hipStream_t)stream);
    if (rc < 0) { sed_set_error("C1 mode weight gradient: shape not covered (needs W = 64, 32 -> 32 channels)"); return 1; }
    if (rc) return rc;
    hipError_t e_ = hipGetLastError();
    if (e_ != hipSuccess) { sed_set_error(std::string("C1 mode wgrad launch failed: ") + hipGetErrorString(e_)); return 2; }
    const size_t n = (size_t)9 * 32 * Coutp;
    reduce_wgrad_slabs(workspace, dwpack, p.strips, n, dw, Cout, Cin, 32, Coutp, (hipStream_t)stream);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_conv3x3_wgrad_fused_c1(int dtype, const float* x1, const float* fmean, const float* fstd, const float* w1,
                                          const float* pro_scale, const float* pro_shift, const void* gsrc, const void* zsrc,
                                          const float* scale, const float* shift, const float* ca, const float* cb,
                                          const float* cc, int pool, void* dz_out, float* dwpack, float* workspace, int B, int H,
                                          int W, int Coutp, void* stream) {
    return wgrad_fused_c1_impl(dtype, x1, fmean, fstd, w1, pro_scale, pro_shift, gsrc, zsrc, scale, shift, ca, cb, cc, pool, dz_out,
                               dwpack, workspace, B, H, W, Coutp, stream, nullptr, 0, 0);
}

extern "C" int sed_conv3x3_wgrad_fused_c1_u(int dtype, const float* x1, const float* fmean, const float* fstd, const float* w1,
                                            const float* pro_scale, const float* pro_shift, const void* gsrc, const void* zsrc,
                                            const float* scale, const float* shift, const float* ca, const float* cb,
                                            const float* cc, int pool, void* dz_out, float* dwpack, float* workspace, int B, int H,
                                            int W, int Coutp, float* dw, int Cout, int Cin, void* stream) {
    SED_REQUIRE(dw && Cout > 0 && Cin > 0 && Cout <= Coutp && Cin <= 32, "unpacked gradient operands");
    return wgrad_fused_c1_impl(dtype, x1, fmean, fstd, w1, pro_scale, pro_shift, gsrc, zsrc, scale, shift, ca, cb, cc, pool, dz_out,
                               dwpack, workspace, B, H, W, Coutp, stream, dw, Cout, Cin);
}

extern "C" int sed_conv3x3_bwd_fused_c1_supported(int dtype, int W, int Coutp, int pool) {
    if (!(dtype == SED_BF16 && W == 64 && Coutp == 32 && pool == 2)) return 0;
    if (const char* e = sed_getenv("SED_BWD_FUSED_C1")) if (e[0] == '0') return 0;
    return 1;
}

extern "C" int sed_conv3x3_bwd_fused_c1(int dtype, const float* x1, const float* fmean, const float* fstd, const float* w1,
                                        const float* pro_scale, const float* pro_shift, const void* gsrc, const void* zsrc,
                                        const float* scale, const float* shift, const float* ca, const float* cb, const float* cc,
                                        int pool, const void* wpack_t, const void* relu_mask, float* a_partial, float* dwpack,
                                        float* workspace, int B, int H, int W, int Coutp, float* dw, int Cout, int Cin, void* stream) {
    SED_REQUIRE(sed_conv3x3_bwd_fused_c1_supported(dtype, W, Coutp, pool), "covered: bf16, W = 64, 32 -> 32 channels, 2x2 pooling");
    SED_REQUIRE(x1 && w1 && pro_scale && pro_shift && gsrc && zsrc && scale && shift && ca && cb && cc && wpack_t &&
                a_partial && dwpack && workspace && B > 0 && H > 0, "operands");
    SED_REQUIRE(relu_mask == nullptr, "the ReLU gate is derived from the rebuilt activation tile: relu_mask must be NULL");
    SED_REQUIRE((fmean == nullptr) == (fstd == nullptr), "mean/std must both be given or both NULL");
    SED_REQUIRE(dw == nullptr || (Cout > 0 && Cin > 0 && Cout <= 32 && Cin <= 32), "unpacked gradient operands");
    SED_REQUIRE((double)H * W * 32 * 2 < 2147483648.0, "one image must stay below 2 GiB");
    int nwg = 0;
    const int rc = launch_bwd_fused_c1(x1, fmean, fstd, w1, pro_scale, pro_shift, gsrc, zsrc, scale, shift, ca, cb, cc, wpack_t,
                                       a_partial, sed_conv_dgrad_c1_nparts(), workspace, B, H, &nwg, (hipStream_t)stream);
    SED_REQUIRE(rc >= 0, "not covered");
    if (rc) return rc;
    SED_LAUNCH_CHECK();
    const size_t n = (size_t)9 * 32 * 32;
    reduce_wgrad_slabs(workspace, dwpack, nwg, n, dw, Cout, Cin, 32, 32, (hipStream_t)stream);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_bn_bwd_finalize_c1(const float* partial, int nparts, double count, const float* a_sum, const float* w1,
                                      const float* gamma, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                                      float* ca, float* cb, float* cc, int C, int Cp, void* stream) {
    SED_REQUIRE(nparts > 0 && count > 0 && C <= Cp && a_sum && w1, "bad sizes");
    bn_bwd_finalize_c1_kernel<<<Cp, 256, 0, (hipStream_t)stream>>>(partial, nparts, count, a_sum, w1, gamma, mean, invstd, dgamma,
                                                                   dbeta, ca, cb, cc, C, Cp);
    SED_LAUNCH_CHECK();
    return 0;
}
