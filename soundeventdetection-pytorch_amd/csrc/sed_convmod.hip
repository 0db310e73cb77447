// Self-attention temporal head: the Conformer convolution module between the attention and the feed-forward sub-layer of an encoder
// layer -- pointwise conv -> GLU -> depthwise conv along time -> BatchNorm -> SiLU -> pointwise conv.  The two pointwise convolutions
// are sed_gemm_nt launches and the BatchNorm finalisation is sed_bn_train_finalize / sed_bn_eval_coeffs / sed_bn_bwd_finalize /
// sed_bn_eval_stats / sed_bn_eval_bwd_finalize (sed_ops.hip, with Cp = C); this file holds what lies between them.
//
// With R = B*t rows, C channels, an odd tap count k in [3, 31] and p = (k - 1) / 2:
//   v[r][c]   = g[r][c] * sigmoid(g[r][C + c])                                   g [R][2C]  (F.glu over the channels)
//   z[b,i,c]  = bias[c] + sum_{j<k} w[c][j] * v[b, i + j - p, c]                  w [C][k]   (Conv1d(C, C, k, padding=p, groups=C);
//                                                                                            frames outside [0, t) of the SAME clip are 0)
//   partial   = per-workgroup (sum z, sum z^2) per channel                        [nparts][2][C] (what sed_bn_train_finalize reads)
//   s         = y * sigmoid(y),  y = scale * z + shift                            (sed_bn_silu_fwd)
// backward:
//   gz        = ds * sigmoid(y) * (1 + y * (1 - sigmoid(y)))                      (sed_bn_silu_bwd_reduce)
//   partial   = per-workgroup (sum gz, sum gz * xhat),  xhat = (z - mean) * invstd   [nparts][2][C] (what sed_bn_bwd_finalize reads)
//   dz        = ca * gz + cb * z + cc                                             (formed on load, sed_dwconv_glu_bwd)
//   dv[b,i,c] = sum_{j<k} w[c][j] * dz[b, i - j + p, c]                           (the transposed convolution, zero outside the clip)
//   dg[r][c]  = dv * sigma,   dg[r][C + c] = dv * g[r][c] * sigma * (1 - sigma),  sigma = sigmoid(g[r][C + c])
//   dw[c][j]  = sum_{b,i} dz[b,i,c] * v[b, i + j - p, c],   dbias[c] = sum_{b,i} dz[b,i,c]
// (tests/convmod_formula.py is the same in float64 numpy.)
//
// Everything here is fp32 vector arithmetic in every precision mode: k multiply-adds per element are a bandwidth problem, not a matrix
// one.  sigmoid(x) = 1 / (1 + expf(-x)) with the IEEE division (exactly 1 for x >= 17, 0 for x <= -104).
//
// sed_dwconv_glu_fwd / _bwd: a workgroup of 256 threads owns DW_TILE = 64 frames of one clip across DW_CH = 32 channels.  It stages
// the tile plus its p-frame halo in LDS -- the forward v with the GLU applied on load, so that a sigmoid is computed once and not k
// times, the backward dz and v -- and every thread forms two frames of four channels from LDS.  Global accesses are 16 bytes along the
// channel axis.  A training forward STORES v (tile rows only, each element once): the weight gradient reads it back with its halo, which
// costs one read of [R][C] in the backward instead of a second read of g's halo rows and k-fold recomputed sigmoids.
// The weight-gradient partials: thread (channel quad, slice, j) owns tap j of four channels over a slice of the tile's 64 frames (one
// slice at k = 31, four at k = 7), walks them in order, and the slices are summed in order through LDS; lane j = k owns the bias
// gradient.  sed_dwconv_glu_bwd's second launch sums the partial rows in fp64 in a fixed order (16 lanes per element, then one).
// No atomics anywhere: the same bits on every run.  Frames of a neighbouring clip and rows past R are never read.
#include "common.h"
#include <math.h>

#define DW_TILE 64                          // frames a workgroup owns
#define DW_CH 32                            // channels a workgroup owns
#define DW_MAXK 31
#define DW_ROWS (DW_TILE + DW_MAXK - 1)     // tile + both halos at the widest filter
#define DW_FL (256 / (DW_CH / 4))           // frame lanes: 32
#define BS_ROWS 128                         // rows a workgroup of sed_bn_silu_bwd_reduce owns

namespace {

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }
// four consecutive floats through scalar-width loads (per-channel vectors: no alignment asked of them)
__device__ __forceinline__ f32x4 ld4u(const float* p) { return (f32x4){p[0], p[1], p[2], p[3]}; }

struct DwGeom {
    int B, t, C, k, ntile;
};

// the filter taps of the workgroup's channels, tap-major: ws[j][cc]; zero past C
__device__ __forceinline__ void stage_taps(float (*ws)[DW_CH], const float* __restrict__ w, int c0, int C, int k, int tid) {
    for (int idx = tid; idx < k * DW_CH; idx += 256) {
        const int j = idx / DW_CH, cc = idx % DW_CH;
        ws[j][cc] = c0 + cc < C ? w[(size_t)(c0 + cc) * k + j] : 0.f;
    }
}

// sum of red[which][0 .. DW_FL) per channel in a fixed order -> partial[part][which][c]   (threads 0 .. 63)
__device__ __forceinline__ void write_stat_partials(float (*red)[DW_FL][DW_CH], float* __restrict__ partial, size_t part, int c0, int C,
                                                    int tid) {
    if (tid < 2 * DW_CH) {
        const int which = tid / DW_CH, cc = tid % DW_CH;
        float sum = 0.f;
        for (int r = 0; r < DW_FL; ++r) sum += red[which][r][cc];
        if (c0 + cc < C) partial[(part * 2 + which) * C + c0 + cc] = sum;
    }
}

__global__ __launch_bounds__(256) void dwconv_glu_fwd_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ z,
                                                             float* __restrict__ v, float* __restrict__ partial, DwGeom geo) {
    __shared__ float vs[DW_ROWS][DW_CH];
    __shared__ float ws[DW_MAXK][DW_CH];
    __shared__ float red[2][DW_FL][DW_CH];
    const int tid = threadIdx.x, cq = tid % (DW_CH / 4), fr = tid / (DW_CH / 4);
    const int tile = blockIdx.x, c0 = blockIdx.y * DW_CH, b = blockIdx.z;
    const int k = geo.k, p = (k - 1) >> 1, t = geo.t, C = geo.C;
    const int i0 = tile * DW_TILE, c = c0 + 4 * cq;
    const bool cact = c < C;
    const size_t row0 = (size_t)b * t;
    stage_taps(ws, w, c0, C, k, tid);
    const int nrows = DW_TILE + 2 * p;
    for (int r = fr; r < nrows; r += DW_FL) {
        const int f = i0 - p + r;
        f32x4 val = {0.f, 0.f, 0.f, 0.f};
        if (cact && f >= 0 && f < t) {
            const float* gp = g + (row0 + f) * (size_t)(2 * C) + c;
            const f32x4 a = ld4(gp), gate = ld4(gp + C);
#pragma unroll
            for (int q = 0; q < 4; ++q) val[q] = a[q] * sigmoid_f(gate[q]);
            if (v != nullptr && r >= p && r < p + DW_TILE) st4(v + (row0 + f) * (size_t)C + c, val);
        }
        st4(&vs[r][4 * cq], val);
    }
    __syncthreads();
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, q2 = {0.f, 0.f, 0.f, 0.f};
    const f32x4 bia = cact ? ld4u(bias + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int h = 0; h < DW_TILE / DW_FL; ++h) {
        const int li = fr + DW_FL * h, f = i0 + li;
        if (cact && f < t) {
            f32x4 acc = bia;
            for (int j = 0; j < k; ++j) {
                const f32x4 wv = ld4(&ws[j][4 * cq]), xv = ld4(&vs[li + j][4 * cq]);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = fmaf(wv[q], xv[q], acc[q]);
            }
            st4(z + (row0 + f) * (size_t)C + c, acc);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                s[q] += acc[q];
                q2[q] = fmaf(acc[q], acc[q], q2[q]);
            }
        }
    }
    if (partial != nullptr) {
        st4(&red[0][fr][4 * cq], s);
        st4(&red[1][fr][4 * cq], q2);
        __syncthreads();
        write_stat_partials(red, partial, (size_t)b * geo.ntile + tile, c0, C, tid);
    }
}

__global__ __launch_bounds__(256) void bn_silu_fwd_kernel(const float* __restrict__ z, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, float* __restrict__ s, size_t n4, int C) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int c = (int)((i * 4) % (size_t)C);
    const f32x4 zv = ld4(z + i * 4), sc = ld4u(scale + c), sh = ld4u(shift + c);
    f32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float y = fmaf(zv[q], sc[q], sh[q]);
        o[q] = y * sigmoid_f(y);
    }
    st4(s + i * 4, o);
}

__global__ __launch_bounds__(256) void bn_silu_bwd_reduce_kernel(const float* __restrict__ ds, const float* __restrict__ z,
                                                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                                                 const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                 float* __restrict__ gz, float* __restrict__ partial, size_t R, int C) {
    __shared__ float red[2][DW_FL][DW_CH];
    const int tid = threadIdx.x, cq = tid % (DW_CH / 4), rl = tid / (DW_CH / 4);
    const int c0 = blockIdx.y * DW_CH, c = c0 + 4 * cq;
    const bool cact = c < C;
    const size_t r0 = (size_t)blockIdx.x * BS_ROWS;
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, q2 = {0.f, 0.f, 0.f, 0.f};
    if (cact) {
        const f32x4 sc = ld4u(scale + c), sh = ld4u(shift + c), mu = ld4u(mean + c), is = ld4u(invstd + c);
#pragma unroll
        for (int h = 0; h < BS_ROWS / DW_FL; ++h) {
            const size_t r = r0 + rl + DW_FL * h;
            if (r < R) {
                const f32x4 dv = ld4(ds + r * C + c), zv = ld4(z + r * C + c);
                f32x4 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float y = fmaf(zv[q], sc[q], sh[q]);
                    const float sg = sigmoid_f(y);
                    o[q] = dv[q] * (sg * fmaf(y, 1.f - sg, 1.f));
                    s[q] += o[q];
                    q2[q] = fmaf(o[q], (zv[q] - mu[q]) * is[q], q2[q]);
                }
                st4(gz + r * C + c, o);
            }
        }
    }
    st4(&red[0][rl][4 * cq], s);
    st4(&red[1][rl][4 * cq], q2);
    __syncthreads();
    write_stat_partials(red, partial, blockIdx.x, c0, C, tid);
}

__global__ __launch_bounds__(256) void dwconv_glu_bwd_kernel(const float* __restrict__ gz, const float* __restrict__ z,
                                                             const float* __restrict__ ca, const float* __restrict__ cb,
                                                             const float* __restrict__ cc, const float* __restrict__ v,
                                                             const float* __restrict__ g, const float* __restrict__ w,
                                                             float* __restrict__ dg, float* __restrict__ wpart, DwGeom geo) {
    __shared__ float dzs[DW_ROWS][DW_CH];
    __shared__ float vs[DW_ROWS][DW_CH];
    __shared__ float ws[DW_MAXK][DW_CH];
    __shared__ float wred[DW_FL][DW_CH];
    const int tid = threadIdx.x, cq = tid % (DW_CH / 4), fr = tid / (DW_CH / 4);
    const int tile = blockIdx.x, c0 = blockIdx.y * DW_CH, b = blockIdx.z;
    const int k = geo.k, p = (k - 1) >> 1, t = geo.t, C = geo.C;
    const int i0 = tile * DW_TILE, c = c0 + 4 * cq;
    const bool cact = c < C;
    const size_t row0 = (size_t)b * t;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    stage_taps(ws, w, c0, C, k, tid);
    const f32x4 a4 = cact ? ld4u(ca + c) : zero, b4 = cact ? ld4u(cb + c) : zero, c4 = cact ? ld4u(cc + c) : zero;
    const int nrows = DW_TILE + 2 * p;
    for (int r = fr; r < nrows; r += DW_FL) {
        const int f = i0 - p + r;
        f32x4 dz = zero, vv = zero;
        if (cact && f >= 0 && f < t) {
            const size_t o = (row0 + f) * (size_t)C + c;
            const f32x4 gv = ld4(gz + o), zv = ld4(z + o);
#pragma unroll
            for (int q = 0; q < 4; ++q) dz[q] = fmaf(a4[q], gv[q], fmaf(b4[q], zv[q], c4[q]));
            vv = ld4(v + o);
        }
        st4(&dzs[r][4 * cq], dz);
        st4(&vs[r][4 * cq], vv);
    }
    __syncthreads();
    // the data gradient: dv from the dz rows, then through the GLU into both halves of dg
#pragma unroll
    for (int h = 0; h < DW_TILE / DW_FL; ++h) {
        const int li = fr + DW_FL * h, f = i0 + li;
        if (cact && f < t) {
            f32x4 acc = zero;
            for (int j = 0; j < k; ++j) {
                const f32x4 wv = ld4(&ws[j][4 * cq]), dv = ld4(&dzs[li + 2 * p - j][4 * cq]);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = fmaf(wv[q], dv[q], acc[q]);
            }
            const size_t o = (row0 + f) * (size_t)(2 * C) + c;
            const f32x4 a = ld4(g + o), gate = ld4(g + o + C);
            f32x4 da, dgate;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float sg = sigmoid_f(gate[q]);
                da[q] = acc[q] * sg;
                dgate[q] = acc[q] * a[q] * (sg * (1.f - sg));
            }
            st4(dg + o, da);
            st4(dg + o + C, dgate);
        }
    }
    // the filter and bias gradients of this tile: the 32 frame lanes are nslice slices of the tile x nj taps (nj = the power of two that
    // holds the k taps and the bias, j = k); a lane walks its slice's frames in order, the slices are then summed in order through LDS
    int nj = 4;
    while (nj < k + 1) nj <<= 1;
    const int nslice = DW_FL / nj, j = fr % nj, slice = fr / nj, per = DW_TILE / nslice;
    f32x4 acc = zero;
    if (cact && j < k) {
        for (int li = slice * per; li < (slice + 1) * per; ++li) {
            const f32x4 dz = ld4(&dzs[li + p][4 * cq]), vv = ld4(&vs[li + j][4 * cq]);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = fmaf(dz[q], vv[q], acc[q]);
        }
    } else if (cact && j == k) {
        for (int li = slice * per; li < (slice + 1) * per; ++li) {
            const f32x4 dz = ld4(&dzs[li + p][4 * cq]);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += dz[q];
        }
    }
    st4(&wred[fr][4 * cq], acc);
    __syncthreads();
    if (cact && slice == 0 && j <= k) {
        f32x4 sum = ld4(&wred[j][4 * cq]);
        for (int sl = 1; sl < nslice; ++sl) {
            const f32x4 o = ld4(&wred[sl * nj + j][4 * cq]);
#pragma unroll
            for (int q = 0; q < 4; ++q) sum[q] += o[q];
        }
        st4(wpart + (((size_t)b * geo.ntile + tile) * (k + 1) + j) * C + c, sum);
    }
}

#define FIN_EL 16         // elements of the (k + 1) x C gradient a workgroup of the finalisation owns ...
#define FIN_PL 16         // ... and the lanes that share the partial rows of one element

// dw[c][j] = sum over the partial rows of wpart[.][j][c] (fp64), dbias[c] = the same of row j = k: lane pl of an element sums rows pl,
// pl + FIN_PL, ... in order, then one lane sums the FIN_PL lanes in order
__global__ __launch_bounds__(FIN_EL * FIN_PL) void dwconv_wgrad_finalize_kernel(const float* __restrict__ wpart, int nparts,
                                                                              float* __restrict__ dw, float* __restrict__ dbias, int C,
                                                                              int k) {
    __shared__ double sm[FIN_PL][FIN_EL];
    const int e = threadIdx.x % FIN_EL, pl = threadIdx.x / FIN_EL;
    const int idx = blockIdx.x * FIN_EL + e, n = (k + 1) * C;
    double sum = 0.0;
    if (idx < n)
        for (int i = pl; i < nparts; i += FIN_PL) sum += (double)wpart[(size_t)i * n + idx];
    sm[pl][e] = sum;
    __syncthreads();
    if (pl == 0 && idx < n) {
        double tot = sm[0][e];
        for (int i = 1; i < FIN_PL; ++i) tot += sm[i][e];
        const int j = idx / C, c = idx % C;
        if (j < k) dw[(size_t)c * k + j] = (float)tot;
        else dbias[c] = (float)tot;
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline bool geom_ok(int B, int t, int C, int k) {
    return B > 0 && t > 0 && C > 0 && B <= 65535 && cdiv(C, DW_CH) <= 65535 && C % 4 == 0 && k >= 3 && k <= DW_MAXK && (k & 1) &&
           (size_t)t * 2 * C * 4 < ((size_t)1 << 31) && (size_t)B * cdiv(t, DW_TILE) < ((size_t)1 << 31);
}

}  // namespace

extern "C" int sed_dwconv_tile(void) { return DW_TILE; }

extern "C" int sed_dwconv_nparts(int B, int t) { return B > 0 && t > 0 ? B * cdiv(t, DW_TILE) : 0; }

extern "C" size_t sed_dwconv_glu_fwd_ws_floats(int B, int t, int C) { return (size_t)sed_dwconv_nparts(B, t) * 2 * (C > 0 ? C : 0); }

extern "C" int sed_dwconv_glu_fwd(const float* g, const float* w, const float* bias, float* z, float* v, float* partial, int B, int t,
                                  int C, int k, void* stream) {
    SED_REQUIRE(geom_ok(B, t, C, k), "B, t, C > 0, C % 4 == 0, k odd in [3, 31], t*2C*4 < 2^31 bytes, B <= 65535");
    SED_REQUIRE(g != nullptr && w != nullptr && bias != nullptr && z != nullptr, "g, w, bias and z are required (v and partial are optional)");
    SED_REQUIRE(aligned16(g) && aligned16(z) && aligned16(v), "g, z and v must be 16-byte aligned");
    const DwGeom geo = {B, t, C, k, cdiv(t, DW_TILE)};
    dwconv_glu_fwd_kernel<<<dim3(geo.ntile, cdiv(C, DW_CH), B), 256, 0, (hipStream_t)stream>>>(g, w, bias, z, v, partial, geo);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_bn_silu_fwd(const float* z, const float* scale, const float* shift, float* s, size_t R, int C, void* stream) {
    SED_REQUIRE(R > 0 && C > 0 && C % 4 == 0 && cdivz(R * (size_t)C / 4, 256) < ((size_t)1 << 31), "R, C > 0, C % 4 == 0");
    SED_REQUIRE(z != nullptr && scale != nullptr && shift != nullptr && s != nullptr, "every pointer is required");
    SED_REQUIRE(aligned16(z) && aligned16(s), "z and s must be 16-byte aligned");
    const size_t n4 = R * (size_t)C / 4;
    bn_silu_fwd_kernel<<<(unsigned)cdivz(n4, 256), 256, 0, (hipStream_t)stream>>>(z, scale, shift, s, n4, C);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_bn_silu_bwd_nparts(size_t R) { return R > 0 && cdivz(R, BS_ROWS) < ((size_t)1 << 31) ? (int)cdivz(R, BS_ROWS) : 0; }

extern "C" int sed_bn_silu_bwd_reduce(const float* ds, const float* z, const float* scale, const float* shift, const float* mean,
                                      const float* invstd, float* gz, float* partial, size_t R, int C, void* stream) {
    SED_REQUIRE(R > 0 && C > 0 && C % 4 == 0 && cdiv(C, DW_CH) <= 65535 && sed_bn_silu_bwd_nparts(R) > 0, "R, C > 0, C % 4 == 0");
    SED_REQUIRE(ds != nullptr && z != nullptr && scale != nullptr && shift != nullptr && mean != nullptr && invstd != nullptr &&
                    gz != nullptr && partial != nullptr,
                "every pointer is required");
    SED_REQUIRE(aligned16(ds) && aligned16(z) && aligned16(gz), "ds, z and gz must be 16-byte aligned");
    bn_silu_bwd_reduce_kernel<<<dim3(sed_bn_silu_bwd_nparts(R), cdiv(C, DW_CH)), 256, 0, (hipStream_t)stream>>>(ds, z, scale, shift, mean,
                                                                                                                 invstd, gz, partial, R, C);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t sed_dwconv_glu_bwd_ws_floats(int B, int t, int C, int k) {
    return geom_ok(B, t, C, k) ? (size_t)sed_dwconv_nparts(B, t) * (k + 1) * C : 0;
}

extern "C" int sed_dwconv_glu_bwd(const float* gz, const float* z, const float* ca, const float* cb, const float* cc, const float* v,
                                  const float* g, const float* w, float* dg, float* dw, float* dbias, float* workspace, int B, int t,
                                  int C, int k, void* stream) {
    SED_REQUIRE(geom_ok(B, t, C, k), "B, t, C > 0, C % 4 == 0, k odd in [3, 31], t*2C*4 < 2^31 bytes, B <= 65535");
    SED_REQUIRE(gz != nullptr && z != nullptr && ca != nullptr && cb != nullptr && cc != nullptr && v != nullptr && g != nullptr &&
                    w != nullptr && dg != nullptr && dw != nullptr && dbias != nullptr && workspace != nullptr,
                "every pointer is required");
    SED_REQUIRE(aligned16(gz) && aligned16(z) && aligned16(v) && aligned16(g) && aligned16(dg) && aligned16(workspace),
                "gz, z, v, g, dg and the workspace must be 16-byte aligned");
    const DwGeom geo = {B, t, C, k, cdiv(t, DW_TILE)};
    hipStream_t st = (hipStream_t)stream;
    dwconv_glu_bwd_kernel<<<dim3(geo.ntile, cdiv(C, DW_CH), B), 256, 0, st>>>(gz, z, ca, cb, cc, v, g, w, dg, workspace, geo);
    SED_LAUNCH_CHECK();
    dwconv_wgrad_finalize_kernel<<<cdiv((long long)(k + 1) * C, FIN_EL), FIN_EL * FIN_PL, 0, st>>>(workspace, B * geo.ntile, dw, dbias, C, k);
    SED_LAUNCH_CHECK();
    return 0;
}
