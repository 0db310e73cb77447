// Width-general 3x3 convolution kernels: any line width 1 <= W <= 256, chosen at run time (the mel-bin count of the input is a
// model setting; the specialised kernels of sed_conv.hip / sed_conv_wgrad.hip / sed_conv_pc.hip / sed_wgrad*.hip are compiled for W = 8 / 16 / 32 / 64).
//
// forward / data gradient (the contract of sed_conv3x3_fwd): implicit GEMM, D[cout][pixel] = W[cout][k] * X[k][pixel] with
//   k = (tap, 32-channel chunk).  A tile is TH = max(1, 256 / W) whole image rows; its TH*W pixels are padded to 256 MFMA rows
//   (4 waves along M x 2 tiles of 32) and the padding rows are masked in the stores and the statistics.  The (TH+2) x (W+2) halo of
//   one 32-channel chunk (prologue applied, zeros outside the image) and the chunk's weights are staged in LDS; every lane
//   computes its pixel's (row, column, LDS offset) once per launch.  The epilogue stores from the accumulator and forms the
//   BatchNorm statistics partials [nparts][2][Coutp] (SED_EPI_STATS: sum z, sum z^2; SED_EPI_RELUBWD: sum g, sum g*xhat) in the
//   layout sed_bn_train_finalize / sed_bn_bwd_finalize read.
// weight gradient (the contract of sed_conv3x3_wgrad, dz given): dW[tap][cin][cout] = sum_pix a[pix + tap][cin] * dz[pix][cout].
//   The reduction index runs over the tile's pixels in the halo's row pitch (W + 2): pixel (row, col) is k = row*(W+2) + col, and
//   tap (ti, tj) reads halo pixel k + ti*(W+2) + tj -- a uniform shift for every lane.  dz is zero at the two pitch columns
//   col >= W and at rows past the image, so those k contribute nothing.  Both operands are [pixel][channel] in LDS; bf16 fragments
//   come from ds_read_b64_tr_b16 as in conv_wgrad2_kernel (sed_conv_wgrad.hip), whose wave layout (tap row x 32-cout slab) and per-strip fp32 slabs
//   [strips][9][Cinp][Coutp] this kernel keeps, so the reduction (inline or deferred) is the existing one.
// Storage types: bf16 (v_mfma_f32_32x32x16_bf16) and fp32 (v_mfma_f32_32x32x2f32, exact products as the other fp32 kernels); both
// accumulate in fp32.
#include "conv_common.h"

namespace {

constexpr int kAwBM = 256;          // MFMA rows (pixels) of a forward tile
constexpr int kAwK = 256;           // pitch pixels of a weight-gradient tile (before rounding up to 16)

// LDS pixel stride in elements: bf16 80 B (16-byte fragment reads of 32 consecutive pixels are conflict-free, 8-byte transpose
// reads stay aligned); fp32 33 words (one element per lane: consecutive pixels on consecutive banks)
template <typename T> struct AwPS { static constexpr int v = sizeof(T) == 2 ? 40 : 33; };

inline __host__ __device__ int aw_fwd_rows(int W) { const int t = kAwBM / W; return t < 1 ? 1 : t; }
inline __host__ __device__ int aw_wg_rows(int W) { const int t = kAwK / (W + 2); return t < 1 ? 1 : t; }
inline __host__ __device__ int aw_round8(int n) { return (n + 7) & ~7; }

// one 8-channel item of the halo: pro(x[b][h][w][c0 .. c0+7]) or zeros outside the image -> LDS
template <typename T, int PRO>
__device__ __forceinline__ void aw_stage_item(T* __restrict__ dst, const T* __restrict__ xg, bool ok, size_t off,
                                              const float* __restrict__ sc, const float* __restrict__ sh, int c0) {
    float v[8];
    if (ok) {
        load8<T>(xg + off, v);
        if (PRO == SED_PRO_BNRELU) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = fmaxf(0.f, fmaf(v[e], sc[c0 + e], sh[c0 + e]));
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
    }
    if constexpr (sizeof(T) == 2) {
        store8<T>(dst, v);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) dst[e] = v[e];
    }
}

// stage the (rows x (W+2)) halo of channels [c0, c0+32) of image b, first halo row h0 - 1
template <typename T, int PRO>
__device__ __forceinline__ void aw_stage_halo(T* __restrict__ xs, const T* __restrict__ xg, int b, int h0, int rows, int H, int W,
                                              int Cinp, int c0, const float* __restrict__ sc, const float* __restrict__ sh,
                                              int tid, int nthr) {
    constexpr int PS = AwPS<T>::v;
    const int WP = W + 2;
    const int items = rows * WP * 4;
    for (int it = tid; it < items; it += nthr) {
        const int pix = it >> 2, cq = it & 3;
        const int rowi = pix / WP, coli = pix - rowi * WP;
        const int h = h0 - 1 + rowi, w = coli - 1;
        const bool ok = h >= 0 && h < H && w >= 0 && w < W;
        const size_t off = ok ? (((size_t)b * H + h) * W + w) * Cinp + c0 + cq * 8 : 0;
        aw_stage_item<T, PRO>(xs + pix * PS + cq * 8, xg, ok, off, sc, sh, c0 + cq * 8);
    }
}

// =================================================================================================
// forward / data gradient
// =================================================================================================
template <typename T, int WN, int PRO, int EPI>
__global__ __launch_bounds__(256 * WN) void conv_anyw_kernel(ConvParams p, int W) {
    constexpr int BN = 32 * WN;
    constexpr int NTHR = 256 * WN;
    constexpr int MT = kAwBM / 128;          // 32-pixel tiles per wave (4 waves along M)
    typedef typename EL<T>::frag_t frag_t;
    constexpr int KR = EL<T>::KR, KSTEP = EL<T>::KSTEP;
    constexpr int PS = AwPS<T>::v;
    constexpr int WS = 9 * 32 * BN;          // elements of one weight chunk
    const int TH = aw_fwd_rows(W), WP = W + 2, ROWS = TH + 2;
    const int npx = TH * W;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* xs = reinterpret_cast<T*>(smem);
    T* ws = xs + aw_round8(ROWS * WP * PS);

    const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3, wn = tid >> 8;
    const int r = lane & 31, hh = lane >> 5;
    const int NY = p.Coutp / BN;
    const int by = blockIdx.x % NY, bx = blockIdx.x / NY;
    const int n0 = by * BN;
    const int H = p.H, Cinp = p.Cinp, Coutp = p.Coutp;
    const int nchunks = Cinp >> 5;
    const T* __restrict__ xg = reinterpret_cast<const T*>(p.x);
    const T* __restrict__ wg = reinterpret_cast<const T*>(p.wpack);
    T* __restrict__ zg = reinterpret_cast<T*>(p.z);
    const T* __restrict__ zr = reinterpret_cast<const T*>(p.zref);

    // tile-invariant per-lane pixel map
    int prow[MT], pcol[MT], xbase[MT];
    bool qok[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int q = (wave * MT + mt) * 32 + r;
        qok[mt] = q < npx;
        prow[mt] = qok[mt] ? q / W : 0;
        pcol[mt] = qok[mt] ? q - prow[mt] * W : 0;
        xbase[mt] = (prow[mt] * WP + pcol[mt]) * PS;      // padding rows read pixel 0's (finite) halo and are never stored
    }
    // the lane's 16 output channels: register i = 4*g + e -> channel n0 + wn*32 + 8*g + 4*hh + e
    const int chl = n0 + wn * 32 + 4 * hh;
    float ces[16], cet[16], cem[16];
    if (EPI == SED_EPI_RELUBWD) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = chl + 8 * (i >> 2) + (i & 3);
            ces[i] = p.epi_scale[c]; cet[i] = p.epi_shift[c]; cem[i] = p.epi_mean[c];
        }
    }
    float S[16], Q[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { S[i] = 0.f; Q[i] = 0.f; }

    const int t_begin = bx * p.tpb;
    const int t_end = min(p.totalTiles, t_begin + p.tpb);
    bool w_staged = false;
    for (int tile = t_begin; tile < t_end; ++tile) {
        const int b = tile / p.tilesPerImg;
        const int h0 = (tile - b * p.tilesPerImg) * TH;
        f32x16 acc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
        for (int kc = 0; kc < nchunks; ++kc) {
            __syncthreads();                               // previous stage's readers of xs / ws are done
            aw_stage_halo<T, PRO>(xs, xg, b, h0, ROWS, H, W, Cinp, kc * 32, p.pro_scale, p.pro_shift, tid, NTHR);
            if (nchunks > 1 || !w_staged) {
                // weight rows (tap, kq) of BN*KR contiguous elements; source row stride Coutp*KR
                constexpr int IPR = BN * KR / 8;
                for (int it = tid; it < WS / 8; it += NTHR) {
                    const int row = it / IPR, off = (it - row * IPR) * 8;
                    const T* src = wg + ((size_t)(kc * 9 * (32 / KR) + row) * Coutp + n0) * KR + off;
                    lds_store_raw<T>(ws + row * BN * KR + off, raw_load8<T>(src));
                }
                w_staged = true;
            }
            __syncthreads();
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int toff = ((tap / 3) * WP + (tap % 3)) * PS;
#pragma unroll 4
                for (int ks = 0; ks < 32 / KSTEP; ++ks) {
                    const int kb = ks * KSTEP + hh * KR;   // first channel of this lane's fragment
                    const frag_t wf = *reinterpret_cast<const frag_t*>(ws + ((tap * (32 / KR) + kb / KR) * BN + wn * 32 + r) * KR);
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        const frag_t xf = *reinterpret_cast<const frag_t*>(xs + xbase[mt] + toff + kb);
                        acc[mt] = mfma(wf, xf, acc[mt]);
                    }
                }
            }
        }
        // ---- epilogue straight from the accumulators: lane = pixel, 4 consecutive channels per register group ----
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int h = h0 + prow[mt];
            if (!qok[mt] || h >= H) continue;
            const size_t po = (((size_t)b * H + h) * W + pcol[mt]) * Coutp;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[mt][4 * g + e];
                const int c = chl + 8 * g;
                if (EPI == SED_EPI_STATS) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { S[4 * g + e] += v[e]; Q[4 * g + e] = fmaf(v[e], v[e], Q[4 * g + e]); }
                } else if (EPI == SED_EPI_RELUBWD) {
                    float z[4];
                    load4<T>(zr + po + c, z);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int i = 4 * g + e;
                        const float gate = fmaf(z[e], ces[i], cet[i]) > 0.f ? v[e] : 0.f;
                        v[e] = gate;
                        S[i] += gate;
                        Q[i] = fmaf(gate, z[e] - cem[i], Q[i]);
                    }
                }
                store4<T>(zg + po + c, v);
            }
        }
    }

    // ---- per-workgroup statistics partial (every workgroup writes its row, zeros if it had no tile) ----------------
    if (EPI == SED_EPI_STATS || EPI == SED_EPI_RELUBWD) {
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);   // [wn][wave][quarter][stat][16]
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float sv = row16_sum(S[i]);
            const float qv = row16_sum(Q[i]);
            if ((lane & 15) == 0) {
                const int quarter = lane >> 4;
                red[(((wn * 4 + wave) * 4 + quarter) * 2 + 0) * 16 + i] = sv;
                red[(((wn * 4 + wave) * 4 + quarter) * 2 + 1) * 16 + i] = qv;
            }
        }
        __syncthreads();
        if (tid < 2 * BN) {
            const int stat = tid / BN, cn = tid % BN;
            const int wcol = cn >> 5, within = cn & 31;
            const int hhh = (within >> 2) & 1;
            const int reg = (within & 3) + 4 * (within >> 3);
            float tot = 0.f;
#pragma unroll
            for (int wv = 0; wv < 4; ++wv)
#pragma unroll
                for (int qq = 0; qq < 2; ++qq)
                    tot += red[(((wcol * 4 + wv) * 4 + 2 * hhh + qq) * 2 + stat) * 16 + reg];
            if (EPI == SED_EPI_RELUBWD && stat) tot *= p.epi_invstd[n0 + cn];
            p.partial[((size_t)bx * 2 + stat) * Coutp + n0 + cn] = tot;
        }
    }
}

// =================================================================================================
// weight gradient, dz given
// =================================================================================================
template <typename T, int WN, int PRO>
__global__ __launch_bounds__(192 * WN) void wgrad_anyw_kernel(Wgrad2Params p, int W) {
    typedef typename EL<T>::frag_t frag_t;
    constexpr int KSTEP = EL<T>::KSTEP;
    constexpr int NTHR = 192 * WN;
    constexpr int CO = 32 * WN;
    constexpr int PS = AwPS<T>::v;
    const int TH = aw_wg_rows(W), WP = W + 2, ROWS = TH + 2;
    const int KP = TH * WP, KPr = (KP + 15) & ~15;
    const int XPIX = ROWS * WP + 17;                   // + the pixels a rounded-up k range shifted by the last tap reaches

    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* xs = reinterpret_cast<T*>(smem);                // [XPIX][PS]
    T* dzs = xs + aw_round8(XPIX * PS);                // [WN][KPr][PS]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wt = wave % 3, wn = wave / 3;
    const int r = lane & 31, hh = lane >> 5;
    const int H = p.H, Cinp = p.Cinp, Coutp = p.Coutp;
    const int NCO = Coutp / CO;
    const int NY = (Cinp >> 5) * NCO;
    const int strip = blockIdx.x / NY, yb = blockIdx.x - strip * NY;
    const int ci0 = (yb / NCO) * 32, co0 = (yb % NCO) * CO;
    const T* __restrict__ xg = reinterpret_cast<const T*>(p.x);
    const T* __restrict__ dg = reinterpret_cast<const T*>(p.dz);

    // the tail pixels are never staged: zero (finite) once
    for (int i = tid; i < (XPIX - ROWS * WP) * PS; i += NTHR) xs[ROWS * WP * PS + i] = (T)0.f;

    f32x16 acc[3];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

    // transpose-read lane offsets (bf16): the lane supplies k-row 8*hh + qq (+4 for the second half), channels ch .. ch+3
    int offA[2], offB[2];
    {
        const int i16 = lane & 15, gbit = (lane >> 4) & 1;
        const int qq = i16 >> 2, pp = i16 & 3, ch = 16 * gbit + 4 * pp;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int kl = 8 * hh + qq + 4 * half;
            offA[half] = kl * PS + ch;
            offB[half] = kl * PS + ch;
        }
    }
    const T* __restrict__ dzw = dzs + (size_t)wn * KPr * PS;

    const int t_begin = strip * p.tpb;
    const int t_end = min(p.totalTiles, t_begin + p.tpb);
    for (int tile = t_begin; tile < t_end; ++tile) {
        const int b = tile / p.tilesPerImg;
        const int h0 = (tile - b * p.tilesPerImg) * TH;
        __syncthreads();                               // previous tile's readers are done
        aw_stage_halo<T, PRO>(xs, xg, b, h0, ROWS, H, W, Cinp, ci0, p.pro_scale, p.pro_shift, tid, NTHR);
        {   // dz in pitch order: k = row*(W+2) + col, zero at col >= W, rows past the image and the rounding tail
            constexpr int IPP = CO / 8;
            const int items = KPr * IPP;
            for (int it = tid; it < items; it += NTHR) {
                const int k = it / IPP, c8 = (it - k * IPP) * 8;
                const int row = k / WP, col = k - row * WP;
                const int h = h0 + row;
                const bool ok = k < KP && col < W && h < H;
                const size_t off = ok ? (((size_t)b * H + h) * W + col) * Coutp + co0 + c8 : 0;
                aw_stage_item<T, SED_PRO_NONE>(dzs + ((c8 >> 5) * KPr + k) * PS + (c8 & 31), dg, ok, off, nullptr, nullptr, 0);
            }
        }
        __syncthreads();
        for (int k0 = 0; k0 < KPr; k0 += KSTEP) {
            frag_t bf;
            frag_t af[3];
            if constexpr (sizeof(T) == 2) {
                bf = join_tr(ds_read_tr16_b64(dzw + k0 * PS + offB[0]), ds_read_tr16_b64(dzw + k0 * PS + offB[1]));
#pragma unroll
                for (int tj = 0; tj < 3; ++tj) {
                    const T* xa = xs + (k0 + wt * WP + tj) * PS;
                    af[tj] = join_tr(ds_read_tr16_b64(xa + offA[0]), ds_read_tr16_b64(xa + offA[1]));
                }
            } else {
                const int k = k0 + hh;
                bf = dzw[k * PS + r];
#pragma unroll
                for (int tj = 0; tj < 3; ++tj) af[tj] = xs[(k + wt * WP + tj) * PS + r];
            }
#pragma unroll
            for (int tj = 0; tj < 3; ++tj) acc[tj] = mfma(af[tj], bf, acc[tj]);
        }
    }

    // each wave stores its own 3 taps x 32 cin x 32 cout slab: D row = cin, col (lane) = cout
    float* out = p.ws + (size_t)strip * 9 * Cinp * Coutp;
#pragma unroll
    for (int tj = 0; tj < 3; ++tj) {
        const int tap = wt * 3 + tj;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int cin = ci0 + (i & 3) + 8 * (i >> 2) + 4 * hh;
            out[((size_t)tap * Cinp + cin) * Coutp + co0 + wn * 32 + r] = acc[tj][i];
        }
    }
}

template <typename T, int WN, int PRO, int EPI>
int launch_fwd(ConvParams& p, int W, hipStream_t st) {
    constexpr int BN = 32 * WN;
    constexpr int PS = AwPS<T>::v;
    const int TH = aw_fwd_rows(W);
    const size_t lds = ((size_t)aw_round8((TH + 2) * (W + 2) * PS) + (size_t)9 * 32 * BN) * sizeof(T);
    if (int rc_ = sed_set_max_lds<&conv_anyw_kernel<T, WN, PRO, EPI>>(lds)) return rc_;
    p.tilesPerImg = cdiv(p.H, TH);
    p.totalTiles = p.B * p.tilesPerImg;
    p.tpb = cdiv(p.totalTiles, p.nparts);
    conv_anyw_kernel<T, WN, PRO, EPI><<<dim3(p.nparts * (p.Coutp / BN)), dim3(256 * WN), lds, st>>>(p, W);
    return 0;
}

template <typename T, int WN>
int dispatch_fwd(ConvParams& p, int W, hipStream_t st) {
    if (p.pro == SED_PRO_NONE && p.epi == SED_EPI_STATS) return launch_fwd<T, WN, SED_PRO_NONE, SED_EPI_STATS>(p, W, st);
    if (p.pro == SED_PRO_BNRELU && p.epi == SED_EPI_STATS) return launch_fwd<T, WN, SED_PRO_BNRELU, SED_EPI_STATS>(p, W, st);
    if (p.pro == SED_PRO_NONE && p.epi == SED_EPI_STORE) return launch_fwd<T, WN, SED_PRO_NONE, SED_EPI_STORE>(p, W, st);
    if (p.pro == SED_PRO_BNRELU && p.epi == SED_EPI_STORE) return launch_fwd<T, WN, SED_PRO_BNRELU, SED_EPI_STORE>(p, W, st);
    if (p.pro == SED_PRO_NONE && p.epi == SED_EPI_RELUBWD) return launch_fwd<T, WN, SED_PRO_NONE, SED_EPI_RELUBWD>(p, W, st);
    if (p.pro == SED_PRO_BNRELU && p.epi == SED_EPI_RELUBWD) return launch_fwd<T, WN, SED_PRO_BNRELU, SED_EPI_RELUBWD>(p, W, st);
    sed_set_error("sed_conv3x3_fwd (any width): unsupported prologue/epilogue combination");
    return 1;
}

template <typename T, int WN, int PRO>
int launch_wg(Wgrad2Params& p, int W, hipStream_t st) {
    constexpr int PS = AwPS<T>::v;
    const int TH = aw_wg_rows(W);
    const int KPr = (TH * (W + 2) + 15) & ~15;
    const size_t lds = ((size_t)aw_round8(((TH + 2) * (W + 2) + 17) * PS) + (size_t)WN * KPr * PS) * sizeof(T);
    if (int rc_ = sed_set_max_lds<&wgrad_anyw_kernel<T, WN, PRO>>(lds)) return rc_;
    p.tilesPerImg = cdiv(p.H, TH);
    p.totalTiles = p.B * p.tilesPerImg;
    if (p.strips > p.totalTiles) p.strips = p.totalTiles;      // (never more slabs than the caller's workspace holds)
    if (p.strips < 1) p.strips = 1;
    p.tpb = cdiv(p.totalTiles, p.strips);
    const int ny = (p.Cinp / 32) * (p.Coutp / (32 * WN));
    wgrad_anyw_kernel<T, WN, PRO><<<dim3(p.strips * ny), dim3(192 * WN), lds, st>>>(p, W);
    return 0;
}

template <typename T, int WN>
int dispatch_wg(Wgrad2Params& p, int W, hipStream_t st) {
    return p.pro == SED_PRO_BNRELU ? launch_wg<T, WN, SED_PRO_BNRELU>(p, W, st) : launch_wg<T, WN, SED_PRO_NONE>(p, W, st);
}

}  // namespace

int launch_conv_anyw(int dtype, ConvParams& p, int W, hipStream_t st) {
    if (W < 1 || W > SED_ANYW_MAX_W) { sed_set_error("sed_conv3x3_fwd: W must be in [1, 256]"); return 1; }
    // fp32 keeps one 32-channel N tile per workgroup: halo + weights of two stay inside the LDS at W = 256
    if (dtype == SED_BF16) return p.Coutp % 64 == 0 ? dispatch_fwd<bf16_t, 2>(p, W, st) : dispatch_fwd<bf16_t, 1>(p, W, st);
    if (dtype == SED_F32) return dispatch_fwd<float, 1>(p, W, st);
    sed_set_error("sed_conv3x3_fwd: at W outside {8, 16, 32, 64} only SED_BF16 and SED_F32 are covered");
    return 1;
}

int launch_wgrad_anyw(int dtype, int dzmode, Wgrad2Params& p, int W, hipStream_t st) {
    if (W < 1 || W > SED_ANYW_MAX_W) { sed_set_error("sed_conv3x3_wgrad: W must be in [1, 256]"); return 1; }
    if (dtype != SED_BF16 && dtype != SED_F32) {
        sed_set_error("sed_conv3x3_wgrad: at W outside {8, 16, 32, 64} only SED_BF16 and SED_F32 are covered");
        return 1;
    }
    if (dzmode != DZ_GIVEN) {
        // the fused forms by composition: the width-agnostic backward kernels write dz into dz_out, the dz-given kernel reads it
        if (p.dz_out == nullptr) { sed_set_error("sed_conv3x3_wgrad_fused: at W outside {8, 16, 32, 64} dz_out is required"); return 1; }
        int rc;
        if (dzmode == DZ_POOL)
            rc = sed_pool_relu_bn_bwd_apply(dtype, p.dz, p.zsrc, p.scale, p.shift, p.ca, p.cb, p.cc, p.dz_out, p.B, p.H, W, p.Coutp,
                                            p.pool, st);
        else
            rc = sed_bn_bwd_apply(dtype, p.dz, p.zsrc, p.ca, p.cb, p.cc, p.dz_out, (size_t)p.B * p.H * W, p.Coutp, st);
        if (rc) return rc;
        p.dz = p.dz_out;
    }
    if (dtype == SED_BF16) return p.Coutp % 64 == 0 ? dispatch_wg<bf16_t, 2>(p, W, st) : dispatch_wg<bf16_t, 1>(p, W, st);
    return dispatch_wg<float, 1>(p, W, st);
}
