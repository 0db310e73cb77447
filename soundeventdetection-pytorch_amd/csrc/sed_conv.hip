// 3x3 convolution kernels for gfx950 (CDNA4): implicit GEMM on MFMA over LDS-staged NHWC tiles.  This file holds the fp32 and
// fallback forward / data-gradient kernels (conv_igemm_kernel, conv_wreg_kernel) and the forward / data-gradient entry points
// with their dispatch to the faster kernels (sed_conv_pc.hip, sed_conv_x3.hip, sed_conv_anyw.hip).  The rest of the conv entry
// layer: weight packing and slab reduction in sed_conv_pack.hip, the weight gradient in sed_conv_wgrad.hip, the Cin = 1 first
// layer and the C1-mode entries in sed_c1.hip.
//
// Replaces nn.Conv2d(3x3, s1, p1, bias=False) forward / autograd backward of ConvBlock
// (models/spectogram_models.py:132-140,155-156 of the reference).
//
// Orientation: D[cout][pixel] += Wfrag[cout][k] * Xfrag[k][pixel]   (k = input channels of a tap)
//   - MFMA 32x32x16 bf16 (or 32x32x2 f32 in the fp32-accurate mode): A operand = weights,
//     B operand = activations, so the accumulator has the PIXEL on the lane and 4 consecutive
//     output channels in consecutive registers -> NHWC stores of 8/16 B per lane, and per-channel
//     BatchNorm statistics accumulate per lane across tiles and are reduced once per workgroup.
//   - activations: LDS image [rows+2][W+2 (pitch WP)][32 ch], XOR-swizzled per pixel column so that
//     the 32 pixels of a fragment read hit distinct banks; the 9 taps are 9 shifted reads of it.
//   - weights: pre-packed by sed_pack_conv_weight() (sed_conv_pack.hip) to [chunk][tap][32/KR][Coutp][KR] so both the
//     global->LDS copy and the fragment read are linear.
#include "conv_common.h"

// xs[(rowi*WP + coli)*32 + swizzled channel] <- pro(x[b][h0-1+rowi][coli-1][c0 + ..32 channels])
template <typename T, int W, int ROWS, int NTHR> struct HaloRegs {
    static constexpr int ITEMS = ROWS * (W + 2) * 4;
    static constexpr int IPT = (ITEMS + NTHR - 1) / NTHR;
    Raw8<T> raw[IPT];
    bool ok[IPT];
};

// phase 1: every global load of the thread, back to back
template <typename T, int W, int ROWS, int NTHR>
__device__ __forceinline__ void halo_issue(HaloRegs<T, W, ROWS, NTHR>& hr, const T* __restrict__ xg, int b, int h0,
                                           int H, int Cinp, int c0, int tid) {
    typedef HaloRegs<T, W, ROWS, NTHR> HR;
    const int cq = tid & 3;
#pragma unroll
    for (int u = 0; u < HR::IPT; ++u) {
        const int it = tid + u * NTHR;
        const int pix = it >> 2;
        const int rowi = pix / (W + 2), coli = pix - rowi * (W + 2);
        const int h = h0 - 1 + rowi, w = coli - 1;
        hr.ok[u] = (it < HR::ITEMS) && h >= 0 && h < H && w >= 0 && w < W;
        const size_t off = hr.ok[u] ? ((((size_t)b * H + h) * W + w) * Cinp + c0 + cq * 8) : (size_t)(c0 + cq * 8);
        hr.raw[u] = raw_load8<T>(xg + off);
    }
}

// phase 2: prologue + LDS writes.  PS = LDS pixel stride in elements: 32 -> XOR-swizzled channels,
// 40 (bf16 only) -> linear with 16 B of padding per pixel (80 B stride: 5p mod 16 visits every 16-B
// slot, so ds_read_b128 fragment reads are conflict-free AND tap shifts are plain immediates).
template <typename T, int W, int ROWS, int WP, int NTHR, int PS = 32>
__device__ __forceinline__ void halo_commit(const HaloRegs<T, W, ROWS, NTHR>& hr, T* __restrict__ xs, int c0, int pro,
                                            const float* __restrict__ pro_scale, const float* __restrict__ pro_shift,
                                            int tid) {
    typedef HaloRegs<T, W, ROWS, NTHR> HR;
    const int cq = tid & 3;
    float sc[8], sh[8];
    if (pro == SED_PRO_BNRELU) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { sc[e] = pro_scale[c0 + cq * 8 + e]; sh[e] = pro_shift[c0 + cq * 8 + e]; }
    }
#pragma unroll
    for (int u = 0; u < HR::IPT; ++u) {
        const int it = tid + u * NTHR;
        if (it < HR::ITEMS) {
            const int pix = it >> 2;
            const int rowi = pix / (W + 2), coli = pix - rowi * (W + 2);
            float v[8];
            raw_to_f(hr.raw[u], v);
            if (pro == SED_PRO_BNRELU) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = fmaxf(0.f, fmaf(v[e], sc[e], sh[e]));
            }
            if (!hr.ok[u]) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = 0.f;
            }
            T* dst = xs + (rowi * WP + coli) * PS;
            if constexpr (PS != 32) {
                store8<T>(dst + cq * 8, v);
            } else {
                const int sx = swz<T>(coli);
                if constexpr (sizeof(T) == 2) {
                    store8<T>(dst + ((cq * 8) ^ sx), v);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) dst[(cq * 8 + e) ^ sx] = v[e];
                }
            }
        }
    }
}

// =================================================================================================
// generic implicit-GEMM conv (forward and data gradient)
// =================================================================================================

template <typename T, int W, int BM, int WN, int PRO, int EPI>
__global__ __launch_bounds__(256 * WN, 2) void conv_igemm_kernel(ConvParams p) {
    constexpr int BN = 32 * WN;          // output channels per workgroup: one 32-wide N tile per wave column
    constexpr int NTHR = 256 * WN;
    typedef typename EL<T>::frag_t frag_t;
    constexpr int KR = EL<T>::KR, KSTEP = EL<T>::KSTEP;
    constexpr int ES = (int)sizeof(T);
    constexpr int TH = BM / W;
    constexpr int WP = (W + 2 + 3) & ~3;
    constexpr int ROWS = TH + 2;
    constexpr int PS = (sizeof(T) == 2) ? 40 : 32;   // LDS pixel stride: padded-linear (bf16) / XOR-swizzled (f32)
    constexpr int XS = ROWS * WP * PS;   // elements
    constexpr int WS = 9 * 32 * BN;      // elements
    constexpr int MT = BM / 128;         // 32-pixel tiles per wave (4 waves along M)
    constexpr int WITEMS = WS / 8;       // 8-element items of one weight chunk
    constexpr int WIPT = (WITEMS + NTHR - 1) / NTHR;
    static_assert(BM % 128 == 0 && BM % W == 0, "tile shape");
    typedef HaloPlan<T, W, ROWS, WP, NTHR, PS> XPlan;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const bool wres = p.wres != 0;
    const int nchunks_ = p.Cinp >> 5;
    T* xs = reinterpret_cast<T*>(smem);
    T* ws = xs + XS;                                     // [wres ? nchunks : 1][WS]
    T* os = ws + (wres ? nchunks_ : 1) * WS;             // [BM][BN + pad]: output staging of the coalesced epilogue

    const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3, wn = tid >> 8;
    const int r = lane & 31, hh = lane >> 5;
    const int NY = p.Coutp / BN;
    const unsigned logical = xcd_remap(blockIdx.x, gridDim.x);
    const int by = logical % NY, bx = logical / NY;
    const int n0 = by * BN;
    const int H = p.H, Cinp = p.Cinp, Coutp = p.Coutp;
    const int nchunks = Cinp >> 5;
    const T* __restrict__ xg = reinterpret_cast<const T*>(p.x);
    const T* __restrict__ wg = reinterpret_cast<const T*>(p.wpack);
    T* __restrict__ zg = reinterpret_cast<T*>(p.z);
    const T* __restrict__ zr = reinterpret_cast<const T*>(p.zref);
    constexpr int epi = EPI;             // compile-time: straight-line prologue/epilogue code

    // ---- tile-invariant per-lane coordinates / offsets ----------------------------------------------------
    int prow[MT], xbase[MT];
    unsigned eoff[MT];                   // byte offset of the lane's first output channel inside the image, tile row 0
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int q = (wave * MT + mt) * 32 + r;
        prow[mt] = q / W;
        const int rot = (PS == 32) ? 0 : (W == 16) ? 12 * (prow[mt] & 1) : (W == 8) ? 4 * ((((prow[mt] & 3) + 1) >> 1) & 1) : 0;
        const int pcol = (q % W + rot) % W;
        xbase[mt] = (prow[mt] * WP + pcol) * PS;
        eoff[mt] = (unsigned)(((prow[mt] * W + pcol) * Coutp + n0 + wn * 32 + 4 * hh) * ES);
    }
    XPlan xp;
    xp.init(tid, Cinp);
    // weight chunk items: row (tap, kq) of BN*KR contiguous elements in LDS; source row stride Coutp*KR
    unsigned wsrc[WIPT];
    int wdst[WIPT];
    Raw8<T> wraw[WIPT];
    {
        constexpr int ROWLEN = BN * KR;
        constexpr int ITEMS_PER_ROW = ROWLEN / 8;
#pragma unroll
        for (int u = 0; u < WIPT; ++u) {
            const int it = tid + u * NTHR;
            const int rowi = it / ITEMS_PER_ROW, off = (it - rowi * ITEMS_PER_ROW) * 8;
            const bool ok = it < WITEMS;
            wsrc[u] = ok ? (unsigned)(((rowi * Coutp + n0) * KR + off) * ES) : SED_OOB;
            wdst[u] = ok ? rowi * ROWLEN + off : 0;
        }
    }
    const size_t wchunk_bytes = (size_t)(9 * 32 / KR) * Coutp * KR * ES;     // one 32-input-channel chunk of wpack
    const __amdgpu_buffer_rsrc_t wsrd = make_srd(wg, wchunk_bytes * nchunks);
    const size_t ximg = (size_t)H * W * Cinp, zimg = (size_t)H * W * Coutp;

    float S[16], Q[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { S[i] = 0.f; Q[i] = 0.f; }

    // ---- coalesced epilogue ---------------------------------------------------------------------------------
    // The accumulator has the pixel on the lane and 4 consecutive output channels per register group: stored
    // straight from there, every lane of a store instruction hits a different 128-byte line (8 bytes each).
    // Instead the tile is written to an LDS staging image [pixel][BN (+16 B pad)] and, after the next barrier
    // of the stage loop, read back 16 bytes per lane in pixel-major order: each store instruction then writes
    // whole lines.  The fused ReLU-mask / BatchNorm-backward statistics run in that pass, on coalesced loads of
    // the reference tile (requested one stage ahead): a thread's items all belong to the same 8 channels.
    constexpr int BNP = BN + 16 / ES;
    constexpr int IPR = BN / 8;                   // 8-channel items per staged pixel
    constexpr int FIPT = BM * IPR / NTHR;         // items per thread
    constexpr int FQS = NTHR / IPR;               // pixels between two items of a thread
    static_assert((BM * IPR) % NTHR == 0 && NTHR % IPR == 0, "flush geometry");
    int ostg[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int q = (wave * MT + mt) * 32 + r;
        const int rot = (PS == 32) ? 0 : (W == 16) ? 12 * (prow[mt] & 1) : (W == 8) ? 4 * ((((prow[mt] & 3) + 1) >> 1) & 1) : 0;
        ostg[mt] = (prow[mt] * W + (q % W + rot) % W) * BNP + wn * 32 + 4 * hh;
    }
    const int fcg = tid % IPR, fq0 = tid / IPR;
    const int fl_lds0 = fq0 * BNP + fcg * 8;
    const unsigned fl_off0 = (unsigned)((fq0 * Coutp + n0 + fcg * 8) * ES);
    const unsigned fl_step = (unsigned)(FQS * Coutp * ES);
    Raw8<T> zraw[FIPT];
    float ces[8], cet[8], cem[8];
    if (epi == SED_EPI_RELUBWD) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            ces[e] = p.epi_scale[n0 + fcg * 8 + e];
            cet[e] = p.epi_shift[n0 + fcg * 8 + e];
            cem[e] = p.epi_mean[n0 + fcg * 8 + e];
        }
    }
    int fb = 0, fh0 = 0;
    bool pending = false;
    auto flush = [&]() {
        const __amdgpu_buffer_rsrc_t zs = make_srd(zg + (size_t)fb * zimg, zimg * ES);
        const unsigned tq = (unsigned)(fh0 * W * Coutp * ES);
#pragma unroll
        for (int u = 0; u < FIPT; ++u) {
            float v[8];
            load8<T>(os + fl_lds0 + u * FQS * BNP, v);
            if (epi == SED_EPI_RELUBWD) {
                float z[8];
                raw_to_f(zraw[u], z);
                const bool valid = fh0 + (fq0 + u * FQS) / W < H;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float gate = (valid && fmaf(z[e], ces[e], cet[e]) > 0.f) ? v[e] : 0.f;
                    v[e] = gate;
                    S[e] += gate;
                    Q[e] = fmaf(gate, z[e] - cem[e], Q[e]);
                }
            }
            if (!(SED_DBG(p, 1))) buf_store8<T>(zs, fl_off0 + u * fl_step + tq, v);
        }
    };

    const int t_begin = bx * p.tpb;
    const int t_end = min(p.totalTiles, t_begin + p.tpb);
    const int nst = (t_end > t_begin ? (t_end - t_begin) : 0) * nchunks;   // stages = (tile, chunk)

    auto coords = [&](int s, int& b, int& h0, int& kc) {
        const int tl = s / nchunks;
        kc = s - tl * nchunks;
        const int tile = t_begin + tl;
        b = tile / p.tilesPerImg;
        h0 = (tile - b * p.tilesPerImg) * TH;
    };
    auto issue = [&](int s, bool with_w) {
        int b, h0, kc;
        coords(s, b, h0, kc);
        if (SED_DBG(p, 8)) return;
        xp.issue(make_srd(xg + (size_t)b * ximg, ximg * ES), (unsigned)((((h0 - 1) * W - 1) * Cinp + kc * 32) * ES));
        if (with_w) {
            const unsigned wo = (unsigned)(kc * wchunk_bytes);
#pragma unroll
            for (int u = 0; u < WIPT; ++u) wraw[u] = buf_load8<T>(wsrd, wsrc[u] + wo);
        }
    };
    auto commit = [&](int s, bool with_w) {
        int b, h0, kc;
        coords(s, b, h0, kc);
        const int row_hi = (H - h0 < ROWS - 1) ? (H - h0) : (ROWS - 1);
        xp.template commit<PRO>(xs, tid, p.pro_scale, p.pro_shift, kc * 32, h0 == 0 ? 1 : 0, row_hi);
        if (with_w) {
#pragma unroll
            for (int u = 0; u < WIPT; ++u) {
                if (u == WIPT - 1 && tid + u * NTHR >= WITEMS) break;
                lds_store_raw<T>(ws + wdst[u], wraw[u]);
            }
        }
    };
    if (wres && nst > 0) {      // one-time: every chunk of this N slice into LDS
        for (int c = 0; c < nchunks; ++c) {
            const unsigned wo = (unsigned)(c * wchunk_bytes);
#pragma unroll
            for (int u = 0; u < WIPT; ++u) wraw[u] = buf_load8<T>(wsrd, wsrc[u] + wo);
#pragma unroll
            for (int u = 0; u < WIPT; ++u) {
                if (u == WIPT - 1 && tid + u * NTHR >= WITEMS) break;
                lds_store_raw<T>(ws + c * WS + wdst[u], wraw[u]);
            }
        }
    }
    const bool stage_w_each = !wres && nchunks > 1;

    f32x16 acc[MT];
    if (nst > 0) issue(0, !wres);
    for (int s = 0; s < nst; ++s) {
        int b, h0, kc;
        coords(s, b, h0, kc);
        __syncthreads();                                   // previous stage's readers of xs/ws are done; staging is complete
        if (pending) { flush(); pending = false; }         // previous tile: LDS -> whole-line global stores
        const bool need_w = stage_w_each || (!wres && s == 0);   // single-chunk layers: staged once, stay resident
        commit(s, need_w);
        __syncthreads();
        if (s + 1 < nst) issue(s + 1, stage_w_each);       // next stage's loads fly during the MFMAs below
        if (kc == 0) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
        }
        const unsigned tq = (unsigned)(h0 * W * Coutp * ES);
        if (epi == SED_EPI_RELUBWD && kc == nchunks - 1) {   // reference tile of the flush one stage from now
            const __amdgpu_buffer_rsrc_t rs = make_srd(zr + (size_t)b * zimg, zimg * ES);
#pragma unroll
            for (int u = 0; u < FIPT; ++u) zraw[u] = buf_load8<T>(rs, fl_off0 + u * fl_step + tq);
        }
        // ---- 9 taps x (32/KSTEP) k-steps of MFMA ------------------------------------------------------------
        const T* __restrict__ wsc = ws + (wres ? kc * WS : 0);
        if (!(SED_DBG(p, 2)))
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ti = tap / 3, tj = tap % 3;
#pragma unroll 4
            for (int ks = 0; ks < 32 / KSTEP; ++ks) {
                const int kb = ks * KSTEP + hh * KR;   // first channel of this lane's fragment
                const frag_t wf = *reinterpret_cast<const frag_t*>(wsc + ((tap * (32 / KR) + kb / KR) * BN + wn * 32 + r) * KR);
                frag_t xf[MT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    if constexpr (PS == 32) {
                        const int col = (xbase[mt] / PS) % WP + tj;
                        xf[mt] = *reinterpret_cast<const frag_t*>(xs + xbase[mt] + (ti * WP + tj) * PS + (kb ^ swz<T>(col)));
                    } else {
                        xf[mt] = *reinterpret_cast<const frag_t*>(xs + xbase[mt] + (ti * WP + tj) * PS + kb);
                    }
                }
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma(wf, xf[mt], acc[mt]);
            }
        }
        if (kc != nchunks - 1) continue;

        // ---- tile done: forward statistics from the fp32 accumulators, then stage the tile for the flush ------
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const bool valid = h0 + prow[mt] < H;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[mt][4 * g + e];
                if (epi == SED_EPI_STATS && valid) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { S[4 * g + e] += v[e]; Q[4 * g + e] = fmaf(v[e], v[e], Q[4 * g + e]); }
                }
                store4<T>(os + ostg[mt] + 8 * g, v);
            }
        }
        fb = b; fh0 = h0; pending = true;
    }
    if (pending) {
        __syncthreads();
        flush();
    }

    // ---- per-workgroup statistics partial ------------------------------------------------------
    if (epi == SED_EPI_STATS) {
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);   // [wn][wave][quarter][stat][16] (reuses the tile buffers)
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
            p.partial[((size_t)bx * 2 + stat) * Coutp + n0 + cn] = tot;
        }
    } else if (epi == SED_EPI_RELUBWD) {
        // thread t accumulated channels 8*(t % IPR) .. +7 over its pixels: fixed-order sum over the FQS threads
        // of each channel group; Q was accumulated as gate*(z - mean), the 1/std factor is applied here
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);   // [NTHR][16]
#pragma unroll
        for (int e = 0; e < 8; ++e) { red[tid * 16 + e] = S[e]; red[tid * 16 + 8 + e] = Q[e]; }
        __syncthreads();
        if (tid < 2 * BN) {
            const int stat = tid / BN, cn = tid % BN;
            const int cg = cn >> 3, e = cn & 7;
            float tot = 0.f;
            for (int k = 0; k < FQS; ++k) tot += red[(cg + IPR * k) * 16 + stat * 8 + e];
            if (stat) tot *= p.epi_invstd[n0 + cn];
            p.partial[((size_t)bx * 2 + stat) * Coutp + n0 + cn] = tot;
        }
    }
}

// =================================================================================================
// bf16 fast path: weights stationary in REGISTERS.
//   Each wave owns 32 output channels (wn) and MT 32-pixel tiles (wm): its 18 A-fragments of the
//   current 32-channel chunk (9 taps x 2 k-steps, 72 VGPRs) are loaded straight from the packed
//   weights in L2 (coalesced 16 B/lane) -- once per workgroup when Cin = 32, otherwise prefetched
//   for the next chunk into a second register set while the current chunk computes.  Only the
//   activation halo tile goes through LDS (double buffered; the next stage's global loads are in
//   flight during the MFMAs, its LDS writes follow them; ONE barrier per stage), and every MFMA
//   needs exactly one ds_read_b128 (the B-fragment), half of what the LDS-weights tiling needs.
//   One wave per SIMD (up to 512 registers): the overlap is explicit, not by occupancy.
// =================================================================================================
template <int W, int WM, int WN, int PRO, int EPI>
__global__ __launch_bounds__(256) void conv_wreg_kernel(ConvParams p) {
    typedef bf16_t T;
    constexpr int BM = 256;
    constexpr int MT = BM / (32 * WM);
    constexpr int TH = BM / W;
    constexpr int WP = (W + 2 + 3) & ~3;
    constexpr int ROWS = TH + 2;
    constexpr int PS = 40;               // padded LDS pixel stride (elements)
    constexpr int XS = ROWS * WP * PS;
    constexpr int BN = 32 * WN;
    static_assert(WM * WN == 4, "four waves");
    typedef HaloRegs<T, W, ROWS, 256> HR;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* xs0 = reinterpret_cast<T*>(smem);
    T* xs1 = xs0 + XS;
    constexpr int BNP = BN + 8;          // output staging row (elements): BN channels + 16 bytes of padding
    T* os = xs1 + XS;                    // [BM][BNP]: output staging of the coalesced epilogue (see conv_igemm_kernel)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int r = lane & 31, hh = lane >> 5;
    const int NY = p.Coutp / BN;
    const unsigned logical = xcd_remap(blockIdx.x, gridDim.x);
    const int by = logical % NY, bx = logical / NY;
    const int n0 = by * BN, cw = n0 + wn * 32;
    const int H = p.H, Cinp = p.Cinp, Coutp = p.Coutp;
    const int nchunks = Cinp >> 5;
    const T* __restrict__ xg = reinterpret_cast<const T*>(p.x);
    const bf16x8* __restrict__ wg8 = reinterpret_cast<const bf16x8*>(p.wpack);
    T* __restrict__ zg = reinterpret_cast<T*>(p.z);
    constexpr int pro = PRO, epi = EPI;

    int prow[MT], pcol[MT], xbase[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int q = (wm * MT + mt) * 32 + r;
        prow[mt] = q / W;
        // A 32-pixel MFMA tile spans 32/W rows; rotating the columns of some rows (found by exhaustive
        // search over the ds_read_b128 lane groups) keeps the padded layout bank-conflict free:
        // W=16: odd rows +12; W=8: rows 1,2 (mod 4) +4.  Any lane->pixel bijection is legal.
        const int rot = (W == 16) ? 12 * (prow[mt] & 1) : (W == 8) ? 4 * ((((prow[mt] & 3) + 1) >> 1) & 1) : 0;
        pcol[mt] = (q % W + rot) % W;
        xbase[mt] = (prow[mt] * WP + pcol[mt]) * PS + hh * 8;   // + (ti*WP + tj)*PS + ks*16: immediates
    }

    f32x16 acc[MT];

    // 18 A-fragments of chunk kc: wpack[kc][tap][kq = 2*ks + hh][Coutp][8]
    auto load_w = [&](bf16x8 (&wf)[18], int kc) {
#pragma unroll
        for (int t = 0; t < 18; ++t)
            wf[t] = wg8[(size_t)((kc * 9 + (t >> 1)) * 4 + (t & 1) * 2 + hh) * Coutp + cw + r];
    };

    // 18 groups (tap, k-step) of MT MFMAs.  Both operand sets are refilled IN PLACE: the B-fragment of
    // M tile mt is re-read from LDS for group g+1 right after its MFMA of group g has issued (it is
    // needed MT MFMAs later), and -- when the next stage uses another chunk (`refill`) -- weight fragment
    // g is re-loaded from L2 after its last MFMA (needed a whole stage later).  One fragment set each;
    // the fences stop the scheduler from hoisting everything and spilling.
    auto xfrag = [&](const T* __restrict__ xs, int g, int mt) -> bf16x8 {
        const int tap = g >> 1, ks = g & 1;
        const int ti = tap / 3, tj = tap % 3;
        return *reinterpret_cast<const bf16x8*>(xs + xbase[mt] + (ti * WP + tj) * PS + ks * 16);
    };
    auto compute = [&](bf16x8 (&wf)[18], const T* __restrict__ xs, bool refill, int kc_next) {
        bf16x8 xf[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) xf[mt] = xfrag(xs, 0, mt);
#pragma unroll
        for (int g = 0; g < 18; ++g) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[g], xf[mt], acc[mt], 0, 0, 0);
                if (g + 1 < 18) xf[mt] = xfrag(xs, g + 1, mt);
            }
            if (refill) wf[g] = wg8[(size_t)((kc_next * 9 + (g >> 1)) * 4 + (g & 1) * 2 + hh) * Coutp + cw + r];
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // tile done: it goes to the LDS staging image [pixel][BN + pad] and is written out with whole-line stores
    // by flush() after the stage's barrier.  The forward BatchNorm statistics are taken there too, from the
    // values as stored (bf16), 8 fixed channels per thread, accumulated in a thread-owned LDS slot: this
    // kernel has no registers left for 32 persistent accumulators (they spilled to scratch).
    static_assert(EPI != SED_EPI_RELUBWD, "the fused ReLU/BN-backward epilogue runs in conv_igemm_kernel");
    auto epilogue = [&]() {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int ob = (prow[mt] * W + pcol[mt]) * BNP + wn * 32 + 4 * hh;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[mt][4 * g + e];
                store4<T>(os + ob + 8 * g, v);
            }
        }
    };
    constexpr int IPR = BN / 8, FIPT = BM * IPR / 256, FQS = 256 / IPR;
    const int fcg = tid % IPR, fq0 = tid / IPR;
    const size_t zimg = (size_t)H * W * Coutp;
    float* sslot = reinterpret_cast<float*>(os + BM * BNP) + tid * 16;   // [256][S 0..7, Q 0..7]
    if (epi == SED_EPI_STATS) {
#pragma unroll
        for (int e = 0; e < 16; ++e) sslot[e] = 0.f;
    }
    int fb = 0, fh0 = 0;
    bool pending = false;
    auto flush = [&]() {
        const __amdgpu_buffer_rsrc_t zs = make_srd(zg + (size_t)fb * zimg, zimg * 2);
        const unsigned base = (unsigned)(((fh0 * W + fq0) * Coutp + n0 + fcg * 8) * 2);
        float ts[8], tq[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { ts[e] = 0.f; tq[e] = 0.f; }
#pragma unroll
        for (int u = 0; u < FIPT; ++u) {
            const bf16x8 v = *reinterpret_cast<const bf16x8*>(os + (fq0 + u * FQS) * BNP + fcg * 8);
            if (epi == SED_EPI_STATS && fh0 + (fq0 + u * FQS) / W < H) {
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float f = (float)v[e]; ts[e] += f; tq[e] = fmaf(f, f, tq[e]); }
            }
            if (!(SED_DBG(p, 1)))    // rows past the image: dropped by the descriptor's range check
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), zs, base + (unsigned)(u * FQS * Coutp * 2), 0, 0);
        }
        if (epi == SED_EPI_STATS) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { sslot[e] += ts[e]; sslot[8 + e] += tq[e]; }
        }
    };

    const int t_begin = bx * p.tpb;
    const int t_end = min(p.totalTiles, t_begin + p.tpb);
    const int nst = (t_end > t_begin ? (t_end - t_begin) : 0) * nchunks;   // stages = (tile, chunk) pairs

    auto stage_coords = [&](int s, int& b, int& h0, int& kc) {
        const int tile = t_begin + s / nchunks;
        kc = s - (s / nchunks) * nchunks;
        b = tile / p.tilesPerImg;
        h0 = (tile - b * p.tilesPerImg) * TH;
    };

    bf16x8 wf[18];
    HR hr;
    if (nst > 0) {
        int b, h0, kc;
        stage_coords(0, b, h0, kc);
        load_w(wf, 0);
        halo_issue<T, W, ROWS, 256>(hr, xg, b, h0, H, Cinp, 0, tid);
        halo_commit<T, W, ROWS, WP, 256, PS>(hr, xs0, 0, pro, p.pro_scale, p.pro_shift, tid);
    }
    __syncthreads();

    // one stage: issue stage s+1's activation loads (-> hr), compute stage s from xs[s&1] (refilling
    // the weight fragments for stage s+1 on the way), then write stage s+1's activations into the
    // other LDS buffer; ONE barrier per stage.
    for (int s = 0; s < nst; ++s) {
        int b, h0, kc;
        stage_coords(s, b, h0, kc);
        const bool more = (s + 1 < nst);
        int b1 = 0, h1 = 0, kc1 = 0;
        if (pending) { flush(); pending = false; }   // staged by every wave before the barrier that ended the last stage
        if (more) {
            stage_coords(s + 1, b1, h1, kc1);
            halo_issue<T, W, ROWS, 256>(hr, xg, b1, h1, H, Cinp, kc1 * 32, tid);
        }
        if (kc == 0) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
        }
        if (!(SED_DBG(p, 2))) compute(wf, (s & 1) ? xs1 : xs0, more && nchunks > 1, kc1);
        // (the next write of the staging image is >= 2 stages = one more barrier away: nchunks >= 2 here)
        if (kc == nchunks - 1) { epilogue(); fb = b; fh0 = h0; pending = true; }
        if (more) halo_commit<T, W, ROWS, WP, 256, PS>(hr, (s & 1) ? xs0 : xs1, kc1 * 32, pro, p.pro_scale, p.pro_shift, tid);
        __syncthreads();
    }
    if (pending) flush();

    // ---- per-workgroup statistics partial ------------------------------------------------------
    if (epi == SED_EPI_STATS) {
        // fixed-order sum over the FQS threads that own each channel group
        __syncthreads();
        const float* slots = reinterpret_cast<const float*>(os + BM * BNP);
        if (tid < 2 * BN) {
            const int stat = tid / BN, cn = tid % BN;
            const int cg = cn >> 3, e = cn & 7;
            float tot = 0.f;
            for (int k = 0; k < FQS; ++k) tot += slots[(cg + IPR * k) * 16 + stat * 8 + e];
            p.partial[((size_t)bx * 2 + stat) * Coutp + n0 + cn] = tot;
        }
    }
}

// =================================================================================================
// host launchers (C ABI)
// =================================================================================================
static const int kMaxParts = 1024;

extern "C" int sed_conv_nparts(int B, int H, int W) {
    const long long tiles = (long long)B * cdiv((long long)H * W, 256);
    return (int)(tiles < kMaxParts ? tiles : kMaxParts);
}

// the (prologue, epilogue) pairs the training / inference paths use
#define SED_PE_DISPATCH(CALL)                                                                         \
    do {                                                                                              \
        if (p.pro == SED_PRO_NONE && p.epi == SED_EPI_STATS) return CALL(SED_PRO_NONE, SED_EPI_STATS);       \
        if (p.pro == SED_PRO_BNRELU && p.epi == SED_EPI_STATS) return CALL(SED_PRO_BNRELU, SED_EPI_STATS);   \
        if (p.pro == SED_PRO_NONE && p.epi == SED_EPI_STORE) return CALL(SED_PRO_NONE, SED_EPI_STORE);       \
        if (p.pro == SED_PRO_BNRELU && p.epi == SED_EPI_STORE) return CALL(SED_PRO_BNRELU, SED_EPI_STORE);   \
        if (p.pro == SED_PRO_NONE && p.epi == SED_EPI_RELUBWD) return CALL(SED_PRO_NONE, SED_EPI_RELUBWD);   \
        sed_set_error("sed_conv3x3_fwd: unsupported prologue/epilogue combination");                  \
        return 1;                                                                                     \
    } while (0)

template <typename T, int W, int BM, int WN, int PRO, int EPI>
static int launch_conv(ConvParams& p, hipStream_t st) {
    constexpr int BN = 32 * WN;
    constexpr int TH = BM / W;
    constexpr int WP = (W + 2 + 3) & ~3;
    constexpr int PS = (sizeof(T) == 2) ? 40 : 32;
    constexpr size_t lds_x = (size_t)(TH + 2) * WP * PS * sizeof(T);
    constexpr size_t lds_w1 = (size_t)9 * 32 * BN * sizeof(T);
    constexpr size_t lds_o = (size_t)BM * (BN + 16 / sizeof(T)) * sizeof(T);     // output staging (coalesced epilogue)
    const int nchunks = p.Cinp / 32;
    // multi-chunk layers keep every weight chunk resident when that fits beside the activation tile
    p.wres = (nchunks > 1 && lds_x + nchunks * lds_w1 + lds_o <= 150 * 1024) ? 1 : 0;
    const size_t lds = lds_x + (p.wres ? nchunks : 1) * lds_w1 + lds_o;
    if (int rc_ = sed_set_max_lds<&conv_igemm_kernel<T, W, BM, WN, PRO, EPI>>(lds)) return rc_;
    p.tilesPerImg = cdiv(p.H, TH);
    p.totalTiles = p.B * p.tilesPerImg;
    p.tpb = cdiv(p.totalTiles, p.nparts);
    const int ny = p.Coutp / BN;
    conv_igemm_kernel<T, W, BM, WN, PRO, EPI><<<dim3(p.nparts * ny), dim3(256 * WN), lds, st>>>(p);
    return 0;
}

template <typename T, int W, int BM>
static int dispatch_conv_pe(ConvParams& p, hipStream_t st) {
    if (p.Coutp % 64 == 0) {
#define SED_CALL(P_, E_) launch_conv<T, W, BM, 2, P_, E_>(p, st)
        SED_PE_DISPATCH(SED_CALL);
#undef SED_CALL
    } else {
#define SED_CALL(P_, E_) launch_conv<T, W, BM, 1, P_, E_>(p, st)
        SED_PE_DISPATCH(SED_CALL);
#undef SED_CALL
    }
}

template <typename T, int BM>
static int dispatch_conv_w(ConvParams& p, int W, hipStream_t st) {
    switch (W) {
        case 8: return dispatch_conv_pe<T, 8, BM>(p, st);
        case 16: return dispatch_conv_pe<T, 16, BM>(p, st);
        case 32: return dispatch_conv_pe<T, 32, BM>(p, st);
        case 64: return dispatch_conv_pe<T, 64, BM>(p, st);
    }
    sed_set_error("sed_conv3x3_fwd: W must be one of 8,16,32,64");
    return 1;
}

template <int W, int WM, int WN, int PRO, int EPI>
static int launch_wreg(ConvParams& p, hipStream_t st) {
    constexpr int BM = 256;
    constexpr int TH = BM / W;
    constexpr int WP = (W + 2 + 3) & ~3;
    constexpr size_t lds = (size_t)2 * (TH + 2) * WP * 40 * sizeof(bf16_t) + (size_t)BM * (32 * WN + 8) * sizeof(bf16_t) +
                           (EPI == SED_EPI_STATS ? 256 * 16 * sizeof(float) : 0);
    if (int rc_ = sed_set_max_lds<&conv_wreg_kernel<W, WM, WN, PRO, EPI>>(lds)) return rc_;
    p.tilesPerImg = cdiv(p.H, TH);
    p.totalTiles = p.B * p.tilesPerImg;
    p.tpb = cdiv(p.totalTiles, p.nparts);
    const int ny = p.Coutp / (32 * WN);
    conv_wreg_kernel<W, WM, WN, PRO, EPI><<<dim3(p.nparts * ny), dim3(256), lds, st>>>(p);
    return 0;
}

template <int W>
static int dispatch_wreg_pe(ConvParams& p, hipStream_t st) {
    // only the 128-output-channel configuration is dispatched to this kernel (see sed_conv3x3_fwd)
    if (p.pro == SED_PRO_NONE && p.epi == SED_EPI_STATS) return launch_wreg<W, 1, 4, SED_PRO_NONE, SED_EPI_STATS>(p, st);
    if (p.pro == SED_PRO_BNRELU && p.epi == SED_EPI_STATS) return launch_wreg<W, 1, 4, SED_PRO_BNRELU, SED_EPI_STATS>(p, st);
    if (p.pro == SED_PRO_NONE && p.epi == SED_EPI_STORE) return launch_wreg<W, 1, 4, SED_PRO_NONE, SED_EPI_STORE>(p, st);
    if (p.pro == SED_PRO_BNRELU && p.epi == SED_EPI_STORE) return launch_wreg<W, 1, 4, SED_PRO_BNRELU, SED_EPI_STORE>(p, st);
    sed_set_error("sed_conv3x3_fwd: unsupported prologue/epilogue combination for the register-weights kernel");
    return 1;
}

static int dispatch_wreg(ConvParams& p, int W, hipStream_t st) {
    switch (W) {
        case 8: return dispatch_wreg_pe<8>(p, st);
        case 16: return dispatch_wreg_pe<16>(p, st);
        case 32: return dispatch_wreg_pe<32>(p, st);
        case 64: return dispatch_wreg_pe<64>(p, st);
    }
    sed_set_error("sed_conv3x3_fwd: W must be one of 8,16,32,64");
    return 1;
}

static int conv3x3_fwd_impl(int dtype, int pro, int epi, const void* x, const float* pro_scale,
                            const float* pro_shift, const void* wpack, void* z, const void* zref,
                            const float* epi_scale, const float* epi_shift, const float* epi_mean,
                            const float* epi_invstd, float* partial, int B, int H, int W, int Cinp, int Coutp,
                            void* stream, int col_only, bool anyw = false) {
    // SED_F32H3: bits 8..15 of dtype = signed power-of-two exponent applied to the streamed operand x before the fp16 split (gradients)
    const int xexp = (int)(signed char)((dtype >> 8) & 0xff);
    dtype &= 0xff;
    SED_REQUIRE(xexp == 0 || dtype == SED_F32H3, "an operand exponent belongs to dtype SED_F32H3");
    SED_REQUIRE(Cinp % 32 == 0 && Coutp % 32 == 0 && Cinp > 0 && Coutp > 0, "channels must be padded to 32");
    SED_REQUIRE(B > 0 && H > 0, "empty input");
    SED_REQUIRE(pro == SED_PRO_NONE || (pro == SED_PRO_BNRELU && pro_scale && pro_shift), "prologue operands");
    SED_REQUIRE(epi == SED_EPI_STORE || partial, "epilogue needs a partial buffer");
    SED_REQUIRE(epi != SED_EPI_RELUBWD || (zref && epi_scale && epi_shift && epi_mean && epi_invstd), "epilogue operands");
    // buffer addressing: one descriptor per image, 32-bit byte offsets inside it
    SED_REQUIRE((double)H * W * (Cinp > Coutp ? Cinp : Coutp) * (dtype == SED_BF16 ? 2 : 4) < 2147483648.0,
                "one image (H*W*C elements) must stay below 2 GiB");
    ConvParams p = {};
    p.x = x; p.pro_scale = pro_scale; p.pro_shift = pro_shift; p.wpack = wpack; p.z = z; p.zref = zref;
    p.epi_scale = epi_scale; p.epi_shift = epi_shift; p.epi_mean = epi_mean; p.epi_invstd = epi_invstd;
    p.partial = partial; p.B = B; p.H = H; p.Cinp = Cinp; p.Coutp = Coutp; p.pro = pro; p.epi = epi; p.wres = 0;
    p.col_only = col_only;
    p.xexp = xexp;
    p.dbg = sed_dbg_env();
    p.nparts = sed_conv_nparts(B, H, W);
    int rc;
    // widths outside the specialised set (and the direct _anyw entry): the width-general kernels (csrc/sed_conv_anyw.hip)
    if (anyw || !sed_w_specialised(W)) {
        rc = launch_conv_anyw(dtype, p, W, (hipStream_t)stream);
        if (rc) return rc;
        SED_LAUNCH_CHECK();
        return 0;
    }
    // bf16: the register-stationary-weights kernel wins when a workgroup covers 128 output channels
    // (MFMA-bound layers); the LDS-weights kernel (2 workgroups/CU) wins on the low-channel,
    // memory-bound layers.  SED_CONV_KERNEL=lds|wreg forces one of them (A/B runs).
    const char* force = sed_getenv("SED_CONV_KERNEL");
    // (its fused ReLU/BN-backward epilogue variant does not fit the register file with MT = 8: that
    // one always takes the LDS-weights kernel)
    // register-resident weights (sed_conv_wir.hip) for the >= 64-channel layers it covers; SED_CONV_KERNEL=r forces it
    // where it applies, =p keeps the producer/consumer kernel everywhere (A/B runs)
#ifdef SED_EXPERIMENTS     // (make EXPERIMENTS=1: the two opt-in resident-weight kernels, measured <= the producer/consumer kernel)
    if (dtype == SED_BF16 && force && force[0] == 'r') {
        const int rc_w = launch_conv_wir(p, W, (hipStream_t)stream);
        if (rc_w > 0) return rc_w;
        if (rc_w == 0) { SED_LAUNCH_CHECK(); return 0; }
    }
    // one wave per SIMD, all weights of its 32 output channels in registers (sed_conv_w4.hip); SED_CONV_KERNEL=4
    if (dtype == SED_BF16 && force && force[0] == '4') {
        const int rc_w = launch_conv_w4(p, W, (hipStream_t)stream);
        if (rc_w > 0) return rc_w;
        if (rc_w == 0) { SED_LAUNCH_CHECK(); return 0; }
    }
#else
    SED_REQUIRE(!(force && (force[0] == 'r' || force[0] == '4')), "SED_CONV_KERNEL=r/4 need a library built with make EXPERIMENTS=1");
#endif
    if (dtype == SED_BF16 && !(force && force[0] != 'p' && force[0] != 'r' && force[0] != '4')) {      // producer/consumer kernel (sed_conv_pc.hip) where it covers the shape
        const int rc_pc = launch_conv_pc(p, W, (hipStream_t)stream);
        if (rc_pc > 0) return rc_pc;
        if (rc_pc == 0) { SED_LAUNCH_CHECK(); return 0; }
    }
    const bool want_wreg = (Coutp % 128 == 0) && epi != SED_EPI_RELUBWD && Cinp >= 64 && (force ? (force[0] == 'w') : true);
    if (dtype == SED_BF16 && want_wreg) rc = dispatch_wreg(p, W, (hipStream_t)stream);
    else if (dtype == SED_BF16) rc = dispatch_conv_w<bf16_t, 256>(p, W, (hipStream_t)stream);
    else if (dtype == SED_F32) rc = dispatch_conv_w<float, 128>(p, W, (hipStream_t)stream);
    else if (dtype == SED_F32X3 || dtype == SED_F32H3) rc = launch_conv_x3(dtype == SED_F32H3, p, W, (hipStream_t)stream);
    else { sed_set_error("sed_conv3x3_fwd: bad dtype"); return 1; }
    if (rc) return rc;
    SED_LAUNCH_CHECK();
    return 0;
}

// Data gradient whose epilogue also accumulates the pool + ReLU + BatchNorm backward statistics of the block that produced
// its output's forward twin (include/sed_hip.h).  bf16, shapes of the producer/consumer kernel only.
extern "C" int sed_dgrad_poolstats_supported(int dtype, int W, int Cinp, int Coutp) {
    if (!(dtype == SED_BF16 && (W == 8 || W == 16 || W == 32 || W == 64) && Cinp % 32 == 0 && Coutp % 32 == 0 && Cinp > 0 && Coutp > 0))
        return 0;
    ConvParams p = {};      // ask the producer/consumer dispatcher itself (its LDS budget decides for wide layers)
    p.B = 1; p.H = 64; p.Cinp = Cinp; p.Coutp = Coutp; p.pro = SED_PRO_NONE; p.epi = SED_EPI_POOLSTATS; p.nparts = 1; p.dry = 1;
    return launch_conv_pc(p, W, nullptr) == 0;
}

extern "C" int sed_conv3x3_dgrad_poolstats(int dtype, const void* dz, const void* wpack_t, void* dy, const void* y_pooled,
                                           const void* cnt, const float* scale, const float* shift, const float* mean,
                                           const float* invstd, float* partial, int nparts, int* flag, int B, int H, int W,
                                           int Cinp, int Coutp, void* stream) {
    SED_REQUIRE(sed_dgrad_poolstats_supported(dtype, W, Cinp, Coutp), "sed_conv3x3_dgrad_poolstats: bf16, W in {8,16,32,64}, channels padded to 32");
    SED_REQUIRE(B > 0 && H > 0 && dz && wpack_t && dy && y_pooled && cnt && scale && shift && mean && invstd && partial && flag, "operands");
    SED_REQUIRE((double)H * W * (Cinp > Coutp ? Cinp : Coutp) * 2 < 2147483648.0, "one image (H*W*C elements) must stay below 2 GiB");
    ConvParams p = {};
    p.x = dz; p.wpack = wpack_t; p.z = dy; p.zref = y_pooled; p.cnt = reinterpret_cast<const unsigned char*>(cnt); p.flag = flag;
    p.epi_scale = scale; p.epi_shift = shift; p.epi_mean = mean; p.epi_invstd = invstd;
    p.partial = partial; p.B = B; p.H = H; p.Cinp = Cinp; p.Coutp = Coutp; p.pro = SED_PRO_NONE; p.epi = SED_EPI_POOLSTATS;
    p.dbg = sed_dbg_env();
    const int own = sed_conv_nparts(B, H, W);
    SED_REQUIRE(nparts >= own, "partial needs at least sed_conv_nparts(B, H, W) rows");
    p.nparts = nparts;
    const int rc = launch_conv_pc(p, W, (hipStream_t)stream);
    SED_REQUIRE(rc >= 0, "sed_conv3x3_dgrad_poolstats: shape not covered by the producer/consumer kernel");
    if (rc > 0) return rc;
    SED_LAUNCH_CHECK();
    return 0;
}

// Data gradient that PRODUCES dz on load (csrc/sed_conv_pc.hip, SED_PRO_DZBN / SED_PRO_DZPOOL) and writes it out once for the
// weight-gradient call with dz given (include/sed_hip.h).  bf16, W = 16 / 8, dz channels (the layer's outputs) a multiple of 32.
static int dgrad_dz_setup(ConvParams& p, int dzmode, int epi, int B, int H, int C, int Cx, int pool) {
    p.B = B; p.H = H; p.Cinp = C; p.Coutp = Cx; p.epi = epi;
    p.pro = dzmode == SED_DZ_POOL ? SED_PRO_DZPOOL : SED_PRO_DZBN;
    p.dz_pool = dzmode == SED_DZ_POOL ? pool : 1;
    return 0;
}
extern "C" int sed_conv3x3_dgrad_dz_supported(int dtype, int W, int C, int Cx, int dzmode, int epi, int pool) {
    if (!(dtype == SED_BF16 && (W == 8 || W == 16) && C % 32 == 0 && Cx % 32 == 0 && C > 0 && Cx > 0)) return 0;
    if (!(dzmode == SED_DZ_BN || (dzmode == SED_DZ_POOL && (pool == 1 || pool == 2)))) return 0;
    if (dzmode == SED_DZ_BN && !(epi == SED_EPI_STORE || epi == SED_EPI_POOLSTATS)) return 0;
    if (dzmode == SED_DZ_POOL && epi != SED_EPI_RELUBWD) return 0;
#ifndef SED_EXPERIMENTS
    return 0;          // (measured slower than the round-3 order, csrc/sed_conv_pc.hip: built with make EXPERIMENTS=1 only)
#endif
    ConvParams p = {};
    dgrad_dz_setup(p, dzmode, epi, 1, 64, C, Cx, pool);
    p.nparts = 1; p.dry = 1;
    return launch_conv_pc(p, W, nullptr) == 0;
}
extern "C" int sed_conv3x3_dgrad_dz(int dtype, int dzmode, const void* gsrc, const void* zsrc, const float* scale, const float* shift,
                                    const float* ca, const float* cb, const float* cc, int pool, const void* wpack_t, void* dz_out,
                                    void* dx, int epi, const void* zref, const void* cnt, const float* epi_scale, const float* epi_shift,
                                    const float* epi_mean, const float* epi_invstd, float* partial, int nparts, int* flag, int B, int H,
                                    int W, int C, int Cx, void* stream) {
    SED_REQUIRE(sed_conv3x3_dgrad_dz_supported(dtype, W, C, Cx, dzmode, epi, pool),
                "covered: bf16, W = 16 / 8; SED_DZ_BN with STORE / POOLSTATS, SED_DZ_POOL (pool 1 / 2) with RELUBWD");
    SED_REQUIRE(B > 0 && H > 0 && gsrc && zsrc && ca && cb && cc && wpack_t && dz_out && dx, "operands");
    SED_REQUIRE(dzmode != SED_DZ_POOL || (scale && shift), "pool-backward operands");
    SED_REQUIRE(epi == SED_EPI_STORE || (zref && epi_scale && epi_shift && epi_mean && epi_invstd && partial), "epilogue operands");
    SED_REQUIRE(epi != SED_EPI_POOLSTATS || (cnt && flag), "pooled-tensor statistics operands");
    SED_REQUIRE((double)H * W * (C > Cx ? C : Cx) * 2 < 2147483648.0, "one image (H*W*C elements) must stay below 2 GiB");
    ConvParams p = {};
    dgrad_dz_setup(p, dzmode, epi, B, H, C, Cx, pool);
    p.x = zsrc; p.dz_g = gsrc; p.dz_ca = ca; p.dz_cb = cb; p.dz_cc = cc; p.dz_sc = scale; p.dz_sh = shift; p.dz_out = dz_out;
    p.wpack = wpack_t; p.z = dx; p.zref = zref; p.cnt = reinterpret_cast<const unsigned char*>(cnt); p.flag = flag;
    p.epi_scale = epi_scale; p.epi_shift = epi_shift; p.epi_mean = epi_mean; p.epi_invstd = epi_invstd; p.partial = partial;
    p.dbg = sed_dbg_env();
    const int own = sed_conv_nparts(B, H, W);
    SED_REQUIRE(epi == SED_EPI_STORE || nparts >= own, "partial needs at least sed_conv_nparts(B, H, W) rows");
    p.nparts = epi == SED_EPI_STORE ? own : nparts;
    const int rc = launch_conv_pc(p, W, (hipStream_t)stream);
    SED_REQUIRE(rc >= 0, "sed_conv3x3_dgrad_dz: shape not covered by the producer/consumer kernel");
    if (rc > 0) return rc;
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_conv3x3_fwd(int dtype, int pro, int epi, const void* x, const float* pro_scale,
                               const float* pro_shift, const void* wpack, void* z, const void* zref,
                               const float* epi_scale, const float* epi_shift, const float* epi_mean,
                               const float* epi_invstd, float* partial, int B, int H, int W, int Cinp, int Coutp,
                               void* stream) {
    return conv3x3_fwd_impl(dtype, pro, epi, x, pro_scale, pro_shift, wpack, z, zref, epi_scale, epi_shift, epi_mean, epi_invstd,
                            partial, B, H, W, Cinp, Coutp, stream, 0);
}

// the same call for 3x3 weights whose side columns are zero (a k = 3 Conv1d over interleaved frames, W = 8): the covered
// kernels skip the six zero taps, every other path computes them (same result)
extern "C" int sed_conv3x3_fwd_col(int dtype, int pro, int epi, const void* x, const float* pro_scale,
                                   const float* pro_shift, const void* wpack, void* z, const void* zref,
                                   const float* epi_scale, const float* epi_shift, const float* epi_mean,
                                   const float* epi_invstd, float* partial, int B, int H, int W, int Cinp, int Coutp,
                                   void* stream) {
    return conv3x3_fwd_impl(dtype, pro, epi, x, pro_scale, pro_shift, wpack, z, zref, epi_scale, epi_shift, epi_mean, epi_invstd,
                            partial, B, H, W, Cinp, Coutp, stream, 1);
}

extern "C" int sed_conv3x3_fwd_anyw(int dtype, int pro, int epi, const void* x, const float* pro_scale,
                                    const float* pro_shift, const void* wpack, void* z, const void* zref,
                                    const float* epi_scale, const float* epi_shift, const float* epi_mean,
                                    const float* epi_invstd, float* partial, int B, int H, int W, int Cinp, int Coutp,
                                    void* stream) {
    return conv3x3_fwd_impl(dtype, pro, epi, x, pro_scale, pro_shift, wpack, z, zref, epi_scale, epi_shift, epi_mean, epi_invstd,
                            partial, B, H, W, Cinp, Coutp, stream, 0, true);
}
