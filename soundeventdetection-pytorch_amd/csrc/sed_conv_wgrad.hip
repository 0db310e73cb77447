// Weight gradient of the 3x3 convolution (gfx950): the fp32 and fallback kernel conv_wgrad2_kernel, and the weight-gradient and
// fused-backward entry points with their dispatch to the faster kernels (sed_wgrad.hip, sed_wgrad_wide.hip, sed_wgrad_x3.hip,
// sed_conv_anyw.hip, sed_bwd_fused.hip).
//
// Replaces autograd's weight gradient of ConvBlock's nn.Conv2d(3x3, s1, p1, bias=False) layers, with the BatchNorm / ReLU /
// avg-pool backward that produces its dz folded in (models/spectogram_models.py:132-140,155-158 of the reference).
#include "conv_common.h"

#include <stdlib.h>
#include <algorithm>

// =================================================================================================
// weight gradient v2.
//   dW[tap][cin][cout] = sum_pix a[pix+tap][cin] * dz[pix][cout]
//   * the 9 taps are split over waves by tap ROW: wave (wt, wn) owns taps (wt, 0..2) x 32 cin x 32 cout
//     (48 accumulator registers; no cross-wave reduction, each wave stores its own slab);
//   * both operands are k(=pixel)-strided in NHWC: bf16 fragments come from ds_read_b64_tr_b16;
//   * the next tile's global loads are issued before the current tile's MFMAs (register prefetch);
//   * dz can be PRODUCED here (fused BatchNorm/ReLU/pool backward), and is then also written out by
//     the cin-tile-0 workgroups for the data-gradient kernel:
//       DZ_GIVEN : dz read as stored
//       DZ_POOL  : dz = ca*g + cb*z + cc, g = up(dy)/pool^2 * [scale*z+shift > 0]   (z = z2 of the block)
//       DZ_BN    : dz = ca*g + cb*z + cc, g stored (data-gradient epilogue output), z = z1
// =================================================================================================
template <typename T, int W, int WN, int DZ, int PRO>
__global__ __launch_bounds__(192 * WN) void conv_wgrad2_kernel(Wgrad2Params p) {
    typedef typename EL<T>::frag_t frag_t;
    constexpr int KSTEP = EL<T>::KSTEP;
    constexpr int NTHR = 192 * WN;
    constexpr int BM = 128;
    constexpr int TH = BM / W;
    constexpr int WP = (W + 2 + 3) & ~3;
    constexpr int ROWS = TH + 2;
    constexpr int XS = ROWS * WP * 32;
    constexpr int CO = 32 * WN;
    constexpr int IPP = CO / 8;                       // 8-channel items per pixel of the dz tile
    constexpr int DITEMS = BM * IPP;
    constexpr int DIT = (DITEMS + NTHR - 1) / NTHR;
    constexpr int ES = (int)sizeof(T);
    typedef HaloPlan<T, W, ROWS, WP, NTHR, 32> XPlan;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* xs = reinterpret_cast<T*>(smem);
    T* dzs = xs + XS;                                  // [WN][BM][32]
    float* coef = reinterpret_cast<float*>(dzs + WN * BM * 32);   // [5][CO]: scale, shift, ca, cb, cc

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wt = wave % 3, wn = wave / 3;
    const int r = lane & 31, hh = lane >> 5;
    const int H = p.H, Cinp = p.Cinp, Coutp = p.Coutp;
    const int NCO = Coutp / CO;
    // 1-D grid, XCD-aware: the NY = (Cinp/32)*NCO workgroups of one strip read the same dz sources (and the
    // same 128-byte lines of x), so they get consecutive logical ids = the same XCD's L2, close in time.
    const int NY = (Cinp >> 5) * NCO;
    const unsigned logical = xcd_remap(blockIdx.x, gridDim.x);
    const int strip = logical / NY, yb = logical - strip * NY;
    const int ci_tile = yb / NCO;
    const int ci0 = ci_tile * 32, co0 = (yb % NCO) * CO;
    const T* __restrict__ xg = reinterpret_cast<const T*>(p.x);
    const T* __restrict__ dg = reinterpret_cast<const T*>(p.dz);
    const T* __restrict__ zsg = reinterpret_cast<const T*>(p.zsrc);
    T* __restrict__ dzo = (ci_tile == 0) ? reinterpret_cast<T*>(p.dz_out) : nullptr;
    const int psh = p.pool >> 1;                      // pool is 1 or 2
    const int Ho = H >> psh, Wo = W >> psh;
    const float inv_pool = psh ? 0.25f : 1.0f;

    if (DZ != DZ_GIVEN) {
        for (int i = tid; i < 5 * CO; i += NTHR) {
            const int a = i / CO, c = i - a * CO;
            const float* src = (a == 0) ? p.scale : (a == 1) ? p.shift : (a == 2) ? p.ca : (a == 3) ? p.cb : p.cc;
            float v = (src != nullptr) ? src[co0 + c] : 0.f;
            if (a == 2 && DZ == DZ_POOL) v *= inv_pool;       // the 1/pool^2 of the avg-pool backward folded into ca
            coef[i] = v;
        }
    }

    f32x16 acc[3];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

    // lane-constant parts of the transpose-read addresses (bf16): the lane supplies k-row
    // 8*hh + q (+4 for the second half) and the 4 channels 16*gbit + 4*pp .. +3
    int offA[3][2], offB[2];
    {
        const int i16 = lane & 15, gbit = (lane >> 4) & 1;
        const int qq = i16 >> 2, pp = i16 & 3, ch = 16 * gbit + 4 * pp;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int kl = 8 * hh + qq + 4 * half;
            const int rq = kl / W, cq = kl % W;
#pragma unroll
            for (int tj = 0; tj < 3; ++tj)
                offA[tj][half] = ((rq + wt) * WP + cq + tj) * 32 + (ch ^ swz<bf16_t>(cq + tj));
            offB[half] = (wn * BM + kl) * 32 + ch;
        }
    }

    // ---- tile-invariant staging plans ---------------------------------------------------------------------
    XPlan xp;
    xp.init(tid, Cinp);
    unsigned dvoff[DIT], pvoff[DIT];
    int dlds[DIT], dq[DIT];
    Raw8<T> da[DIT], db[DIT];
#pragma unroll
    for (int u = 0; u < DIT; ++u) {
        const int it = tid + u * NTHR;
        const int q = it / IPP, c8 = (it - q * IPP) * 8;
        const bool ok = it < DITEMS;
        dq[u] = ok ? q : BM;                           // BM = "never valid"
        dvoff[u] = ok ? (unsigned)((q * Coutp + co0 + c8) * ES) : SED_OOB;
        pvoff[u] = ok ? (unsigned)(((((q / W) >> psh) * Wo + ((q % W) >> psh)) * Coutp + co0 + c8) * ES) : SED_OOB;
        dlds[u] = ((c8 >> 5) * BM + (ok ? q : 0)) * 32 + (c8 & 31);
    }
    const size_t ximg = (size_t)H * W * Cinp, zimg = (size_t)H * W * Coutp, pimg = (size_t)Ho * Wo * Coutp;

    auto issue = [&](int tile) {
        const int b = tile / p.tilesPerImg;
        const int h0 = (tile - b * p.tilesPerImg) * TH;
        if (SED_DBG(p, 8)) return;
        xp.issue(make_srd(xg + (size_t)b * ximg, ximg * ES), (unsigned)((((h0 - 1) * W - 1) * Cinp + ci0) * ES));
        const unsigned dt = (unsigned)(h0 * W * Coutp * ES);
        if (DZ == DZ_POOL) {
            const __amdgpu_buffer_rsrc_t gs = make_srd(dg + (size_t)b * pimg, pimg * ES);
            const __amdgpu_buffer_rsrc_t zs = make_srd(zsg + (size_t)b * zimg, zimg * ES);
            const unsigned pt = (unsigned)((h0 >> psh) * Wo * Coutp * ES);
#pragma unroll
            for (int u = 0; u < DIT; ++u) { da[u] = buf_load8<T>(gs, pvoff[u] + pt); db[u] = buf_load8<T>(zs, dvoff[u] + dt); }
        } else if (DZ == DZ_BN) {
            const __amdgpu_buffer_rsrc_t gs = make_srd(dg + (size_t)b * zimg, zimg * ES);
            const __amdgpu_buffer_rsrc_t zs = make_srd(zsg + (size_t)b * zimg, zimg * ES);
#pragma unroll
            for (int u = 0; u < DIT; ++u) { da[u] = buf_load8<T>(gs, dvoff[u] + dt); db[u] = buf_load8<T>(zs, dvoff[u] + dt); }
        } else {
            const __amdgpu_buffer_rsrc_t gs = make_srd(dg + (size_t)b * zimg, zimg * ES);
#pragma unroll
            for (int u = 0; u < DIT; ++u) da[u] = buf_load8<T>(gs, dvoff[u] + dt);
        }
    };

    auto commit = [&](int tile) {
        const int b = tile / p.tilesPerImg;
        const int h0 = (tile - b * p.tilesPerImg) * TH;
        const int row_hi = (H - h0 < ROWS - 1) ? (H - h0) : (ROWS - 1);
        xp.template commit<PRO>(xs, tid, p.pro_scale, p.pro_shift, ci0, h0 == 0 ? 1 : 0, row_hi);
        const int qmax = (H - h0) * W;                 // pixels of the tile inside the image (>= BM except on the last tile)
        const __amdgpu_buffer_rsrc_t os = make_srd(dzo ? dzo + (size_t)b * zimg : nullptr, dzo ? zimg * ES : 0);
        const unsigned dt = (unsigned)(h0 * W * Coutp * ES);
#pragma unroll
        for (int u = 0; u < DIT; ++u) {
            if (u == DIT - 1 && dq[u] >= BM) break;
            if (DZ == DZ_GIVEN) {
                lds_store_raw<T>(dzs + dlds[u], da[u]);     // rows past the image were read as zeros
            } else {
                const int c8 = (dlds[u] & 31) + 32 * (dlds[u] / (BM * 32));
                float g[8], z[8], v[8];
                raw_to_f(da[u], g);
                raw_to_f(db[u], z);
                const f32x4* cf = reinterpret_cast<const f32x4*>(coef);
#pragma unroll
                for (int e4 = 0; e4 < 2; ++e4) {
                    const int ci4 = (c8 >> 2) + e4;
                    const f32x4 a4 = cf[2 * (CO / 4) + ci4], b4 = cf[3 * (CO / 4) + ci4], c4 = cf[4 * (CO / 4) + ci4];
                    f32x4 s4, t4;
                    if (DZ == DZ_POOL) { s4 = cf[0 * (CO / 4) + ci4]; t4 = cf[1 * (CO / 4) + ci4]; }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int i = e4 * 4 + e;
                        const float base = fmaf(b4[e], z[i], c4[e]);        // cb*z + cc
                        const float full = fmaf(a4[e], g[i], base);         // + ca*g  (g is 0 where the pool floor dropped the pixel)
                        if (DZ == DZ_POOL) v[i] = (fmaf(z[i], s4[e], t4[e]) > 0.f) ? full : base;   // ReLU gate on g only
                        else v[i] = full;
                    }
                }
                if (qmax < BM && dq[u] >= qmax) {     // only the last tile of an image has rows past it
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = 0.f;
                }
                store8<T>(dzs + dlds[u], v);
                if (dzo != nullptr && !(SED_DBG(p, 1))) buf_store8<T>(os, dvoff[u] + dt, v);   // rows past the image: dropped by the range check
            }
        }
    };

    const int t_begin = strip * p.tpb;
    const int t_end = min(p.totalTiles, t_begin + p.tpb);
    if (t_begin < t_end) issue(t_begin);
    for (int tile = t_begin; tile < t_end; ++tile) {
        __syncthreads();                       // previous tile's readers are done (and coef is visible)
        commit(tile);
        __syncthreads();
        if (tile + 1 < t_end) issue(tile + 1);
        if (!(SED_DBG(p, 2)))
#pragma unroll 2
        for (int k0 = 0; k0 < BM; k0 += KSTEP) {
            frag_t bf;
            frag_t af[3];
            if constexpr (sizeof(T) == 2) {
                const int ub = ((k0 / W) * WP + (k0 % W)) * 32;
                bf = join_tr(ds_read_tr16_b64(dzs + k0 * 32 + offB[0]), ds_read_tr16_b64(dzs + k0 * 32 + offB[1]));
#pragma unroll
                for (int tj = 0; tj < 3; ++tj)
                    af[tj] = join_tr(ds_read_tr16_b64(xs + ub + offA[tj][0]), ds_read_tr16_b64(xs + ub + offA[tj][1]));
            } else {
                const int k = k0 + hh;
                bf = dzs[(wn * BM + k) * 32 + r];
#pragma unroll
                for (int tj = 0; tj < 3; ++tj) {
                    const int rr = k / W + wt, cc = k % W + tj;
                    af[tj] = xs[(rr * WP + cc) * 32 + (r ^ swz<T>(cc))];
                }
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

// =================================================================================================
// host launchers (C ABI)
// =================================================================================================

static int wgrad_strips(int B, int H, int W, int Cinp, int Coutp, int* wn_out) {
    const int wn = Coutp % 128 == 0 ? 4 : (Coutp % 64 == 0 ? 2 : 1);
    if (wn_out) *wn_out = wn;
    const int ny = (Cinp / 32) * (Coutp / (32 * wn));
    const int TH = (W >= 1 && W <= 128) ? 128 / W : 1;      // (W > 128: one row per tile)
    const long long tiles = (long long)B * cdiv(H, TH);
    long long target = (ny == 1) ? 1024 : 512;     // measured optimum (tools/bench_layer.py sweep); total workgroups
    if (const char* e = sed_getenv("SED_WGRAD_BLOCKS")) target = atoll(e) > 0 ? atoll(e) : target;   // tuning knob
    long long strips = cdiv(target, ny);
    if (strips > tiles) strips = tiles;
    if (strips < 1) strips = 1;
    return (int)strips;
}

extern "C" size_t sed_conv_wgrad_ws_floats(int B, int H, int W, int Cinp, int Coutp) {
    // one slab per workgroup of whichever kernel runs (bf16: producer/consumer, fp32: v2; the fused backward launches of
    // sed_bwd_fused.hip / sed_bwd_fused_c1.hip cut their strips differently: H + 1 rows, shorter tiles -> more slabs when B*H is small)
    int n = wgrad_strips(B, H, W, Cinp, Coutp, nullptr);
    n = std::max(n, wgrad3_strips(B, H, W, Cinp, Coutp));
    n = std::max(n, bwd_fused_max_nwg(B, H, W, Cinp, Coutp));
    if (W == 64 && Cinp == 32 && Coutp == 32) n = std::max(n, bwd_fused_c1_nwg(B, H));
    return (size_t)n * 9 * Cinp * Coutp;
}

template <typename T, int W, int WN, int DZ, int PRO>
static int launch_wgrad2(Wgrad2Params& p, hipStream_t st) {
    constexpr int TH = 128 / W;
    constexpr int WP = (W + 2 + 3) & ~3;
    constexpr size_t lds = ((size_t)(TH + 2) * WP * 32 + (size_t)WN * 128 * 32) * sizeof(T) + (size_t)5 * 32 * WN * sizeof(float);
    if (int rc_ = sed_set_max_lds<&conv_wgrad2_kernel<T, W, WN, DZ, PRO>>(lds)) return rc_;
    p.tilesPerImg = cdiv(p.H, TH);
    p.totalTiles = p.B * p.tilesPerImg;
    p.tpb = cdiv(p.totalTiles, p.strips);
    const int ny = (p.Cinp / 32) * (p.Coutp / (32 * WN));
    conv_wgrad2_kernel<T, W, WN, DZ, PRO><<<dim3(p.strips * ny), dim3(192 * WN), lds, st>>>(p);
    return 0;
}

template <typename T, int DZ>
static int dispatch_wgrad2(Wgrad2Params& p, int W, int wn, hipStream_t st) {
#define SED_CASE(WW)                                                                                          \
    case WW:                                                                                                  \
        if (p.pro == SED_PRO_BNRELU) {                                                                        \
            if (wn == 4) return launch_wgrad2<T, WW, 4, DZ, SED_PRO_BNRELU>(p, st);                           \
            if (wn == 2) return launch_wgrad2<T, WW, 2, DZ, SED_PRO_BNRELU>(p, st);                           \
            return launch_wgrad2<T, WW, 1, DZ, SED_PRO_BNRELU>(p, st);                                        \
        }                                                                                                     \
        if (wn == 4) return launch_wgrad2<T, WW, 4, DZ, SED_PRO_NONE>(p, st);                                 \
        if (wn == 2) return launch_wgrad2<T, WW, 2, DZ, SED_PRO_NONE>(p, st);                                 \
        return launch_wgrad2<T, WW, 1, DZ, SED_PRO_NONE>(p, st);
    switch (W) {
        SED_CASE(8)
        SED_CASE(16)
        SED_CASE(32)
        SED_CASE(64)
    }
#undef SED_CASE
    sed_set_error("sed_conv3x3_wgrad: W must be one of 8,16,32,64");
    return 1;
}

static int wgrad_common(int dtype, int pro, int dzmode, const void* x, const float* pro_scale, const float* pro_shift,
                        const void* dz, const void* zsrc, const float* scale, const float* shift, const float* ca,
                        const float* cb, const float* cc, int pool, void* dz_out, float* dwpack, float* workspace,
                        int B, int H, int W, int Cinp, int Coutp, hipStream_t st, float* dw = nullptr, int Cout = 0, int Cin = 0,
                        bool anyw = false) {
    SED_REQUIRE(dwpack, "the reduced gradient (dwpack) is required");
    const int dzexp = (int)(signed char)((dtype >> 8) & 0xff);      // SED_F32H3: exponent applied to dz before the fp16 split
    dtype &= 0xff;
    if (dzexp != 0 && dtype != SED_F32H3) { sed_set_error("sed_conv3x3_wgrad: an operand exponent belongs to dtype SED_F32H3"); return 1; }
    if ((double)H * W * (Cinp > Coutp ? Cinp : Coutp) * (dtype == SED_BF16 ? 2 : 4) >= 2147483648.0) {
        sed_set_error("sed_conv3x3_wgrad: one image (H*W*C elements) must stay below 2 GiB");
        return 1;
    }
    Wgrad2Params p = {};
    p.dzexp = dzexp;
    int wn;
    p.strips = wgrad_strips(B, H, W, Cinp, Coutp, &wn);
    p.x = x; p.pro_scale = pro_scale; p.pro_shift = pro_shift; p.dz = dz; p.zsrc = zsrc; p.scale = scale;
    p.shift = shift; p.ca = ca; p.cb = cb; p.cc = cc; p.dz_out = dz_out; p.ws = workspace;
    p.B = B; p.H = H; p.Cinp = Cinp; p.Coutp = Coutp; p.pro = pro; p.pool = pool < 1 ? 1 : pool;
    p.dbg = sed_dbg_env();
    int rc = 1;
    if (anyw || !sed_w_specialised(W)) {      // the width-general kernel (csrc/sed_conv_anyw.hip); p.strips: at most wgrad_strips()
        if (B <= 0 || H <= 0) { sed_set_error("sed_conv3x3_wgrad: empty input"); return 1; }
        rc = launch_wgrad_anyw(dtype, dzmode, p, W, st);
    } else if (dtype == SED_BF16) {           // producer/consumer kernel (sed_wgrad.hip) where the shape is covered
        rc = launch_wgrad3(dzmode, p, W, st);
    } else {
        rc = -1;
    }
    if (rc < 0) {
        p.strips = wgrad_strips(B, H, W, Cinp, Coutp, &wn);
#define SED_DZ(T_)                                                                         \
    (dzmode == DZ_GIVEN ? dispatch_wgrad2<T_, DZ_GIVEN>(p, W, wn, st)                      \
     : dzmode == DZ_POOL ? dispatch_wgrad2<T_, DZ_POOL>(p, W, wn, st)                      \
                         : dispatch_wgrad2<T_, DZ_BN>(p, W, wn, st))
    if (dtype == SED_BF16) rc = SED_DZ(bf16_t);
    else if (dtype == SED_F32) rc = SED_DZ(float);
    else if (dtype == SED_F32X3 || dtype == SED_F32H3) {
        rc = dtype == SED_F32H3 ? launch_wgrad_x3pc(dzmode, p, W, st) : -1;      // fp16 pieces: the producer / consumer kernel
        if (rc < 0) {
            p.strips = wgrad_strips(B, H, W, Cinp, Coutp, &wn);
            rc = launch_wgrad_x3(dtype == SED_F32H3, dzmode, p, W, wn, st);
        }
    }
    else { sed_set_error("sed_conv3x3_wgrad: bad dtype"); return 1; }
#undef SED_DZ
    }
    if (rc) return rc;
    {
        hipError_t e_ = hipGetLastError();
        if (e_ != hipSuccess) { sed_set_error(std::string("sed_conv3x3_wgrad: launch failed: ") + hipGetErrorString(e_)); return 2; }
    }
    const size_t n = (size_t)9 * Cinp * Coutp;
    reduce_wgrad_slabs(workspace, dwpack, p.strips, n, dw, Cout, Cin, Cinp, Coutp, st);
    {
        hipError_t e_ = hipGetLastError();
        if (e_ != hipSuccess) { sed_set_error(std::string("sed_conv3x3_wgrad: reduce launch failed: ") + hipGetErrorString(e_)); return 2; }
    }
    return 0;
}

extern "C" int sed_conv3x3_wgrad(int dtype, int pro, const void* x, const float* pro_scale, const float* pro_shift,
                                 const void* dz, float* dwpack, float* workspace, int B, int H, int W, int Cinp,
                                 int Coutp, void* stream) {
    SED_REQUIRE(Cinp % 32 == 0 && Coutp % 32 == 0, "channels must be padded to 32");
    SED_REQUIRE(pro == SED_PRO_NONE || (pro_scale && pro_shift), "prologue operands");
    return wgrad_common(dtype, pro, DZ_GIVEN, x, pro_scale, pro_shift, dz, nullptr, nullptr, nullptr, nullptr, nullptr,
                        nullptr, 1, nullptr, dwpack, workspace, B, H, W, Cinp, Coutp, (hipStream_t)stream);
}

extern "C" int sed_conv3x3_wgrad_anyw(int dtype, int pro, const void* x, const float* pro_scale, const float* pro_shift,
                                      const void* dz, float* dwpack, float* workspace, int B, int H, int W, int Cinp,
                                      int Coutp, void* stream) {
    SED_REQUIRE(Cinp % 32 == 0 && Coutp % 32 == 0, "channels must be padded to 32");
    SED_REQUIRE(pro == SED_PRO_NONE || (pro_scale && pro_shift), "prologue operands");
    return wgrad_common(dtype, pro, DZ_GIVEN, x, pro_scale, pro_shift, dz, nullptr, nullptr, nullptr, nullptr, nullptr,
                        nullptr, 1, nullptr, dwpack, workspace, B, H, W, Cinp, Coutp, (hipStream_t)stream, nullptr, 0, 0, true);
}

extern "C" int sed_conv3x3_wgrad_u(int dtype, int pro, const void* x, const float* pro_scale, const float* pro_shift, const void* dz,
                                   float* dwpack, float* workspace, int B, int H, int W, int Cinp, int Coutp, float* dw, int Cout,
                                   int Cin, void* stream) {
    SED_REQUIRE(Cinp % 32 == 0 && Coutp % 32 == 0, "channels must be padded to 32");
    SED_REQUIRE(pro == SED_PRO_NONE || (pro_scale && pro_shift), "prologue operands");
    SED_REQUIRE(dw && Cout > 0 && Cin > 0 && Cout <= Coutp && Cin <= Cinp, "unpacked gradient operands");
    return wgrad_common(dtype, pro, DZ_GIVEN, x, pro_scale, pro_shift, dz, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1,
                        nullptr, dwpack, workspace, B, H, W, Cinp, Coutp, (hipStream_t)stream, dw, Cout, Cin);
}

extern "C" int sed_conv3x3_wgrad_fused(int dtype, int pro, const void* x, const float* pro_scale,
                                       const float* pro_shift, int dzmode, const void* gsrc, const void* zsrc,
                                       const float* scale, const float* shift, const float* ca, const float* cb,
                                       const float* cc, int pool, void* dz_out, float* dwpack, float* workspace, int B,
                                       int H, int W, int Cinp, int Coutp, void* stream) {
    SED_REQUIRE(Cinp % 32 == 0 && Coutp % 32 == 0, "channels must be padded to 32");
    SED_REQUIRE(pro == SED_PRO_NONE || (pro_scale && pro_shift), "prologue operands");
    SED_REQUIRE(dzmode == SED_DZ_POOL || dzmode == SED_DZ_BN, "dzmode must be SED_DZ_POOL or SED_DZ_BN");
    SED_REQUIRE(gsrc && zsrc && ca && cb && cc, "fused dz operands");
    SED_REQUIRE(dzmode != SED_DZ_POOL || (scale && shift && (pool == 1 || pool == 2)), "pool-backward operands");
    return wgrad_common(dtype, pro, dzmode, x, pro_scale, pro_shift, gsrc, zsrc, scale, shift, ca, cb, cc, pool, dz_out,
                        dwpack, workspace, B, H, W, Cinp, Coutp, (hipStream_t)stream);
}

extern "C" int sed_conv3x3_wgrad_fused_u(int dtype, int pro, const void* x, const float* pro_scale, const float* pro_shift,
                                         int dzmode, const void* gsrc, const void* zsrc, const float* scale, const float* shift,
                                         const float* ca, const float* cb, const float* cc, int pool, void* dz_out, float* dwpack,
                                         float* workspace, int B, int H, int W, int Cinp, int Coutp, float* dw, int Cout, int Cin,
                                         void* stream) {
    SED_REQUIRE(Cinp % 32 == 0 && Coutp % 32 == 0, "channels must be padded to 32");
    SED_REQUIRE(pro == SED_PRO_NONE || (pro_scale && pro_shift), "prologue operands");
    SED_REQUIRE(dzmode == SED_DZ_POOL || dzmode == SED_DZ_BN, "dzmode must be SED_DZ_POOL or SED_DZ_BN");
    SED_REQUIRE(gsrc && zsrc && ca && cb && cc, "fused dz operands");
    SED_REQUIRE(dzmode != SED_DZ_POOL || (scale && shift && (pool == 1 || pool == 2)), "pool-backward operands");
    SED_REQUIRE(dw && Cout > 0 && Cin > 0 && Cout <= Coutp && Cin <= Cinp, "unpacked gradient operands");
    return wgrad_common(dtype, pro, dzmode, x, pro_scale, pro_shift, gsrc, zsrc, scale, shift, ca, cb, cc, pool, dz_out,
                        dwpack, workspace, B, H, W, Cinp, Coutp, (hipStream_t)stream, dw, Cout, Cin);
}

extern "C" int sed_conv3x3_bwd_fused_supported_pool(int dtype, int W, int Cinp, int Coutp, int dzmode, int pro, int epi, int pool) {
    if (dtype != SED_BF16) return 0;
    if (W == 32) return (dzmode != SED_DZ_POOL || pool == 2) && bwd_fused_nwg(1, 64, W, Cinp, Coutp, dzmode, pro, epi) > 0;
#ifdef SED_EXPERIMENTS
    return bwd_fused_cs_nstrips(1, 64, W, Cinp, Coutp, dzmode, pro, epi, pool) > 0;
#else
    return 0;
#endif
}
extern "C" int sed_conv3x3_bwd_fused_supported(int dtype, int W, int Cinp, int Coutp, int dzmode, int pro, int epi) {
    return sed_conv3x3_bwd_fused_supported_pool(dtype, W, Cinp, Coutp, dzmode, pro, epi, 2);
}

extern "C" int sed_conv3x3_bwd_fused(int dtype, int pro, const void* x, const float* pro_scale, const float* pro_shift, int dzmode,
                                     const void* gsrc, const void* zsrc, const float* scale, const float* shift, const float* ca,
                                     const float* cb, const float* cc, int pool, const void* wpack_t, void* dx, int epi,
                                     const void* zref, const void* cnt, const float* epi_scale, const float* epi_shift,
                                     const float* epi_mean, const float* epi_invstd, float* partial, int nparts, int* flag,
                                     float* dwpack, float* workspace, int B, int H, int W, int Cinp, int Coutp, float* dw, int Cout,
                                     int Cin, void* stream) {
    SED_REQUIRE(sed_conv3x3_bwd_fused_supported_pool(dtype, W, Cinp, Coutp, dzmode, pro, epi, dzmode == SED_DZ_POOL ? pool : 2),
                "covered: bf16; W = 32: 32 -> 64 (DZ_BN, no prologue, STORE / POOLSTATS) or 64 -> 64 (DZ_POOL pool 2, BN+ReLU prologue, "
                "RELUBWD); W = 16 / 8: 64 / 128 -> 128 in the same two forms (DZ_POOL with pool 1 or 2)");
    SED_REQUIRE(B > 0 && H > 0 && x && gsrc && zsrc && ca && cb && cc && wpack_t && dx && dwpack && workspace, "operands");
    SED_REQUIRE(pro == SED_PRO_NONE || (pro_scale && pro_shift), "prologue operands");
    SED_REQUIRE(dzmode != SED_DZ_POOL || (scale && shift && (pool == 1 || pool == 2)), "pool-backward operands");
    SED_REQUIRE(epi == SED_EPI_STORE || (zref && epi_scale && epi_shift && epi_mean && epi_invstd && partial && nparts > 0), "epilogue operands");
    SED_REQUIRE(epi != SED_EPI_POOLSTATS || (cnt && flag), "pooled-tensor statistics operands");
    // both covered layers have zref == x (conv2: the ReLU / BN1 reference is the z tensor its prologue reads; conv1: the pooled
    // activation is the convolution's input): the kernel takes the reference from the tile it already holds
    SED_REQUIRE(epi == SED_EPI_STORE || zref == x, "the epilogue reference must be the convolution's input tensor");
    SED_REQUIRE(epi != SED_EPI_RELUBWD || (epi_scale == pro_scale && epi_shift == pro_shift),
                "the ReLU decision of conv2's data gradient uses the prologue's BatchNorm coefficients (same block, BN1)");
    SED_REQUIRE(dw == nullptr || (Cout > 0 && Cin > 0 && Cout <= Coutp && Cin <= Cinp), "unpacked gradient operands");
    SED_REQUIRE((double)H * W * (Cinp > Coutp ? Cinp : Coutp) * 2 < 2147483648.0, "one image (H*W*C elements) must stay below 2 GiB");
    BwdFusedParams p = {};
    p.x = x; p.pro_scale = pro_scale; p.pro_shift = pro_shift; p.gsrc = gsrc; p.zsrc = zsrc; p.scale = scale; p.shift = shift;
    p.ca = ca; p.cb = cb; p.cc = cc; p.wpack_t = wpack_t; p.dx = dx; p.zref = zref; p.cnt = reinterpret_cast<const unsigned char*>(cnt);
    p.epi_scale = epi_scale; p.epi_shift = epi_shift; p.epi_mean = epi_mean; p.epi_invstd = epi_invstd; p.partial = partial;
    p.flag = flag; p.ws = workspace; p.B = B; p.H = H; p.Cinp = Cinp; p.Coutp = Coutp; p.pool = dzmode == SED_DZ_POOL ? pool : 1;
    p.dzmode = dzmode; p.pro = pro; p.epi = epi; p.nparts = nparts;
    const int rc = launch_bwd_fused(p, W, (hipStream_t)stream);
    SED_REQUIRE(rc >= 0, "shape not covered");
    if (rc) return rc;
    SED_LAUNCH_CHECK();
    const size_t n = (size_t)9 * Cinp * Coutp;
    reduce_wgrad_slabs(workspace, dwpack, p.nwg, n, dw, Cout, Cin, Cinp, Coutp, (hipStream_t)stream);
    SED_LAUNCH_CHECK();
    return 0;
}
