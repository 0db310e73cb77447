/*
 * sed_hip.h -- C ABI of libsed_hip.so: the MI355X (gfx950) kernels of the sound-event-detection
 * training hot path.
 *
 * The reference (ariel415el/SoundEventDetection-Pytorch) has no FFI: its hot path is Python calling
 * torch/ATen/librosa.  Each entry point below therefore names the reference *Python* call it
 * replaces (file:line under the reference root); the host-side mirror of the reference API
 * (soundeventdetection-pytorch_amd/) binds these with ctypes -- see INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless named h_*;
 *   - no ownership transfer: every buffer (workspaces included) is allocated by the caller;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises,
 *     so every call is hipGraph-capturable;
 *   - return value 0 = ok, non-zero = error (sed_last_error() gives the text; the Python side
 *     raises RuntimeError);
 *   - activations are NHWC = [B][H = time frames][W = mel bins][C], C padded to a multiple of 32
 *     (padded channels are exactly 0), element type `dtype` (SED_F32 or SED_BF16); statistics,
 *     parameters, gradients and optimizer state are always fp32;
 *   - "wpack" is a conv weight re-laid for the MFMA A-operand by sed_pack_conv_weight().
 */
#ifndef SED_HIP_H
#define SED_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SED_ABI_VERSION 1

/* SED_F32X3 / SED_F32H3 (round 6, "bf16x3" / "f16x3"): fp32 tensors in memory like SED_F32, but the GEMM-shaped kernels
 * (sed_conv3x3_fwd, sed_conv3x3_wgrad*, with operators packed by sed_pack_conv_weight(s_batch) under the same dtype: two 16-bit
 * images, hi then lo, in the wpack buffer of 9*Cinp*Coutp fp32 words) split every operand a = hi + lo/LS and run three 16-bit MFMAs
 * per product with fp32 accumulation (csrc/sed_conv_x3.hip).  X3: bf16 pieces, LS = 1, ~1e-5 relative per product.  H3: fp16 pieces,
 * LS = 2^11, ~5e-7 per product; because fp16 has five exponent bits, a call whose streamed operand is a GRADIENT (the data gradient's
 * x = dz, the weight gradient's dz) carries a signed power-of-two exponent e in bits 8..15 of the dtype argument
 * (dtype = SED_F32H3 | ((e & 0xff) << 8)): the operand is multiplied by 2^e before the split (and clamped to +-60000), the result by
 * 2^-e; e = round(log2(B*H*W)) + 2 (engine.CnnEngine._grad_dtype) brings a per-pixel loss gradient ~1/(B*H*W) to ~4, and the f16x3
 * gate holds for true gradient scales 2^(-e-12) .. 2^(-e+12) (tests/test_gpu_conv_exact_oracle.py).  Every other entry point takes
 * SED_F32 for such tensors.                                                                                                         */
enum { SED_F32 = 0, SED_BF16 = 1, SED_F32X3 = 2, SED_F32H3 = 3 };

/* prologue applied to the conv input while it is staged into LDS */
enum {
    SED_PRO_NONE = 0,   /* x as stored                                                          */
    SED_PRO_BNRELU = 1  /* relu(scale[c]*x + shift[c]): F.relu_(bn(.)) spectogram_models.py:155  */
};
/* epilogue applied to the conv accumulator */
enum {
    SED_EPI_STORE = 0,    /* store only                                                         */
    SED_EPI_STATS = 1,    /* store + per-channel sum / sum-of-squares partials (BatchNorm stats) */
    SED_EPI_RELUBWD = 2,  /* g = acc * (scale[c]*zref+shift[c] > 0); store g; partials of
                             sum(g), sum(g*xhat), xhat = (zref-mean[c])*invstd[c]               */
    SED_EPI_POOLSTATS = 4 /* sed_conv3x3_bwd_fused only: store + the pooled-tensor statistics of
                             sed_conv3x3_dgrad_poolstats (zref = pooled activation, cnt)         */
};

int sed_abi_version(void);
const char* sed_last_error(void);
/* SED_* tuning / A-B knobs are read from the environment once per name and cached inside the library; this drops the
 * cache (test hook: lets one process flip a knob between two calls).  No reference counterpart.                      */
void sed_config_reload(void);
/* build flags of this library: bit 0 = EXPERIMENTS (opt-in resident-weight kernels, SED_CONV_KERNEL=r/4, extra loader-wave
 * variants), bit 1 = DEBUG_SWITCHES (SED_DBG run-time ablation switches), bit 2 = STAMPS.  The product build returns 0. */
int sed_build_flags(void);
/* number of compute units of the current device (grid sizing on the host side) */
int sed_device_cu_count(void);

/* ---- weights ------------------------------------------------------------------------------
 * torch layout W[Cout][Cin][3][3] fp32 (nn.Conv2d weight, spectogram_models.py:132-140) ->
 * wpack[Cinp/32][9][32/KR][Coutp][KR], KR = 8 (bf16) or 1 (f32), zero padded to Cinp/Coutp.
 * transpose_flip != 0 packs the data-gradient operator W'[c][o][i][j] = W[o][c][2-i][2-j]
 * (then the packed "Cin" is the conv's Cout and vice versa).                                  */
int sed_pack_conv_weight(int dtype, const float* w, void* wpack, int Cout, int Cin, int Coutp,
                         int Cinp, int transpose_flip, void* stream);
/* inverse for gradients: dwpack fp32 [9][Cinp][Coutp] -> dW[Cout][Cin][3][3] fp32              */
int sed_unpack_conv_wgrad(const float* dwpack, float* dw, int Cout, int Cin, int Coutp, int Cinp,
                          void* stream);

/* ---- conv 3x3 s1 p1, no bias (nn.Conv2d forward, spectogram_models.py:155-156) -------------
 * First layer, Cin = 1: x fp32 [B][H][W] (optionally z-scored on load with mean/std[W],
 * SpectogramDataset.transform spectograms_dataset.py:104-108; pass NULL to skip), w fp32
 * [Cout][1][3][3] torch layout, z [B][H][W][Coutp].  stats_partial fp32 [nparts][2][Coutp]
 * receives per-workgroup (sum, sumsq); *nparts is fixed by sed_conv_c1_nparts().               */
int sed_conv_c1_nparts(int B, int H, int W);
int sed_conv3x3_c1_fwd(int dtype, const float* x, const float* mean, const float* std,
                       const float* w, void* z, float* stats_partial, int B, int H, int W,
                       int Cout, int Coutp, void* stream);
/* dW[Cout][1][3][3] for the first layer: dz [B][H][W][Coutp]; dw_partial fp32 [nparts][9][Coutp] */
int sed_conv3x3_c1_wgrad(int dtype, const float* x, const float* mean, const float* std,
                         const void* dz, float* dw_partial, int B, int H, int W, int Coutp,
                         void* stream);

/* Same with the layer's dz produced on load: dz = ca*g + cb*zsrc + cc (BatchNorm backward of the first
 * layer folded in; g = data-gradient epilogue output, zsrc = the layer's pre-BN output).  Block 0 has
 * no data gradient, so its dz never has to be written to memory.                                */
int sed_conv3x3_c1_wgrad_fused(int dtype, const float* x, const float* mean, const float* std,
                               const void* g, const void* zsrc, const float* ca, const float* cb,
                               const float* cc, float* dw_partial, int B, int H, int W, int Coutp,
                               void* stream);

/* Line widths.  The generic layer calls below (sed_conv3x3_fwd, sed_conv3x3_wgrad[_u], sed_conv3x3_wgrad_fused[_u]) take any
 * width 1 <= W <= SED_ANYW_MAX_W.  W in {8, 16, 32, 64} runs the specialised kernels (every dtype); any other W runs the
 * width-general kernels (sed_conv3x3_fwd_anyw / sed_conv3x3_wgrad_anyw below), which cover SED_BF16 and SED_F32 only: SED_F32X3 /
 * SED_F32H3 there return an error.  The fused weight-gradient forms need dz_out at those widths (dz is produced by
 * sed_pool_relu_bn_bwd_apply / sed_bn_bwd_apply into dz_out, then read back).  Every *_supported query answers 0 outside
 * {8, 16, 32, 64}.                                                                                                        */
#define SED_ANYW_MAX_W 256

/* Generic layer (Cinp, Coutp multiples of 32; W as above): implicit GEMM on MFMA.
 * Serves forward (wpack of W) and data-gradient (wpack of W', transpose_flip).
 *   x [B][H][W][Cinp]; pro_scale/pro_shift fp32 [Cinp] (SED_PRO_BNRELU);
 *   z [B][H][W][Coutp];
 *   SED_EPI_STATS: partial fp32 [nparts][2][Coutp] = (sum z, sum z^2) from the fp32 accumulator;
 *   SED_EPI_RELUBWD: zref [B][H][W][Coutp], epi_scale/epi_shift/epi_mean/epi_invstd fp32 [Coutp];
 *                    partial = (sum g, sum g*xhat).
 * nparts = sed_conv_nparts(B, H, W).                                                           */
int sed_conv_nparts(int B, int H, int W);
int sed_conv3x3_fwd(int dtype, int pro, int epi, const void* x, const float* pro_scale,
                    const float* pro_shift, const void* wpack, void* z, const void* zref,
                    const float* epi_scale, const float* epi_shift, const float* epi_mean,
                    const float* epi_invstd, float* partial, int B, int H, int W, int Cinp,
                    int Coutp, void* stream);

/* The same call when the 3x3 weights have ZERO SIDE COLUMNS (taps 0,2,3,5,6,8): a k = 3 Conv1d over frames interleaved on
 * the W axis (the M5 layout, sed_m5_*).  The producer/consumer kernel then contracts taps 1, 4, 7 only (W = 8, bf16); every
 * other path computes all nine taps -- same result.                                                                */
int sed_conv3x3_fwd_col(int dtype, int pro, int epi, const void* x, const float* pro_scale,
                        const float* pro_shift, const void* wpack, void* z, const void* zref,
                        const float* epi_scale, const float* epi_shift, const float* epi_mean,
                        const float* epi_invstd, float* partial, int B, int H, int W, int Cinp,
                        int Coutp, void* stream);

/* Weight gradient of the generic layer: dwpack fp32 [9][Cinp][Coutp] (overwritten) =
 * sum_{b,h,w} a[b][h+i-1][w+j-1][c] * dz[b][h][w][o], a = pro(x).  workspace fp32 of
 * sed_conv_wgrad_ws_floats() floats.                                                          */
size_t sed_conv_wgrad_ws_floats(int B, int H, int W, int Cinp, int Coutp);
int sed_conv3x3_wgrad(int dtype, int pro, const void* x, const float* pro_scale,
                      const float* pro_shift, const void* dz, float* dwpack, float* workspace,
                      int B, int H, int W, int Cinp, int Coutp, void* stream);

/* The width-general kernels called directly, at any 1 <= W <= SED_ANYW_MAX_W (the specialised widths included; SED_BF16 /
 * SED_F32): same arguments and results as sed_conv3x3_fwd (every prologue x epilogue pair) and sed_conv3x3_wgrad.  The
 * workspace of sed_conv_wgrad_ws_floats() suffices; nparts = sed_conv_nparts(B, H, W).                                   */
int sed_conv3x3_fwd_anyw(int dtype, int pro, int epi, const void* x, const float* pro_scale,
                         const float* pro_shift, const void* wpack, void* z, const void* zref,
                         const float* epi_scale, const float* epi_shift, const float* epi_mean,
                         const float* epi_invstd, float* partial, int B, int H, int W, int Cinp,
                         int Coutp, void* stream);
int sed_conv3x3_wgrad_anyw(int dtype, int pro, const void* x, const float* pro_scale,
                           const float* pro_shift, const void* dz, float* dwpack, float* workspace,
                           int B, int H, int W, int Cinp, int Coutp, void* stream);

/* Same weight gradient with the layer's dz PRODUCED on load (fused BatchNorm/ReLU/avg-pool backward,
 * i.e. the autograd nodes between two convolutions of ConvBlock.forward, spectogram_models.py:155-158):
 *   SED_DZ_POOL: dz = ca*g + cb*z + cc with g = up(gsrc)/pool^2 * [scale*z + shift > 0];
 *                gsrc = gradient w.r.t. the pooled block output [B][H/pool][W/pool][Coutp], zsrc = z2
 *   SED_DZ_BN  : dz = ca*gsrc + cb*zsrc + cc; gsrc = data-gradient epilogue output g, zsrc = z1
 * (ca, cb, cc from sed_bn_bwd_finalize).  If dz_out != NULL the produced dz [B][H][W][Coutp] is
 * also written there (consumed by the data-gradient call); it must not alias gsrc/zsrc.           */
enum { SED_DZ_POOL = 1, SED_DZ_BN = 2 };
int sed_conv3x3_wgrad_fused(int dtype, int pro, const void* x, const float* pro_scale,
                            const float* pro_shift, int dzmode, const void* gsrc, const void* zsrc,
                            const float* scale, const float* shift, const float* ca, const float* cb,
                            const float* cc, int pool, void* dz_out, float* dwpack, float* workspace,
                            int B, int H, int W, int Cinp, int Coutp, void* stream);

/* ---- BatchNorm2d (spectogram_models.py:142-143,155-156; eps 1e-5, momentum 0.1) ------------
 * Training statistics from the conv epilogue partials [nparts][2][Cp]: batch mean, biased var ->
 * scale = gamma*invstd, shift = beta - mean*scale, saved mean/invstd, and the running-stat
 * update (unbiased var, n/(n-1)).  gamma/beta/running_* have C (unpadded) entries; outputs Cp
 * entries with padded channels [C, Cp) forced to scale = shift = mean = invstd = 0 (the partials'
 * padded columns are not used).  count = B*H*W; count = 1 keeps the biased variance.  The sums
 * over nparts and var = q/n - mean^2 (clamped at 0) are formed in fp64.  running_* may both be
 * NULL (no update).                                                                            */
int sed_bn_train_finalize(const float* partial, int nparts, double count, const float* gamma,
                          const float* beta, float* running_mean, float* running_var,
                          float momentum, float eps, float* scale, float* shift, float* mean,
                          float* invstd, int C, int Cp, void* stream);
/* Eval mode: scale/shift from the running statistics (padded channels [C, Cp) = 0).            */
int sed_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* scale, float* shift, int C,
                       int Cp, void* stream);
/* Backward reduction finalize: partial [nparts][2][Cp] = (sum g, sum g*xhat) ->
 * dgamma[C], dbeta[C] and the coefficients of dz = ca*g + cb*z + cc (fp32 [Cp] each):
 *   ca = gamma*invstd, cb = -gamma*invstd^2*mgx, cc = -gamma*invstd*(mg - mean*invstd*mgx),
 * mg = sum g / count, mgx = sum g*xhat / count.  ca/cb/cc are 0 on the padded channels [C, Cp);
 * the padded entries of partial, mean and invstd are not used.                                 */
int sed_bn_bwd_finalize(const float* partial, int nparts, double count, const float* gamma,
                        const float* mean, const float* invstd, float* dgamma, float* dbeta,
                        float* ca, float* cb, float* cc, int C, int Cp, void* stream);

/* ---- fused elementwise stages --------------------------------------------------------------
 * y = avg_pool2d(relu(scale*z+shift), pool) (spectogram_models.py:156-158), pool in {1,2};
 * z [B][H][W][Cp] -> y [B][H/pool][W/pool][Cp] (floor: a trailing odd row / column is dropped and
 * never read).  relu'(0) = 0: a pixel with scale*z+shift == 0 is inactive, here and in the backward.
 * All Cp channels are treated alike: padded channels stay 0 through scale = shift = 0.             */
int sed_bn_relu_pool_fwd(int dtype, const void* z, const float* scale, const float* shift, void* y,
                         int B, int H, int W, int Cp, int pool, void* stream);
/* backward, pass 1: g = up(dy)/pool^2 * (scale*z+shift > 0); partial [nparts][2][Cp] =
 * (sum g, sum g*xhat); nparts = sed_pool_bwd_nparts().  dy [B][H/pool][W/pool][Cp].           */
int sed_pool_bwd_nparts(int B, int H, int W, int Cp);
int sed_pool_relu_bwd_stats(int dtype, const void* dy, const void* z, const float* scale,
                            const float* shift, const float* mean, const float* invstd,
                            float* partial, int B, int H, int W, int Cp, int pool, void* stream);
/* The same statistics WITHOUT reading z (pool = 2, bf16): per pooled pixel P the forward also stores
 * cnt(P) = number of its four pixels with scale*z+shift > 0 (uint8 [B][H/2][W/2][Cp]); then
 *   sum g      = sum_P dy(P) * cnt(P) / 4
 *   sum g*xhat = sum_P dy(P) * (y(P) - beta*cnt(P)/4) / gamma      (y = the pooled activation the forward stored,
 *                                                                   gamma*xhat + beta = scale*z + shift)
 * are functions of pooled tensors only, and the data-gradient kernel that PRODUCES dy accumulates them in its epilogue
 * (sed_conv3x3_dgrad_poolstats: no separate pass, no second read of the full-resolution z).  A channel with gamma = 0
 * cannot be recovered that way (0/0): the kernel then raises *flag and sed_pool_relu_bwd_stats_if recomputes the
 * partials from z (it returns at once while *flag is 0).  partial [nparts][2][Cp], nparts >= sed_conv_nparts(B, H, W) of
 * the data-gradient launch; the conditional pass uses min(nparts, its own row count) workgroups and zero-fills the rest.  */
int sed_bn_relu_pool_cnt_fwd(int dtype, const void* z, const float* scale, const float* shift, void* y,
                             void* cnt, int B, int H, int W, int Cp, void* stream);
int sed_dgrad_poolstats_supported(int dtype, int W, int Cinp, int Coutp);
int sed_conv3x3_dgrad_poolstats(int dtype, const void* dz, const void* wpack_t, void* dy, const void* y_pooled,
                                const void* cnt, const float* scale, const float* shift, const float* mean,
                                const float* invstd, float* partial, int nparts, int* flag, int B, int H, int W,
                                int Cinp, int Coutp, void* stream);
int sed_pool_relu_bwd_stats_if(const int* flag, int dtype, const void* dy, const void* z, const float* scale,
                               const float* shift, const float* mean, const float* invstd, float* partial,
                               int nparts, int B, int H, int W, int Cp, int pool, void* stream);
/* backward, pass 2: dz = ca*g + cb*z + cc with g recomputed as in pass 1, on all H x W pixels:
 * g = 0 on the row / column the pooling floor dropped (dz = cb*z + cc there); pass 1 skips them.  */
int sed_pool_relu_bn_bwd_apply(int dtype, const void* dy, const void* z, const float* scale,
                               const float* shift, const float* ca, const float* cb,
                               const float* cc, void* dz, int B, int H, int W, int Cp, int pool,
                               void* stream);
/* dz = ca*g + cb*z + cc for a materialised g (data-gradient epilogue output); in place allowed. */
int sed_bn_bwd_apply(int dtype, const void* g, const void* z, const float* ca, const float* cb,
                     const float* cc, void* dz, size_t npix, int Cp, void* stream);

/* ---- head + loss ---------------------------------------------------------------------------
 * Cnn_AvgPooling.forward tail (spectogram_models.py:193-200): mean over mel (W) -> Linear(C,K)
 * -> raw logits; the x`ratio` interpolate() is NOT materialised here: pre [B][t][K] fp32.
 * feat [B][t][Wf][Cp] (post BN/ReLU/pool activations); fc_w [K][C], fc_b [K] fp32;
 * m_out [B][t][Cp] fp32 keeps the mel-mean for the backward pass; its padded channels [C, Cp) are
 * the mean of feat's padded channels (0 for a well-formed activation) and pre does not depend on
 * them.                                                                                        */
int sed_head_fwd(int dtype, const void* feat, const float* fc_w, const float* fc_b, float* m_out,
                 float* pre, int B, int t, int Wf, int C, int Cp, int K, void* stream);
/* interpolate(): out[b][i][k] = pre[b][i/ratio][k] (spectogram_models.py:9-22)                 */
int sed_interpolate(const float* pre, float* out, int B, int t, int K, int ratio, void* stream);
/* WeightedBCE.__call__ (utils/common.py:16-30) on the interpolated logits without materialising
 * them: N = min(t*ratio, Tt) frames; loss[0] = mean over B*N*K of
 * -(w*y*logsigmoid(x) + (1-y)*logsigmoid(-x)); dpre [B][t][K] = d loss / d pre (the x`ratio`
 * repeat backward already summed). target [B][Tt][K] fp32. loss_partial: fp32 scratch of at
 * least ceil(B*t*K/256) floats. dpre may be NULL (loss only).  dpre is formed as (sum / numel) *
 * grad_scale in that order: a gradient whose unscaled value is subnormal (logits below about -87)
 * is rounded to a multiple of 2^-149 before grad_scale multiplies it.                           */
int sed_bce_fwd_bwd(const float* pre, const float* target, float* loss, float* dpre,
                    float* loss_partial, int B, int t, int K, int ratio, int Tt, float recall_factor,
                    float grad_scale, void* stream);
/* ---- weak-label (clip-level) loss: csrc/sed_weak.hip ------------------------------------------
 * The frame probabilities of a clip are pooled over time into one clip probability per class and
 * WeightedBCE is taken against the clip label, on pre [B][t][K] fp32 like sed_bce_fwd_bwd (the
 * x`ratio` interpolate() is not materialised): with N = min(t*ratio, Tt) virtual frames, row i of
 * pre stands for c_i = clamp(N - i*ratio, 0, ratio) frames; rows with c_i = 0 take no part (not in
 * the max either) and get gradient exactly 0.  For one (b, k), x_i the logit, all in double:
 *   p_i = 1/(1+exp(-x_i)), q_i = 1/(1+exp(x_i));  P the clip probability, Q = 1 - P from its own sums
 *   SED_POOL_MAX     P = p_j, Q = q_j, j the smallest index of the largest x_i;   dP/dp_i = [i == j]
 *   SED_POOL_MEAN    P = sum c_i p_i / N, Q = sum c_i q_i / N;                     dP/dp_i = c_i / N
 *   SED_POOL_LINEAR  P = S2/S1, S1 = sum c_i p_i, S2 = sum c_i p_i^2, Q = sum c_i p_i q_i / S1;
 *                    dP/dp_i = c_i (2 p_i - P) / S1   (S1 == 0: P = 0, Q = 1, gradient 0)
 *   SED_POOL_EXP     P = sum c_i p_i e^{p_i} / E, E = sum c_i e^{p_i}, Q = sum c_i q_i e^{p_i} / E;
 *                    dP/dp_i = c_i e^{p_i} (1 + p_i - P) / E
 *   l = -(w Y max(ln P, -100) + (1 - Y) max(ln Q, -100)), loss = weight * mean over B*K of l,
 *   dl/dP = -w Y / max(P, 1e-12) + (1 - Y) / max(Q, 1e-12),
 *   dpre_i = weight * grad_scale / (B*K) * dl/dP * dP/dp_i * p_i q_i, rounded once to fp32.
 * Every sum is taken in a fixed order without atomics (the same bits on every run); there is no
 * host synchronisation, so the calls can be captured in a HIP graph.                             */
#define SED_POOL_MAX 0
#define SED_POOL_MEAN 1
#define SED_POOL_LINEAR 2
#define SED_POOL_EXP 3
/* clip_prob [B][K] = P only (inference); one launch.                                             */
int sed_clip_pool_fwd(const float* pre, float* clip_prob, int B, int t, int K, int ratio, int Tt,
                      int mode, void* stream);
/* target_frames == 0: target is the clip labels [B][K] and Tt only sets N.  target_frames == Tt:
 * target is the strong [B][Tt][K] tensor and Y is the maximum over its first N frames, taken by the
 * kernel.  Y may be soft.  clip_prob [B][K] and dpre [B][t][K] may be NULL.  accumulate = 1 adds to
 * loss[0] and to dpre (one fp32 add per element) instead of overwriting them: the strong loss runs
 * first and the weak one lands on top.  workspace: sed_weak_bce_ws_bytes() bytes, 8-byte aligned.
 * Two launches.                                                                                  */
size_t sed_weak_bce_ws_bytes(int B, int t, int K);
int sed_weak_bce_fwd_bwd(const float* pre, const float* target, int target_frames, float* clip_prob,
                         float* loss, float* dpre, int accumulate, int B, int t, int K, int ratio,
                         int Tt, int mode, float recall_factor, float weight, float grad_scale,
                         void* workspace, void* stream);
/* ---- semi-supervised training: csrc/sed_semi.hip, csrc/sed_weak.hip ---------------------------
 * Batches that mix strongly labelled, weakly labelled and unlabelled clips, and a mean teacher (an
 * exponential moving average of the student's weights whose frame and clip probabilities the student
 * is pulled towards).  The three losses work on pre [B][t][K] fp32 like sed_bce_fwd_bwd: N =
 * min(t*ratio, Tt) virtual frames, row i stands for the frames [i*ratio, i*ratio + c_i), c_i =
 * clamp(N - i*ratio, 0, ratio).  clip_sel [B] is a byte per clip, nonzero = the clip takes part; NULL =
 * all clips.  S, the number of selected clips, is counted on the device (no host synchronisation).
 * All arithmetic is double, p = 1/(1+exp(-x)) and q = 1/(1+exp(x)) each from its own expression;
 * every result is rounded once to fp32; every sum is taken in a fixed order without atomics (the same
 * bits on every run).  accumulate = 0 overwrites loss[0] and dpre; accumulate = 1 adds to them, one
 * IEEE fp32 add per element.  Cells of unselected clips and of rows with c_i = 0 are written as exact
 * 0 under accumulate = 0 and are not touched under accumulate = 1.  S == 0: the loss term is exactly
 * 0 and so is the gradient.  dpre may be NULL (loss only).  Two launches each.
 *
 * sed_bce_sel_fwd_bwd: WeightedBCE over the selected clips.  target [B][Tt][K] fp32.
 *   l_f = -(w y_f ln sigma(x) + (1 - y_f) ln sigma(-x)), ln sigma(x) = min(x, 0) - log1p(exp(-|x|))
 *   (no -100 clamp, as in sed_bce_fwd_bwd);  loss = weight * sum_{b in sel} sum_{f<N} sum_k l_f / (S N K)
 *   dpre[b][i][k] = weight * grad_scale / (S N K) * sum_{f of row i, f<N} ((1 - y_f) p - w y_f q)
 * workspace: sed_bce_sel_ws_bytes() bytes, 8-byte aligned.                                        */
size_t sed_bce_sel_ws_bytes(int B, int t, int K);
int sed_bce_sel_fwd_bwd(const float* pre, const float* target, const unsigned char* clip_sel, float* loss,
                        float* dpre, int accumulate, int B, int t, int K, int ratio, int Tt,
                        float recall_factor, float weight, float grad_scale, void* workspace, void* stream);
/* sed_weak_bce_fwd_bwd with a clip selection and a criterion; the pooling modes, P, Q and dP/dp_i are
 * those of the weak-label block above, and so are target / target_frames, clip_prob (written for every
 * clip, selected or not) and the workspace (sed_weak_bce_ws_bytes()).
 *   SED_CRIT_BCE  l = -(w Y max(ln P, -100) + (1 - Y) max(ln Q, -100)), dl/dP as above
 *   SED_CRIT_MSE  l = (P - Y)^2, dl/dP = 2 (P - Y); recall_factor is not used
 *   loss = weight * sum_{b in sel} sum_k l / (S K),
 *   dpre_i = weight * grad_scale / (S K) * dl/dP * dP/dp_i * p_i q_i
 * clip_sel == NULL with SED_CRIT_BCE is sed_weak_bce_fwd_bwd, bit for bit.                         */
#define SED_CRIT_BCE 0
#define SED_CRIT_MSE 1
int sed_weak_bce_fwd_bwd_ex(const float* pre, const float* target, int target_frames,
                            const unsigned char* clip_sel, int criterion, float* clip_prob, float* loss,
                            float* dpre, int accumulate, int B, int t, int K, int ratio, int Tt, int mode,
                            float recall_factor, float weight, float grad_scale, void* workspace,
                            void* stream);
/* Frame-level consistency: pre_teacher [B][t][K] fp32 are the teacher's logits, p_T its probabilities.
 *   loss = weight * sum_{b in sel} sum_i c_i sum_k (p - p_T)^2 / (S N K)
 *   dpre[b][i][k] = weight * grad_scale / (S N K) * c_i * 2 (p - p_T) p q
 * The teacher gets no gradient.  workspace: sed_frame_mse_ws_bytes() bytes, 8-byte aligned.        */
size_t sed_frame_mse_ws_bytes(int B, int t, int K);
int sed_frame_mse_fwd_bwd(const float* pre, const float* pre_teacher, const unsigned char* clip_sel,
                          float* loss, float* dpre, int accumulate, int B, int t, int K, int ratio, int Tt,
                          float weight, float grad_scale, void* workspace, void* stream);
/* teacher[i] = alpha * teacher[i] + (1 - alpha) * student[i] over n >= 1 fp32 elements, in double,
 * rounded once; alpha in [0, 1]; alpha = 0 copies the student's bits and alpha = 1 leaves the teacher's,
 * whatever the values (infinities, NaN, -0).  Any 4-byte aligned pointers: 16-byte accesses where both buffers
 * reach a 16-byte boundary after the same number of elements, element-wise before and after it (and
 * throughout when they do not).  The buffers must not overlap.  One launch.                        */
int sed_ema_update(float* teacher, const float* student, size_t n, double alpha, void* stream);
/* Head backward: dfc_w [K][C], dfc_b [K] (overwritten) and dfeat [B][t][Wf][Cp] =
 * (dpre @ fc_w)/Wf broadcast over mel.  `dpre` is [B][t*ratio][K]: with ratio > 1 it is the
 * gradient w.r.t. the interpolate()d logits and the repeat-backward sum is folded in.  m is the
 * forward's m_out [B][t][Cp] (padded channels not read); dfeat's padded channels [C, Cp) are 0.
 * workspace: sed_head_bwd_ws_floats() floats (independent of Cp, Wf and ratio).                  */
size_t sed_head_bwd_ws_floats(int B, int t, int C, int K);
int sed_head_bwd(int dtype, const float* dpre, const float* m, const float* fc_w, float* dfc_w,
                 float* dfc_b, void* dfeat, float* workspace, int B, int t, int Wf, int C, int Cp, int K,
                 int ratio, void* stream);

/* ---- optimizer -----------------------------------------------------------------------------
 * torch.optim.Adam(amsgrad=True, weight_decay=0) step (train.py:85,103) on flat fp32 buffers of
 * n elements; `step` is the 1-based step count; grad_scale multiplies g first (1/world_size).   */
int sed_adam_amsgrad_step(float* p, const float* g, float* m, float* v, float* vmax, size_t n,
                          float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                          void* stream);
/* The same update with its per-step scalars in device memory (for replaying a captured HIP graph of the whole train step):
 * hyper fp32 [3] = {lr, lr/(1-beta1^t), 1/sqrt(1-beta2^t)} (set hyper[0] = lr once), *step = t (starts at 0).  Each call
 * advances t on the device, refreshes the bias corrections and applies lr *= lr_decay after every decay_every-th step
 * (train.py:108-110; decay_every = 0 disables).                                                                   */
int sed_adam_amsgrad_step_dev(float* p, const float* g, float* m, float* v, float* vmax, size_t n,
                              float* hyper, int* step, float beta1, float beta2, float eps,
                              float grad_scale, float lr_decay, int decay_every, void* stream);
/* Global L2 norm of the scaled gradient and the clip factor of torch.nn.utils.clip_grad_norm_(norm_type=2,
 * error_if_nonfinite=False) on a flat fp32 buffer of n elements:
 *   out[0] = (float)sqrt(sum_i ((double)(g[i] * grad_scale))^2)    -- fp64 accumulation: finite fp32 inputs never overflow, the
 *                                                                     result is the float64 norm to within one fp32 ulp
 *   out[1] = coef = min(1, max_norm / (out[0] + 1e-6f)) in fp32, torch's clamp(max=1.0); max_norm <= 0: measure only, coef = 1.
 * A NaN or inf norm propagates the way torch's does (inf -> coef 0, NaN -> coef NaN): there is no skip-step policy.
 * Two plain launches (per-workgroup fp64 partials, then one workgroup), fixed summation order, no atomics; the grid is a
 * function of n alone, so two runs give the same bits.  g is not modified: the optimizer step below applies coef.
 * partial: sed_grad_norm_nparts(n) doubles (8-byte aligned); nparts must be that value; out: 2 floats.               */
int sed_grad_norm_nparts(size_t n);
int sed_grad_norm(const float* g, size_t n, float grad_scale, float max_norm, double* partial, int nparts,
                  float* out, void* stream);
/* torch.optim.Adam / torch.optim.AdamW step with optional amsgrad, weight decay and gradient clipping, on flat fp32 buffers of
 * n elements (16-byte aligned).  Per element, with gse = grad_scale * coef[0] (coef: device pointer, e.g. out + 1 of
 * sed_grad_norm; NULL = 1):
 *   gr = g * gse                                                (clip_grad_norm_'s g.mul_(coef) of the averaged gradient)
 *   !decoupled: gr += weight_decay * p                          (torch.optim.Adam(weight_decay=))
 *    decoupled: p *= (float)(1 - lr * weight_decay)             (torch.optim.AdamW, before the update)
 *   m, v, vmax, denom, p as sed_adam_amsgrad_step; vmax NULL = amsgrad off (v takes vmax's place in denom, vmax is not touched).
 * The two scale factors are multiplied first so that the element arithmetic is sed_adam_amsgrad_step's own: with
 * weight_decay = 0, vmax given and coef NULL or 1.0f the results are bit-identical to it.  weight_decay >= 0.         */
int sed_adam_step_ex(float* p, const float* g, float* m, float* v, float* vmax, size_t n, float lr, float beta1,
                     float beta2, float eps, int step, float grad_scale, float weight_decay, int decoupled,
                     const float* coef, void* stream);
/* The same with the per-step scalars in device memory, as sed_adam_amsgrad_step_dev (same hyper / step protocol, same
 * bits in the same reduced case).  With decoupled decay (weight_decay > 0) hyper has FOUR floats: hyper[3] receives the
 * learning rate of the step being taken (hyper[0] may already hold the decayed one), and the factor is
 * (float)(1 - hyper[3] * weight_decay).                                                                               */
int sed_adam_step_ex_dev(float* p, const float* g, float* m, float* v, float* vmax, size_t n, float* hyper,
                         int* step, float beta1, float beta2, float eps, float grad_scale, float lr_decay,
                         int decay_every, float weight_decay, int decoupled, const float* coef, void* stream);

/* ---- the grouped step: parameter groups, frozen groups and a learning-rate schedule evaluated on the device (csrc/sed_optim.hip)
 * The flat buffers are the ones above (n a multiple of 4: FlatParams pads every parameter's start to 4 floats, so an aligned float4
 * belongs to one parameter).  Two tables in device memory, 16-byte aligned:
 *   tiles  int32 [nt][4] = {start4, count4, group, 0}: units of 4 floats, 1 <= count4 <= SED_OPT_TILE4, ascending and disjoint,
 *                          start4 + count4 <= n / 4, 0 <= group < ng, no tile across a parameter boundary
 *   groups float [ng][4] = {lr_scale, weight_decay, frozen (0 / 1), 0}, 1 <= ng <= SED_OPT_MAX_GROUPS
 * PRECONDITION: the library cannot read the tile table on the host; the caller validates it (train.py's build_tiles does).  The
 * kernels clip a tile to the buffer and skip a group index outside the table, so a damaged table cannot store out of bounds, but
 * what it computes is then undefined.
 * Schedule, all fp64, s = the 1-based step, W = warmup, w(s) = min(1, s / W) for W > 0 else 1, u = clamp((s - W)/(total - W), 0, 1):
 *   SED_SCHED_CONST    d = 1
 *   SED_SCHED_STEP     d = gamma^floor((s - 1) / every)
 *   SED_SCHED_COSINE   d = floor + (1 - floor) * (1 + cos(pi u)) / 2
 *   SED_SCHED_LINEAR   d = floor + (1 - floor) * (1 - u)
 *   SED_SCHED_INVSQRT  d = sqrt(max(W, 1) / max(s, W, 1))
 *   lr(s) = base_lr * w(s) * d(s)
 * sed_adam_groups_step makes two launches.  The first (one workgroup, one thread per group) does s = ++*step and writes
 *   hyper[0] = (float)lr(s), hyper[1] = (float)(1 / sqrt(1 - beta2^s)), hyper[2] = (float)lr(s + 1)        (hyper: 3 floats)
 *   gh[g]    = {(float)(lr(s) scale_g / (1 - beta1^s)), (float)(1 - lr(s) scale_g wd_g), 0, 0}             (gh: ng x 4 floats)
 * the second runs one workgroup of 256 threads per tile with sed_adam_step_ex's element arithmetic: a tile of a frozen group
 * returns at once (p, m, v, vmax keep their bits whatever g holds); wd_g == 0 runs the expressions without decay (no 0 * p term);
 * else L2 (decoupled == 0) or AdamW decay.  vmax NULL = amsgrad off; coef as in sed_adam_step_ex.  There is no host-scalar twin:
 * eager and captured steps run these two kernels.  With one group {1, wd, 0}, SED_SCHED_CONST and base_lr an fp32 value the
 * results are the bits of sed_adam_step_ex_dev(decay_every = 0). */
#define SED_OPT_TILE4 1024
#define SED_OPT_MAX_GROUPS 64
#define SED_SCHED_CONST 0
#define SED_SCHED_STEP 1
#define SED_SCHED_COSINE 2
#define SED_SCHED_LINEAR 3
#define SED_SCHED_INVSQRT 4
int sed_opt_tile4(void);
int sed_adam_groups_step(float* p, const float* g, float* m, float* v, float* vmax, size_t n, const int* tiles, int nt,
                         const float* groups, int ng, float* gh, float* hyper, int* step, double base_lr, int sched_kind,
                         int warmup, int total, int every, double gamma, double floor_lr, float beta1, float beta2, float eps,
                         float grad_scale, int decoupled, const float* coef, void* stream);
/* sed_grad_norm over the tiles of the non-frozen groups only (clip_grad_norm_ sees only parameters that have gradients): one
 * workgroup per tile leaves one fp64 partial through the same fixed LDS tree (a frozen tile writes 0.0), one workgroup folds the nt
 * partials in a fixed order; out as sed_grad_norm's.  partial: nt doubles.  No atomics; two runs give the same bits.  The group
 * index of a tile must lie below the number of rows of `groups` (at most SED_OPT_MAX_GROUPS). */
int sed_grad_norm_groups(const float* g, size_t n, const int* tiles, int nt, const float* groups, float grad_scale,
                         float max_norm, double* partial, float* out, void* stream);

/* ---- log-mel front-end ---------------------------------------------------------------------
 * multichannel_stft + multichannel_complex_to_log_mel (+ transform) for one channel batch
 * (dataset/spectogram/preprocess.py:21-45, spectograms_dataset.py:104-108):
 * wave fp32 [B][samples] -> out fp32 [B][T][n_mels], T = 1 + samples/hop; window fp32 [nfft]
 * (already zero-padded/centred); melT fp32 [n_mels][nfft/2+1] (MEL_FILTER_BANK_MATRIX^T);
 * mel_lo/mel_hi int32 [n_mels] = first/last+1 non-zero bin of each filter; mean/std [n_mels] or
 * NULL.  melT must be zero outside [mel_lo[m], mel_hi[m]) (the batched nfft-1024 kernel multiplies the whole bin
 * range of a 16-filter tile); the nfft-1024 kernels are taken for n_mels <= 64 only, more filters fall back to
 * the generic kernel.  nfft a power of two in [64, 32768].  workspace: sed_logmel_ws_bytes() -- always required, used for the
 * FFT twiddle table only while the stream is being captured or beyond four transform sizes per device; otherwise
 * the library keeps one table per (device, nfft) of its own: the FIRST call for a size allocates it, builds it
 * on `stream` and synchronises that stream once (round 5: no per-call table launch).                             */
size_t sed_logmel_ws_bytes(int B, int samples, int nfft, int hop);
int sed_logmel_fwd(const float* wave, const float* window, const float* melT, const int* mel_lo,
                   const int* mel_hi, const float* mean, const float* std, float* out, void* workspace,
                   int B, int samples, int nfft, int hop, int n_mels, void* stream);
/* multichannel_stft only: spec float2 [B][T][nfft/2+1] (complex64)                             */
int sed_stft_fwd(const float* wave, const float* window, void* spec, void* workspace, int B,
                 int samples, int nfft, int hop, void* stream);

/* multichannel_complex_to_log_mel on an existing spectrogram (preprocess.py:39-45; the in-loop
 * "Complex" mode of spectograms_dataset.py:104-110): spec float2 [nframes][bins] ->
 * out fp32 [nframes][n_mels] = 10*log10(max(1e-10, |spec|^2 . mel)) (optionally z-scored).       */
int sed_complex_to_logmel(const void* spec, const float* melT, const int* mel_lo, const int* mel_hi,
                          const float* mean, const float* std, float* out, size_t nframes, int bins,
                          int n_mels, void* stream);

/* In-loop "Complex" mode of SpectogramDataset (spectograms_dataset.py:58-78, 104-135) on a
 * spectrogram bank resident in HBM: bank float2 [bank_frames][bins] = all training STFTs
 * concatenated on the frame axis (:163).  For sample b: nmix[b] in 1..4 crops starting at frames
 * starts[b][0..nmix[b]-1] are averaged (augment_mix_samples :120-135; the label max is host
 * logic), real Gaussian noise of std noise_std[b] is added when > 0 (augment_add_noise :112-118),
 * the result is z-scored with the COMPLEX mean / real std per bin (transform :105; NULL = skip)
 * and converted with multichannel_complex_to_log_mel (preprocess.py:39-45).
 * noise (nullable) [B][crop][bins] standard-normal draws; NULL = generated in the kernel from
 * (seed, element index) with the counter-based generator restated in oracle/dataset_oracle.py.
 * starts_host/nmix_host are HOST copies of the device tables starts [B][4] / nmix [B]: they are
 * validated against bank_frames before anything is launched.  out fp32 [B][crop][n_mels].        */
int sed_complex_augment_logmel(const void* bank, size_t bank_frames, const int* starts_host,
                               const int* nmix_host, const int* starts, const int* nmix,
                               const float* noise_std, const float* noise, unsigned long long seed,
                               const void* cmean, const float* cstd, const float* melT,
                               const int* mel_lo, const int* mel_hi, float* out, int B, int crop,
                               int bins, int n_mels, void* stream);

/* "logMel" mode of SpectogramDataset.__getitem__ + transform (spectograms_dataset.py:66-69,
 * 104-108) for a batch: out[b][t][m] = (bank[starts[b]+t][m] - mean[m]) / std[m]; bank fp32
 * [bank_frames][n_mels] resident in HBM.  starts_host = host copy of starts (validated first).  */
int sed_logmel_crops(const float* bank, size_t bank_frames, const int* starts_host,
                     const int* starts, const float* mean, const float* std, float* out, int B,
                     int crop, int n_mels, void* stream);

/* Log-mel batch augmentation (csrc/sed_augment.hip), this build only: crop gather + per-mel z-score as in sed_logmel_crops, then a
 * circular time shift, an additive band gain, mixup with a partner sample and SpecAugment time / frequency masks, for features and
 * labels, without an intermediate tensor.  Every decision is the caller's: row b of the int32 table tab [B][row_ints],
 * row_ints = sed_logmel_augment_row_ints(n_tmask, n_fmask) = 4 + 2*(n_tmask + n_fmask), holds
 *   start, shift, partner, lam (float bits), t0_0, w_0, ... (n_tmask pairs), f0_0, w_0, ... (n_fmask pairs).
 * With T = crop, all feature arithmetic in fp32:
 *   z_b[t][f]   = bank[start_b + t][f], with mean / std given (bank[start_b + t][f] - mean[f]) / std[f]
 *   u_b[t][f]   = z_b[(t - shift_b) mod T][f] + gain[b][f]            (the shift wraps inside the crop; gain NULL = no term)
 *   v_b         = u_b if partner_b == b, else lam_b * u_b + (1 - lam_b) * u_partner_b   (the partner's own start, shift, gain)
 *   out[b][t][f] = mask_value if t lies in a time interval [t0, t0 + w) or f in a frequency interval of row b, else v_b[t][f]
 *   r_b[t][k]   = events[start_b + (t - shift_b) mod T][k]
 *   ev_out[b]   = r_b if partner_b == b, else max(r_b, r_p) (label_mix 0) or lam * r_b + (1 - lam) * r_p in double (label_mix 1);
 *                 masks do not touch labels.  events NULL = no labels (K, ev_out ignored); the labels are a second small launch.
 * bank fp32 [bank_frames][n_mels], events double [bank_frames][K], gain fp32 [B][n_mels], out fp32 [B][crop][n_mels], ev_out
 * double [B][crop][K].  A plain (B, T, F) tensor is bank = x, start_b = b*T.  float4 loads / stores when n_mels % 4 == 0 and bank,
 * gain and out are 16-byte aligned, element-wise otherwise.  tab_host is the HOST copy of tab.  Refused before any launch
 * (non-zero): sizes <= 0, more than 8 masks of a kind, mean without std, events without ev_out or K <= 0, start + crop >
 * bank_frames, shift outside [0, crop), partner outside [0, B), lam NaN or outside [0, 1], an interval with t0 < 0, w < 0 or
 * t0 + w > crop (n_mels for the frequency ones), out overlapping bank or gain, ev_out overlapping events; last, a NULL out / tab. */
int sed_logmel_augment_row_ints(int n_tmask, int n_fmask);
int sed_logmel_augment(const float* bank, size_t bank_frames, const double* events, int K, const float* mean, const float* std,
                       const int* tab_host, const int* tab, const float* gain, float mask_value, int label_mix, float* out,
                       double* ev_out, int B, int crop, int n_mels, int n_tmask, int n_fmask, void* stream);

/* ---- audio ingest: PCM decode + channel downmix + polyphase resampling (csrc/sed_resample.hip) ----
 * read_multichannel_audio (dataset/dataset_utils.py:65-91): what the reference does with soundfile's float64 decode, the channel
 * rule of :72-83 and librosa.resample, with scipy.signal.resample_poly(x, up, down)'s defaults (zero extension, Kaiser beta = 5)
 * as the resampler (the documented deviation of this build's dataset_utils.py):
 *   y[m] = sum_k h[m*down + half - k*up] * x[k],  m = 0 .. ceil(n_in*up/down) - 1,  half = 10*max(up, down),
 *   h = up * firwin(2*half + 1, 1/max(up, down), window = ('kaiser', 5.0)); terms with an index outside h or x are absent.
 * pcm [B][n_in][ch_in] interleaved frames of `pcm_dtype`: int16 (scaled by 2^-15), int32 (2^-31) or float32 (as is).
 * out fp32 [B][ch_out][n_out].  Channel map: ch_out == 1 the mean over ch_in; ch_in < ch_out the mean, duplicated; ch_in > ch_out > 1
 * the first ch_out channels; equal counts the identity.  Integer sums are exact and the scaling and division run in fp64 before the
 * one rounding to fp32: with up == down == 1 (decode + downmix alone, taps may be NULL) integer PCM gives float32(host path) bit for bit.
 * taps fp32 [up][Tp], designed by the caller in float64: taps[p][i] = (float)h[p + i*up], 0 where p + i*up > 2*half, with
 * Tp = *h_phase_len of sed_resample_plan (20*max(up, down)/up + 1, made odd).  fp32 fmaf accumulation.
 * up, down coprime in 1..640 (every pair among 8, 11.025, 16, 22.05, 24, 32, 44.1, 48 and 96 kHz except 11.025 kHz against 32 or
 * 96 kHz, which reduce to 1280/441 and 1280/147); n_out must be ceil(n_in*up/down); B <= 65535; 1..64 channels.
 * sed_resample_plan: host-only, no launch; *h_tile = outputs per workgroup (either pointer may be NULL).                        */
enum { SED_PCM_I16 = 0, SED_PCM_I32 = 1, SED_PCM_F32 = 2 };
int sed_resample_plan(int up, int down, int* h_phase_len, int* h_tile);
int sed_resample_poly(int pcm_dtype, const void* pcm, const float* taps, float* out, int B, int n_in, int n_out, int ch_in,
                      int ch_out, int up, int down, void* stream);

/* ---- CRNN head: mean over mel -> bidirectional GRU -> Linear (BASELINE.json configs[3]) -------
 * Not in the reference repository; semantics are torch.nn.GRU's
 * (batch_first, bidirectional, gate order r,z,n; h' = (1-z) n + z h).  The FC on the GRU output
 * reuses sed_head_fwd / sed_head_bwd with dtype SED_F32, Wf = 1, C = Cp = 2*Hd.
 *
 * mean over the mel axis (spectogram_models.py:193): feat [rows][Wf][Cp] (dtype) -> m [rows][C]
 * fp32, and its backward dm -> dfeat (padding channels written as 0).                           */
int sed_mel_mean_fwd(int dtype, const void* feat, float* m, size_t rows, int Wf, int C, int Cp,
                     void* stream);
int sed_mel_mean_bwd(int dtype, const float* dm, void* dfeat, size_t rows, int Wf, int C, int Cp,
                     void* stream);
/* C[M][N] = A[M][K] . B[N][K]^T (+ bias[N]); row-major fp32 in memory, MFMA compute in
 * compute_dtype (SED_BF16: bf16 operands, fp32 accumulate; SED_F32: fp32 MFMA).  ksplit > 1 splits
 * K over workgroups (fixed-order reduction through `workspace`, sed_gemm_nt_ws_floats floats; no
 * bias then).  lda/ldb multiples of 4, A/B 16-byte aligned.
 * Pinned by tests/test_gpu_crnn_exact_oracle.py: the split is kchunk = ceil(ceil(K / ksplit) / 32) * 32 columns per slab and
 * ceil(K / kchunk) slabs (fewer than ksplit when K is short; one slab = the unsplit path, no workspace touched); only columns
 * 0 .. K-1 of a row of A / B are read (the padding up to lda / ldb may hold anything), only columns 0 .. N-1 of a row of C and the
 * first sed_gemm_nt_ws_floats floats of the workspace are written.  Refused (non-zero, nothing launched): a bias or a NULL workspace
 * with ksplit > 1, lda / ldb < K or not a multiple of 4, ldc < N, A or B not 16-byte aligned.                                     */
size_t sed_gemm_nt_ws_floats(int M, int N, int ksplit);
int sed_gemm_nt(int compute_dtype, const float* A, int lda, const float* B, int ldb,
                const float* bias, float* C, int ldc, int M, int N, int K, int ksplit,
                float* workspace, void* stream);
/* dst[c][r] = src[r - shift][c] for rows grouped in sequences of `seq` rows (0 where r - shift
 * leaves the sequence); shift in {-1, 0, +1}.  shift = +1 / -1 builds the "previous hidden state"
 * matrix of a forward / reverse recurrence, already transposed for the weight-gradient GEMM.     */
int sed_transpose_shift(const float* src, int ld_src, float* dst, int ld_dst, int R, int C, int seq,
                        int shift, void* stream);
/* Round 6: C[M][N] = sum_k A[k][m] . B[k - shift][n] -- both operands row-major fp32 with the reduction index k on the ROWS (A [K][lda],
 * B [K][ldb]): the weight-gradient products of the recurrence without transposing anything.  B's rows are shifted by `shift` in
 * {-1, 0, +1} inside sequences of `seq` consecutive rows (K % seq == 0; a row that leaves its sequence contributes zero): shift = +1 /
 * -1 pairs a gate gradient with the PREVIOUS hidden state of a forward / reverse recurrence.  colsum (nullable) [M] = sum_k A[k][m] (the
 * bias gradients).  ksplit > 1 splits K over workgroups, fixed-order reduction through `workspace` (sed_gemm_tn_ws_floats floats).
 * lda/ldb multiples of 4, A/B 16-byte aligned.  Replaces sed_transpose_shift x 5 + sed_gemm_nt x 4 + sed_row_sums x 4 of the BPTT tail.
 * Pinned by tests/test_gpu_crnn_exact_oracle.py: slabs of kchunk = ceil(ceil(K / ksplit) / 64) * 64 rows, ceil(K / kchunk) of them.
 * M and N need not be multiples of 4: only columns 0 .. M-1 / 0 .. N-1 of a row of A / B are read.  The rows of B that a shift
 * excludes (the last row of every sequence for shift = +1, the first for shift = -1) are never read; with seq = 1 and a shift C is
 * exactly 0.  colsum is summed from the fp32 values of A (before any bf16 rounding) and written once per problem, whatever N is.
 * Refused (non-zero, nothing launched): lda < M, ldb < N, ldc < N, lda / ldb not a multiple of 4, A or B not 16-byte aligned,
 * K % seq != 0, a shift outside {-1, 0, +1}, ksplit > 1 without a workspace; for the batch, n outside 1 .. 8.                      */
size_t sed_gemm_tn_ws_floats(int M, int N, int ksplit);
int sed_gemm_tn(int compute_dtype, const float* A, int lda, const float* B, int ldb, float* C, int ldc, float* colsum, int M, int N,
                int K, int seq, int shift, int ksplit, float* workspace, void* stream);
/* The same product for up to 8 independent problems in ONE launch plus ONE reduction launch (each problem with its OWN workspace): the
 * four weight-gradient products of a bidirectional layer's BPTT tail (dW_ih, dW_hh and their biases, two directions) -- 12 launches of
 * 2-3 GFLOP each as four sed_gemm_tn calls.  Fields as sed_gemm_tn's arguments.                                                       */
typedef struct sed_gemm_tn_desc {
    const float* A; const float* B; float* C; float* colsum; float* workspace;
    int lda, ldb, ldc, M, N, K, seq, shift, ksplit;
} sed_gemm_tn_desc;
int sed_gemm_tn_batch(int compute_dtype, const sed_gemm_tn_desc* problems, int n, void* stream);
/* out[r] = sum_c src[r][c] (bias gradients from the transposed gate gradients)                   */
int sed_row_sums(const float* src, int ld, float* out, int R, int C, void* stream);
/* Recurrent weights weight_hh_l0 / weight_hh_l0_reverse ([3Hd][Hd] fp32) -> MFMA-fragment order in
 * `dtype`, for the forward recurrence (pack_fwd) and for its transpose product in BPTT (pack_bwd);
 * each buffer holds sed_gru_pack_elems(Hd) elements.  Hd: multiple of 32, <= 256.                */
size_t sed_gru_pack_elems(int Hd);
int sed_gru_pack_weights(int dtype, const float* whh_fwd, const float* whh_rev, void* pack_fwd,
                         void* pack_bwd, int Hd, void* stream);
/* Forward recurrence of both directions.  gi [B*t][2][3Hd] = x.W_ih^T + b_ih (sed_gemm_nt);
 * bhh [2][3Hd]; hseq [B*t][2][Hd] (= nn.GRU output (B, t, 2Hd)); saved (nullable for inference)
 * [B*t][2][4][Hd] = r, z, n, W_hn h + b_hn for the backward pass.  h0 = 0.
 * Where SED_BF16 rounds (pinned by tests/test_gpu_crnn_exact_oracle.py for both forms of the kernels): W_hh and
 * the previous state are rounded to bf16 (nearest even) as operands of the product W_h* h only; the accumulation, the gates, the
 * blend h' = n + z (h - n) on the fp32 previous state, hseq and all four planes of `saved` are fp32.  saved == NULL gives the same
 * hseq bits.  Rows of hseq / saved past B*t are never written, whatever part of its last chunk B fills.  Sizes: the kernels
 * address with 32-bit byte offsets and B*t*8*Hd*4 bytes (the `saved` tensor) must stay below 4 GiB.  That check counts the real
 * rows only: the offset of a chunk row PAST the batch is computed too, and within (chunk rows - 1) * t rows of the limit it can
 * wrap back into range instead of being dropped -- stay clear of the limit by that margin (not tested: it takes a 4 GiB case). */
int sed_gru_seq_fwd(int dtype, const float* gi, const float* bhh, const void* pack_fwd, float* hseq,
                    float* saved, int B, int t, int Hd, void* stream);
/* BPTT: dhseq [B*t][2][Hd] -> dgi, dgh [B*t][2][3Hd] (gradients w.r.t. the input-side and the
 * hidden-side gate pre-activations).  The weight/bias/input gradients follow as plain GEMMs.
 * A pure function of dhseq, hseq, saved, pack_bwd.  dgi = (dr, dz, dn), dgh = (dr, dz, dn * r), all fp32 from fp32 gate math;
 * SED_BF16 rounds only the operands of the carry product dgh . W_hh (the step's dgh and W_hh, to bf16); the direct path dh * z
 * and the carry itself stay fp32.  Same size limit and the same remark on rows past the batch as the forward call.              */
int sed_gru_seq_bwd(int dtype, const float* dhseq, const float* hseq, const float* saved,
                    const void* pack_bwd, float* dgi, float* dgh, int B, int t, int Hd, void* stream);

/* ---- evaluation ----------------------------------------------------------------------------
 * calculate_metrics / compute_recall_precision (utils/metric_utils.py:4-37) without leaving the
 * device: output [n_out][K], target [n_tgt][K] fp32, N = min(n_out, n_tgt) frames are scored.
 * raw_logits != 0: output holds raw logits and torch.sigmoid (train.py:43) is applied first;
 * prob_out (nullable) [N][K] receives the probabilities.  thresholds: HOST array of nth (<= 64)
 * ascending fp64 values (np.arange(0, 1.05, 0.05) in the reference); the decision is the
 * reference's strict  (double)p > th.  counts (device) [nth][2] uint64 = {TP, positives} with
 * TP = #((2T - O) == 1); gt_sum (device) [1] fp64 = T.sum().  workspace: device scratch of
 * sed_metric_counts_ws_bytes(nth) bytes, 8-byte aligned.                                        */
size_t sed_metric_counts_ws_bytes(int nth);
int sed_metric_counts(const float* output, const float* target, float* prob_out,
                      const double* thresholds, int nth, int raw_logits,
                      unsigned long long* counts, double* gt_sum, void* workspace, size_t n_out,
                      size_t n_tgt, int K, void* stream);

/* ---- event decoding (csrc/sed_events.hip) -----------------------------------------------------
 * Between the frame probabilities and the event scores, without leaving the device.  Tensors are contiguous [B][T][K] (time in the
 * middle, classes innermost).  Every output is a selection or an integer: the results are exact and the same from run to run.
 *
 * sed_median_time: out[b][t][k] = median of in[b][r(t + j)][k], j = -h .. h, win = 2h + 1 odd in 1..511 (1 copies), with the
 * half-sample-symmetric reflection r(i): i mod 2T, then i if < T else 2T - 1 - i, applied as often as needed (win > T is legal):
 * scipy.ndimage.median_filter(x, size=(1, win, 1), mode='reflect').  The result is one of the window's values bit for bit (the
 * values are ordered as fp32 with -0 below +0; inputs are expected finite).  in == out is refused.  B <= 65535, T <= 2^30.
 * sed_median_time_tile: host-only, the outputs per workgroup (no output depends on it).
 *
 * sed_decode_events: per (b, k) row, p[t] = prob[b][t][k] compared in fp32:
 *   1. a candidate run is a maximal interval of p[t] > th_lo (strict); it is kept if one of its frames has p[t] > th_hi
 *      (th_lo <= th_hi; equal: plain thresholding);
 *   2. consecutive kept runs with at most max_gap (>= 0) frames between them merge, and merging chains;
 *   3. a merged event [onset, offset) shorter than min_len (>= 1) frames is dropped -- merge first, then drop.
 * decisions (nullable) uint8 [B][T][K]: 1 inside the surviving events (merged gaps filled), 0 elsewhere.  events int32
 * [max_events][4] = (b, k, onset, offset), offset exclusive, in ascending (b, k, onset) order: rows are counted, the counts prefix-
 * summed, and every row writes at its own offset.  row_counts int32 [B*K]; total int32 [1] = the true number of events: when it
 * exceeds max_events exactly the first max_events are written (events may be NULL with max_events == 0).  A row has at most
 * ceil(T/2) events; B*K*ceil(T/2) must stay below 2^31.  workspace: sed_decode_events_ws_bytes(B, T, K) bytes, 4-byte aligned
 * (0 for a shape the call refuses).  sed_decode_events_chunk: host-only, the frames a wave takes per step (rows of any length work).
 *
 * sed_segment_counts: decisions uint8 [B][T][K], target fp32 [B][Tt][K]; n = min(T, Tt) frames are scored (the truncation of
 * WeightedBCE and calculate_metrics).  Segment s = frames [s*seg_frames, min((s+1)*seg_frames, n)); it is active in the decisions
 * if any frame is non-zero, in the target if any frame is > 0.5.  counts int64 [K][3] = (TP, FP, FN) over b and s.  K <= 65535.  */
int sed_median_time_tile(void);
int sed_median_time(const float* in, float* out, int B, int T, int K, int win, void* stream);
int sed_decode_events_chunk(void);
size_t sed_decode_events_ws_bytes(int B, int T, int K);
int sed_decode_events(const float* prob, int B, int T, int K, float th_hi, float th_lo, int max_gap, int min_len,
                      unsigned char* decisions, int* events, int max_events, int* row_counts, int* total, void* workspace,
                      void* stream);
int sed_segment_counts(const unsigned char* decisions, const float* target, int B, int T, int Tt, int K, int seg_frames,
                       long long* counts, void* stream);

/* ---- rank metrics (csrc/sed_rank.hip) ---------------------------------------------------------
 * Corpus-level average precision, ROC-AUC and the best-F1 operating point per class: a key-only segmented radix sort and one scan.
 * Every count is an integer and AP is a fixed-shape double sum: a given (n, K) and data give the same bits on every run.
 *
 * Scored elements, per class k: the first n = min(n_score, n_tgt) rows of score / target fp32 [rows][K] (classes innermost; the
 * truncation of calculate_metrics).  An element is positive if target > 0.5 (the rule of sed_segment_counts).  A score is valid if
 * 0 <= p <= 1 in fp32; -0 counts as +0.  key = (bits(p) << 1) | positive: below 2^31, ordered like (p, label).  NaN and
 * out-of-range scores are packed as key 0 and counted in invalid[k].
 * Tie groups: with the keys sorted, walk from the highest score down; a tie group g is a maximal run of equal key >> 1, tp_g / fp_g
 * its positives / negatives, TP_g / n_g the positives / elements down to and including it, P = sum tp_g, Nneg = n - P.
 *   AP          = sum_g (tp_g / P) * (TP_g / n_g) in double, the two divisions and the product in that order (sklearn's
 *                 average_precision_score); NaN when P = 0.
 *   auc2        = sum_g fp_g * (2 TP_{g-1} + tp_g), an integer: AUC = auc2 / (2 P Nneg) (undefined when P = 0 or Nneg = 0).
 *   best point  = the group maximising F1_g = 2 TP_g / (n_g + P), chosen by exact 64-bit cross-multiplication, an F1 tie going to the
 *                 higher score: best_tp = TP_g, best_npred = n_g, best_score = the group's score; the decision rule is
 *                 p >= best_score.  P = 0: (0, 0, +1.0).
 *
 * sed_rank_pack: the append step; writes keys[k][offset .. offset + n) of the class-major uint32 buffer [K][capacity] and ADDS the
 * number of invalid scores of class k to invalid[k] (the caller zeroes it once).  offset + n > capacity is refused.
 * sed_rank_sort: sorts the first n keys of each of the K rows ascending; [n, capacity) of every row is left alone.
 * sed_rank_curve: keys_sorted as sed_rank_sort leaves them -> ap double [K], counts uint64 [K][6] = (P, n, auc2, best_tp,
 * best_npred, number of tie groups), best_score fp32 [K].  n = 0 is legal (P = 0; nothing that reads memory is launched).
 * workspace (sort and curve; they may share it): sed_rank_ws_bytes(K, n) bytes, 16-byte aligned; 0 for a shape the calls refuse.
 * K <= 65535, n and capacity <= 2^30.  sed_rank_tile: host-only, the keys one workgroup takes per pass (rows of any length work). */
int sed_rank_tile(void);
size_t sed_rank_ws_bytes(int K, size_t n);
int sed_rank_pack(const float* score, const float* target, size_t n_score, size_t n_tgt, int K, unsigned* keys, size_t capacity,
                  size_t offset, unsigned long long* invalid, void* stream);
int sed_rank_sort(unsigned* keys, int K, size_t n, size_t capacity, void* workspace, void* stream);
int sed_rank_curve(const unsigned* keys_sorted, int K, size_t n, size_t capacity, double* ap, unsigned long long* counts,
                   float* best_score, void* workspace, void* stream);

/* ---- PSDS intersection counts (csrc/sed_psds.hip) ---------------------------------------------
 * The integer counts behind the polyphonic sound detection score (Bilen et al., ICASSP 2020) for a whole threshold sweep in one
 * launch, on the frame grid.  Every count is an integer added with integer atomics: the same bits on every run.
 *
 * prob fp32 [B][T][K] (median-filtered by the caller if wanted: sed_median_time), target fp32 [B][Tt][K], contiguous, classes
 * innermost; the first n = min(T, Tt) frames of each recording are scored.  th: HOST array of nth fp32 thresholds, 1 <= nth <= 64,
 * in any order, copied by value into the launch (the call can be captured).  Criteria as integer fractions num/den with
 * 0 < num <= den <= 2^15: DTC, GTC, CTTC.
 *   ground-truth event of class c in recording b: a maximal run of target[b][t][c] > 0.5 within [0, n).
 *   detection of class k at threshold i: a maximal run of prob[b][t][k] > th[i] within [0, n); strict, in fp32, a NaN never detects
 *     (sed_decode_events with th_lo == th_hi, max_gap = 0, min_len = 1).
 * Per (i, b, k), in integers (the products stay below 2^31 * 2^15):
 *   DTC   a detection d of length |d| is relevant if I * den_dtc >= num_dtc * |d|, I = the number of d's frames with
 *         target[..][k] > 0.5; otherwise d is a false positive.
 *   GTC   a ground-truth event g of class k is a true positive if J * den_gtc >= num_gtc * |g|, J = the number of g's frames covered
 *         by RELEVANT detections of class k.
 *   CTTC  a false-positive detection d of class k is a cross-trigger against class c != k if Ic * den_cttc >= num_cttc * |d|, Ic =
 *         the number of d's frames with target[..][c] > 0.5.  One detection may cross-trigger several classes; it still counts once
 *         as a false positive.
 * Outputs, device int64, the call ADDS to them (the caller zeroes them once, so recordings of different lengths accumulate):
 *   counts [nth][K][K + 3] = (tp, fp, ndet, ct[0..K-1]) for detected class k; ct[k] is always 0;
 *   gt     [K][2]          = (number of ground-truth events, their total frames), added once per call, not once per threshold.
 * K <= 64, B <= 65535, n <= sed_psds_max_frames(K, nth) (host-only; 0 for K / nth out of range; >= 8192 for K <= 16, nth <= 64).  A
 * shape or parameter the call cannot serve returns non-zero and launches nothing; n = 0 is legal and adds nothing.  No workspace. */
int sed_psds_max_frames(int K, int nth);
int sed_psds_counts(const float* prob, const float* target, int B, int T, int Tt, int K, const float* th, int nth, int dtc_num,
                    int dtc_den, int gtc_num, int gtc_den, int cttc_num, int cttc_den, long long* counts, long long* gt,
                    void* stream);

/* First-layer weight gradient WITHOUT the layer's pre-BN output (z1 is never read):
 *   dW1[c][k] = ca[c]*A[c][k] + cb[c]*sum_j w1[c][j]*G[j][k] + cc[c]*sx[k],
 * A = plain sed_conv3x3_c1_wgrad of g (summed partials, [9][Coutp]); G / sx = Gram matrix and sums of the
 * 3x3 input patches: sed_conv3x3_c1_gram -> gram_partial fp32 [sed_conv_c1_gram_nparts][54] (45 upper-triangle
 * products then 9 sums); the combine reduces them in fp64 and writes dwpack [9][Coutp].                */
/* Launch-count diet of the train step (same arithmetic, fewer dispatches):
 *  - sed_pack_conv_weights_batch packs every conv layer of a step in ONE launch: desc = device array of n descriptors of
 *    eight 64-bit words {w, wpack, Cout, Cin, POp, PIp, transpose_flip, first_block} (POp/PIp = packed-out / packed-in
 *    padded channels as in sed_pack_conv_weight; descriptor i owns blocks [first_block_i, first_block_{i+1}) of 1024
 *    elements each; total_blocks = the sum);
 *  - the *_u variants additionally store the weight gradient in torch's [Cout][Cin][3][3] layout from the reduction
 *    kernel itself (what a following sed_unpack_conv_wgrad call would write).                                        */
int sed_pack_conv_weights_batch(int dtype, const void* desc, int n, int total_blocks, void* stream);
/* ---- weight gradient AND data gradient of a layer in one launch: dz never written (csrc/sed_bwd_fused.hip) -----------------
 * autograd through ConvBlock, spectogram_models.py:155-158 under train.py:102.  Replaces the pair
 *   sed_conv3x3_wgrad_fused_u(..., dz_out)  +  sed_conv3x3_fwd(dz_out, wpack_t, SED_EPI_RELUBWD)          (conv2 of a block)
 *   sed_conv3x3_wgrad_fused_u(..., dz_out)  +  sed_conv3x3_dgrad_poolstats(dz_out, wpack_t, ...)           (conv1 of a block)
 * with identical operands and results: dz = the BatchNorm / ReLU / avg-pool backward of (gsrc, zsrc) as in
 * sed_conv3x3_wgrad_fused is produced into an LDS row ring, the weight gradient (dwpack + torch-layout dw) and the data
 * gradient dx [B][H][W][Cinp] (with the epilogue `epi`: SED_EPI_STORE, SED_EPI_RELUBWD with zref / epi_* as in
 * sed_conv3x3_fwd, SED_EPI_POOLSTATS with zref = pooled activation, cnt, flag as in sed_conv3x3_dgrad_poolstats) are
 * contracted from that one image.  Covered (sed_conv3x3_bwd_fused_supported): bf16, W = 32, 32 -> 64 channels with
 * SED_DZ_BN / SED_PRO_NONE / STORE or POOLSTATS, and 64 -> 64 with SED_DZ_POOL / SED_PRO_BNRELU / RELUBWD -- the two layers
 * of the main network's second block, whose two-kernel backward sits at the HBM floor of its dataflow.
 * With an epilogue, zref must be x itself (true for both layers: conv2's ReLU / BN1 reference is the z tensor its prologue
 * reads, conv1's pooled activation is its input) -- the kernel takes the reference from the tile it already holds.
 * workspace: sed_conv_wgrad_ws_floats(B, H, W, Cinp, Coutp) floats; partial [nparts][2][Cinp].                              */
/* Block 0 in C1 mode: sed_conv3x3_wgrad_fused_c1_u and sed_conv3x3_dgrad_c1_stats in ONE launch (csrc/sed_bwd_fused_c1.hip): same
 * operands, same results (dwpack / dw = conv2's weight gradient, a_partial [sed_conv_dgrad_c1_nparts()][10][32] = per-workgroup
 * partials of [A (9 taps); sum g]); dz2 is produced into an LDS row ring and never written.  workspace:
 * sed_conv_wgrad_ws_floats(B, H, 64, 32, 32) floats.  Covered: bf16, W = 64, 32 -> 32, pool 2 (..._supported).
 * relu_mask must be NULL (a non-NULL value is an error): the kernel takes conv1's ReLU decisions from the activation tile it rebuilds
 * for the weight gradient (a1 > 0 -- the same MFMA, the same bits as the forward's mask), so the forward call sed_conv3x3_fwd_c1 can
 * be given relu_mask = NULL as well and no mask tensor exists.  The argument keeps its place in the signature; the mask-given form
 * of the kernel (round 4) is gone.                                                                                              */
int sed_conv3x3_bwd_fused_c1_supported(int dtype, int W, int Coutp, int pool);
int sed_conv3x3_bwd_fused_c1(int dtype, const float* x1, const float* fmean, const float* fstd, const float* w1,
                             const float* pro_scale, const float* pro_shift, const void* gsrc, const void* zsrc,
                             const float* scale, const float* shift, const float* ca, const float* cb, const float* cc, int pool,
                             const void* wpack_t, const void* relu_mask, float* a_partial, float* dwpack, float* workspace, int B,
                             int H, int W, int Coutp, float* dw, int Cout, int Cin, void* stream);
int sed_conv3x3_bwd_fused_supported(int dtype, int W, int Cinp, int Coutp, int dzmode, int pro, int epi);
/* Round 4: the data gradient PRODUCES dz (csrc/sed_conv_pc.hip).  For the 128-output-channel layers (blocks 2-3 of the main
 * network, /root/reference/main.py:35) the weight-gradient kernel's loader waves were its critical path: besides staging two
 * operands per MFMA they computed dz = ca*g + cb*z + cc (BatchNorm / ReLU / avg-pool backward, as sed_conv3x3_wgrad_fused) and
 * wrote it out.  The data-gradient kernel has the spare loader cycles (weights stream from L2 into registers), so the pair
 *     sed_conv3x3_wgrad_fused_u(..., dz_out) ; sed_conv3x3_fwd(dz_out, wpack_t, ...)  /  sed_conv3x3_dgrad_poolstats(dz_out, ...)
 * becomes
 *     sed_conv3x3_dgrad_dz(gsrc, zsrc, ..., dz_out, dx, epi ...) ; sed_conv3x3_wgrad_u(x, dz_out, ...)
 * with identical operands and bit-identical results (dz is rounded to bf16 once, where it is produced).  C = channels of dz (the
 * layer's outputs), Cx = channels of dx (its inputs); dzmode / gsrc / zsrc / scale / shift / ca / cb / cc / pool as in
 * sed_conv3x3_wgrad_fused; epi / zref / cnt / epi_* / partial / nparts / flag as in sed_conv3x3_fwd (SED_EPI_RELUBWD, SED_EPI_STORE) and
 * sed_conv3x3_dgrad_poolstats (SED_EPI_POOLSTATS).  Covered (..._supported): bf16, W = 16 / 8, libraries built with
 * `make EXPERIMENTS=1` only -- measured bit-identical and 11 % slower than the round-3 order (tools/ab_dgrad_dz.py), so the engine
 * does not use it; the default library answers 0.                                                                              */
int sed_conv3x3_dgrad_dz_supported(int dtype, int W, int C, int Cx, int dzmode, int epi, int pool);
int sed_conv3x3_dgrad_dz(int dtype, int dzmode, const void* gsrc, const void* zsrc, const float* scale, const float* shift,
                         const float* ca, const float* cb, const float* cc, int pool, const void* wpack_t, void* dz_out, void* dx,
                         int epi, const void* zref, const void* cnt, const float* epi_scale, const float* epi_shift,
                         const float* epi_mean, const float* epi_invstd, float* partial, int nparts, int* flag, int B, int H, int W,
                         int C, int Cx, void* stream);
/* Weight gradient with dz given, gradient also in torch's [Cout][Cin][3][3] layout (dw), like sed_conv3x3_wgrad_fused_u.        */
int sed_conv3x3_wgrad_u(int dtype, int pro, const void* x, const float* pro_scale, const float* pro_shift, const void* dz,
                        float* dwpack, float* workspace, int B, int H, int W, int Cinp, int Coutp, float* dw, int Cout, int Cin,
                        void* stream);
/* The same question with the block's pooling size (what the SED_DZ_POOL form divides by): W = 32 covers pool 2 only, the
 * 128-output-channel layers at W = 16 / 8 (csrc/sed_bwd_fused_cs.hip: 64 -> 128 and 128 -> 128, the workgroups of a pixel strip
 * sliced by input channels) cover pool 1 and 2.  sed_conv3x3_bwd_fused_supported() answers for pool 2.                          */
int sed_conv3x3_bwd_fused_supported_pool(int dtype, int W, int Cinp, int Coutp, int dzmode, int pro, int epi, int pool);
int sed_conv3x3_bwd_fused(int dtype, int pro, const void* x, const float* pro_scale, const float* pro_shift, int dzmode,
                          const void* gsrc, const void* zsrc, const float* scale, const float* shift, const float* ca,
                          const float* cb, const float* cc, int pool, const void* wpack_t, void* dx, int epi, const void* zref,
                          const void* cnt, const float* epi_scale, const float* epi_shift, const float* epi_mean,
                          const float* epi_invstd, float* partial, int nparts, int* flag, float* dwpack, float* workspace,
                          int B, int H, int W, int Cinp, int Coutp, float* dw, int Cout, int Cin, void* stream);

int sed_conv3x3_wgrad_fused_u(int dtype, int pro, const void* x, const float* pro_scale,
                              const float* pro_shift, int dzmode, const void* gsrc, const void* zsrc,
                              const float* scale, const float* shift, const float* ca, const float* cb,
                              const float* cc, int pool, void* dz_out, float* dwpack, float* workspace,
                              int B, int H, int W, int Cinp, int Coutp, float* dw, int Cout, int Cin,
                              void* stream);
int sed_conv3x3_wgrad_fused_c1_u(int dtype, const float* x1, const float* fmean, const float* fstd,
                                 const float* w1, const float* pro_scale, const float* pro_shift,
                                 const void* gsrc, const void* zsrc, const float* scale,
                                 const float* shift, const float* ca, const float* cb, const float* cc,
                                 int pool, void* dz_out, float* dwpack, float* workspace, int B, int H,
                                 int W, int Coutp, float* dw, int Cout, int Cin, void* stream);
int sed_conv3x3_c1_wgrad_combine_u(const float* a_sum, const float* gram_partial, int nparts,
                                   const float* w, const float* ca, const float* cb, const float* cc,
                                   float* dwpack, int Cout, int Coutp, float* dw, void* stream);
int sed_conv_c1_gram_nparts(int B, int H, int W);
int sed_conv3x3_c1_gram(const float* x, const float* mean, const float* stdv, float* gram_partial,
                        int B, int H, int W, void* stream);
int sed_conv3x3_c1_wgrad_combine(const float* a_sum, const float* gram_partial, int nparts,
                                 const float* w, const float* ca, const float* cb, const float* cc,
                                 float* dwpack, int Cout, int Coutp, void* stream);

/* ---- "C1 mode": the first ConvBlock (spectogram_models.py:153-160) without conv1's output in memory --------
 * z1 = conv3x3(x_norm, w1) has one input channel, so the kernels that need it -- conv2 forward (as
 * relu(bn1(z1))), conv2's weight gradient, and the ReLU/BN1-backward epilogue of conv2's data gradient --
 * rebuild it in their loader waves (one MFMA per 32 pixels) from the fp32 input x1 [B][H][W] (z-scored per
 * column with fmean/fstd, nullable) and w1 [32][9]; BN1's batch statistics come from the Gram statistics of the input patches
 * (sed_conv3x3_c1_gram).  Covered: bf16, W = 64, 32 conv1 channels, conv2 32 -> 32 (sed_c1_mode_supported).  */
int sed_c1_mode_supported(int dtype, int W, int C1, int Cout2);
int sed_bn_train_finalize_c1(const float* gram_partial, int nparts, double count, const float* w1,
                             const float* gamma, const float* beta, float* running_mean,
                             float* running_var, float momentum, float eps, float* scale, float* shift,
                             float* mean, float* invstd, int C, int Cp, void* stream);
/* Round 5: sed_bn_train_finalize_c1 that also hands out the REDUCED Gram statistics gram_sum (54 doubles: the 45 upper-triangle
 * entries of the 9 x 9 patch Gram matrix, then the 9 patch sums), and the backward tail of block 0's conv1 in one launch:
 * sed_c1_bwd_tail = sed_sum_partials(a_partial [a_nparts][10][32] -> a_sum [10][32]) ; sed_bn_bwd_finalize_c1(partial = a_sum row 9,
 * nparts = 1, a_sum) ; sed_conv3x3_c1_wgrad_combine_u(a_sum, Gram, ...) with the Gram statistics taken from gram_sum instead of a
 * second reduction of the forward's partial rows.  Same formulas and rounding points; three dependent launches less per step.
 * Not for SyncBN (the all-reduce of a_sum sits between the first two steps there, and dW1 needs the LOCAL Gram).               */
int sed_bn_train_finalize_c1_g(const float* gram_partial, int nparts, double count, const float* w1,
                               const float* gamma, const float* beta, float* running_mean,
                               float* running_var, float momentum, float eps, float* scale, float* shift,
                               float* mean, float* invstd, int C, int Cp, double* gram_sum, void* stream);
int sed_c1_bwd_tail(const float* a_partial, int a_nparts, const double* gram_sum, double count, const float* w1,
                    const float* gamma, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                    float* ca, float* cb, float* cc, float* a_sum, float* dwpack, int Cout, int Coutp, float* dw,
                    void* stream);
int sed_conv3x3_fwd_c1(int dtype, int epi, const float* x1, const float* fmean, const float* fstd,
                       const float* w1, const float* pro_scale, const float* pro_shift,
                       const void* wpack, void* z, float* partial, void* relu_mask, int B, int H, int W,
                       int Coutp, void* stream);
/* relu_mask: uint16 [B][H][W][2], conv1's ReLU decisions (half g, bit i <-> channel (i&3)+8*(i>>2)+4*g), written
 * by sed_conv3x3_fwd_c1 with SED_EPI_STATS and read by the data gradient below, whose epilogue then yields
 * partial[.][0][c] = sum g only; sed_bn_bwd_finalize_c1 completes BN1's backward with sum g*z1 = w1 . A,
 * A = summed sed_conv3x3_c1_wgrad partials of g ([9][Coutp]).                                               */
int sed_conv3x3_dgrad_c1(int dtype, const void* dz, const void* wpack_t, void* g, const void* relu_mask,
                         float* partial, int B, int H, int W, int Cinp, void* stream);
/* The same data gradient FUSED with its only consumers (csrc/sed_dgrad_c1.hip): g is never written.  The kernel gates
 * conv2^T(dz) with relu_mask in the accumulator registers and contracts it over the pixels on the matrix pipe:
 * a_partial fp32 [sed_conv_dgrad_c1_nparts()][10][32], rows 0..8 = A[tap][c] = sum_px g[px][c] * xz[px + tap]
 * (what sed_conv3x3_c1_wgrad computes from g), row 9 = sum_px g[px][c] (what partial[.][0][c] holds above).
 * Summed over the partial rows (sed_sum_partials) it feeds sed_bn_bwd_finalize_c1 (partial = row 9, nparts = 1,
 * a_sum = rows 0..8) and sed_conv3x3_c1_wgrad_combine.  Covered: bf16, W = 64, 32 -> 32 channels.              */
int sed_conv_dgrad_c1_nparts(void);
int sed_conv3x3_dgrad_c1_stats(int dtype, const void* dz, const void* wpack_t, const float* x1,
                               const float* fmean, const float* fstd, const void* relu_mask,
                               float* a_partial, int B, int H, int W, void* stream);
/* test hook: the same launch additionally stores the gated g [B][H][64][32] bf16 (what sed_conv3x3_dgrad_c1 writes) */
int sed_conv3x3_dgrad_c1_stats_g(int dtype, const void* dz, const void* wpack_t, const float* x1,
                                 const float* fmean, const float* fstd, const void* relu_mask,
                                 float* a_partial, void* g_out, int B, int H, int W, void* stream);
int sed_bn_bwd_finalize_c1(const float* partial, int nparts, double count, const float* a_sum,
                           const float* w1, const float* gamma, const float* mean, const float* invstd,
                           float* dgamma, float* dbeta, float* ca, float* cb, float* cc, int C, int Cp,
                           void* stream);
/* ---- input gradient of the Cin = 1 first layer (csrc/sed_c1_dx.hip) ------------------------------------------------
 * Replaces autograd through conv1 / BN1 of the first ConvBlock down to the model input (spectogram_models.py:153-160):
 *   dz1 = ca*g + cb*z + cc  (BN1 backward, inside the image only),   dx[b][h][w] = sum_{c, tap} w1[c][tap] * dz1[b][h - dh][w - dw][c].
 * g, z [B][H][W][Coutp] (dtype SED_BF16 or SED_F32 storage), w1 fp32 [Cout][1][3][3] torch layout, ca / cb / cc fp32 [Coutp],
 * dx fp32 [B][H][W] (= the (B, 1, T, F) input gradient), fp32 accumulation.  z = NULL: z1 is recomputed from x [B][H][W] fp32
 * (z-scored on load with fmean / fstd [W] when given, as sed_conv3x3_c1_fwd).  fmean / fstd given: dx is the gradient with
 * respect to the RAW features (divided by fstd[w]).  1 <= W <= SED_ANYW_MAX_W, B <= 65535.                                     */
int sed_conv3x3_c1_dgrad(int dtype, const void* g, const void* z, const float* x, const float* fmean, const float* fstd,
                         const float* w1, const float* ca, const float* cb, const float* cc, float* dx, int B, int H, int W,
                         int Cout, int Coutp, void* stream);
/* ---- eval-mode (running-statistics) BatchNorm backward (csrc/sed_ops.hip; the C1 form: csrc/sed_c1_dx.hip) ---------------
 * Autograd through nn.BatchNorm2d in eval mode (spectogram_models.py:155-158 under model.eval()): BN is the fixed affine map
 * gamma*(z - mean_r)*invstd_r + beta.  sed_bn_eval_stats writes mean = running_mean, invstd = 1/sqrt(running_var + eps) (0 in
 * the padded channels): the (mean, invstd) operands the backward statistics kernels take (their partial rows then hold
 * (sum g, sum g*xhat) with xhat in running statistics).  The finalize reduces those rows: dbeta = sum g, dgamma = sum g*xhat,
 * ca = gamma*invstd, cb = cc = 0.  The C1 form takes sum g from row 0 only and sum g*z1 = w1 . a_sum (a_sum [9][Cp], as
 * sed_bn_bwd_finalize_c1).                                                                                                    */
/* out[0] = max |x[i]| over n fp32 elements (one device float; the upstream-gradient magnitude behind the f16x3 pre-scale of an
 * input-gradient or eval-mode backward, CnnEngine._grad_dtype).                                                               */
int sed_absmax(const float* x, size_t n, float* out, void* stream);
int sed_bn_eval_stats(const float* running_mean, const float* running_var, float eps, float* mean, float* invstd, int C, int Cp,
                      void* stream);
int sed_bn_eval_bwd_finalize(const float* partial, int nparts, const float* gamma, const float* mean, const float* invstd,
                             float* dgamma, float* dbeta, float* ca, float* cb, float* cc, int C, int Cp, void* stream);
int sed_bn_eval_bwd_finalize_c1(const float* partial, int nparts, const float* a_sum, const float* w1, const float* gamma,
                                const float* mean, const float* invstd, float* dgamma, float* dbeta, float* ca, float* cb,
                                float* cc, int C, int Cp, void* stream);
int sed_conv3x3_wgrad_fused_c1(int dtype, const float* x1, const float* fmean, const float* fstd,
                               const float* w1, const float* pro_scale, const float* pro_shift,
                               const void* gsrc, const void* zsrc, const float* scale, const float* shift,
                               const float* ca, const float* cb, const float* cc, int pool, void* dz_out,
                               float* dwpack, float* workspace, int B, int H, int W, int Coutp,
                               void* stream);

/* ---- raw-waveform M5 path (models/waveform_models.py:13-71) ------------------------------------
 * Activations use the conv3x3 layout with W = 8: eight frames interleaved on the W axis,
 * [N = B/8][L][8][Cp]; B must be a multiple of 8.  The k=3 Conv1d layers run through sed_conv3x3_*
 * with their weights expanded to 3x3 (zero side columns); these entry points add what only M5 has.
 * conv_block1.0 = Conv1d(1, 64, 79, stride 4, pad 39): x fp32 [B][L], w fp32 [64][79],
 * z [B/8][L1][8][64] with L1 = sed_m5_conv1_len(L); the bias is NOT applied (BatchNorm1d removes it).
 * stats_partial fp32 [sed_m5_conv1_nparts][2][64] (sum z, sum z^2; nullable).  What is summed: the fp32 kernels (SED_F32, and
 * SED_BF16 under SED_M5_MFMA=0) sum their fp32 accumulators, also when z is stored as bf16; the matrix-pipe kernels
 * (sed_m5_conv1_fwd in SED_BF16, sed_m5_conv1_stats) sum the bf16-rounded values as stored.
 * wgrad: dw_partial fp32 [sed_m5_conv1_nparts][80][64] (tap-major).  Tap row 79 is padding: every kernel writes it, its
 * value is UNSPECIFIED (the fp32 kernel leaves a contraction there, the matrix-pipe kernels 0) and consumers read rows
 * 0..78 only.  Every one of the nparts rows is written.
 * The pooled forms (sed_m5_conv1_bn_relu_pool_fwd, sed_m5_conv1_wgrad_fused_pool, sed_m5_conv1_dgrad_fused_pool) need
 * L1 >= 4, the sed_*maxpool4* entry points H >= 4: the pooled tensor must have at least one row.  All of them decide as MaxPool1d does:
 * the FIRST arg-max of relu(scale*z + shift) in a window of 4 (ties keep the earlier step) takes the gradient, and only
 * when that maximum is > 0 (a window whose largest pre-activation is <= 0 passes nothing).          */
int sed_m5_conv1_len(int L);
int sed_m5_conv1_nparts(int B, int L);
int sed_m5_conv1_fwd(int dtype, const float* x, const float* w, void* z, float* stats_partial, int B,
                     int L, void* stream);
int sed_m5_conv1_wgrad(int dtype, const float* x, const void* dz, float* dw_partial, int B, int L,
                       void* stream);
/* bf16: the same weight gradient on the matrix pipe with the BatchNorm1d backward produced on load,
 * dz = ca*g + cb*zsrc + cc (what sed_bn_bwd_apply would have written): dz is never materialised.                */
int sed_m5_conv1_wgrad_fused(int dtype, const float* x, const void* g, const void* zsrc, const float* ca,
                             const float* cb, const float* cc, float* dw_partial, int B, int L,
                             void* stream);
/* Two-pass forward of conv_block1 (bf16, matrix pipe): z1 is 8x its input (2.9 GB at 2880 frames) and, with one input channel, a
 * 128-step tile is 10 MFMAs per wave away from the staged input window, so the second pass computes it again (bit-identical: the same
 * MFMA sequence, rounded to bf16 where sed_m5_conv1_fwd stores it) instead of reading it back:
 *   sed_m5_conv1_stats             the BatchNorm1d statistics of sed_m5_conv1_fwd (stats_partial as there), no z
 *   sed_m5_conv1_bn_relu_pool_fwd  sed_m5_conv1_fwd + sed_bn_relu_maxpool4_fwd: y [B/8][L1/4][8][64]
 * models/waveform_models.py:15-24 (conv_block1) forward.                                                                          */
int sed_m5_conv1_stats(int dtype, const float* x, const float* w, float* stats_partial, int B, int L, void* stream);
int sed_m5_conv1_bn_relu_pool_fwd(int dtype, const float* x, const float* w, const float* scale, const float* shift, void* y,
                                  void* z_out, int B, int L, void* stream);
/* z_out (nullable): also store z [B/8][L1][8][64] for a backward that reads it -- the default bf16 forward of conv_block1 (round 4,
 * sed_m5_fwd2_supported): sed_m5_conv1_stats, the finalize, then this launch; sed_bn_relu_maxpool4_fwd's pass over z is gone.     */
int sed_m5_fwd2_supported(int dtype);
/* sed_m5_conv1_wgrad_fused with g rebuilt on load too: the MaxPool1d(4) + ReLU backward of the pooled gradient dy [B/8][L1/4][8][64]
 * (dy goes to the first arg-max of relu(scale*zsrc + shift) in each window of 4 when that maximum is > 0).  Pairs with
 * sed_maxpool4_relu_bwd(..., g = NULL, ...), which then only produces the BatchNorm-backward statistics.             */
int sed_m5_conv1_wgrad_fused_pool(int dtype, const float* x, const void* dy, const void* zsrc,
                                  const float* scale, const float* shift, const float* ca,
                                  const float* cb, const float* cc, float* dw_partial, int B, int L,
                                  void* stream);
/* Data gradient of conv_block1.0 (/root/reference/models/waveform_models.py:15-24: what autograd leaves in the waveform's .grad),
 * csrc/sed_m5_dgrad.hip:  dx[b][l] = sum_c sum_t dz[b][t][c] * w[c][l + 39 - 4t]  (0 <= l + 39 - 4t < 79, 0 <= t < L1),
 * dz [B/8][L1][8][64] in the mode's type (SED_BF16 / SED_F32), w fp32 [64][79] (rounded to bf16 in bf16 mode, as the forward
 * does), dx fp32 [B][L].  Every element of dx is written (no dependence on its previous contents) and the result is the same
 * bits on every run.  bf16 runs on the bf16 matrix pipe, fp32 on the fp32 one (exact fp32 products, fp32 accumulation).
 * sed_m5_conv1_dgrad_fused_pool (bf16): dz is rebuilt on load from the pooled gradient dy, the stored z, the layer's
 * BatchNorm scale / shift and the (ca, cb, cc) rows of sed_bn_bwd_finalize / sed_bn_eval_bwd_finalize, exactly as
 * sed_m5_conv1_wgrad_fused_pool rebuilds it: no dz tensor is written for the input gradient.                                  */
int sed_m5_conv1_dgrad(int dtype, const void* dz, const float* w, float* dx, int B, int L, void* stream);
int sed_m5_conv1_dgrad_fused_pool(int dtype, const void* dy, const void* zsrc, const float* scale, const float* shift,
                                  const float* ca, const float* cb, const float* cc, const float* w, float* dx, int B,
                                  int L, void* stream);
/* BatchNorm1d -> ReLU -> MaxPool1d(4,4) over H (floor): y [N][H/4][W][Cp] = max relu(scale*z+shift) */
int sed_bn_relu_maxpool4_fwd(int dtype, const void* z, const float* scale, const float* shift,
                             void* y, int N, int H, int W, int Cp, void* stream);
/* its backward: g [N][H][W][Cp] = dy at the FIRST arg-max of each window when that maximum is > 0,
 * else 0 (rows dropped by the floor: 0); partial fp32 [sed_maxpool4_bwd_nparts][2][Cp] =
 * (sum g, sum g*(z-mean)*invstd) for sed_bn_bwd_finalize.                                         */
int sed_maxpool4_bwd_nparts(int N, int H, int W, int Cp);
int sed_maxpool4_relu_bwd(int dtype, const void* dy, const void* z, const float* scale,
                          const float* shift, const float* mean, const float* invstd, void* g,
                          float* partial, int N, int H, int W, int Cp, void* stream);
/* Round 4: the same statistics from POOLED tensors -- g is dy at a window's arg-max where the pooled activation y is positive, and there
 * (z - mean)*invstd = (y - beta)/gamma: partial [sed_maxpool4_bwd_nparts][2][Cp] from one pass over dy and y [N][H/4][W][Cp] (the block
 * output sed_bn_relu_maxpool4_fwd / sed_m5_conv1_bn_relu_pool_fwd stored), a quarter of z's rows each.  y's bf16 rounding is amplified by
 * |beta/gamma|: a channel with |beta| > 8 |gamma| (or gamma = 0) and any active window sets *flag, and sed_maxpool4_relu_bwd_if (a no-op
 * while *flag == 0) then recomputes every partial from z as sed_maxpool4_relu_bwd(..., g = NULL) does AND resets *flag to 0 on the stream
 * afterwards: one fixed flag word (zeroed once by the caller) serves every step, also under graph replay of the pair with fixed pointers.
 * *flag_clear (nullable; kept for callers that alternate two words) is reset to 0 by sed_maxpool4_pooled_stats itself; it must not be the
 * word passed as `flag` in the same call.  Replaces the autograd backward of MaxPool1d + ReLU in front of BatchNorm1d's,
 * /root/reference/models/waveform_models.py:18-24, for a layer whose weight gradient rebuilds g itself (conv_block1).                */
int sed_maxpool4_pooled_stats(int dtype, const void* dy, const void* y, const float* scale, const float* shift, const float* mean,
                              const float* invstd, float* partial, int* flag, int* flag_clear, int N, int H, int W, int Cp, void* stream);
int sed_maxpool4_relu_bwd_if(const int* flag, int dtype, const void* dy, const void* z, const float* scale, const float* shift,
                             const float* mean, const float* invstd, float* partial, int N, int H, int W, int Cp, void* stream);
/* head: m fp32 [B][C] = mean over H of feat [B/8][H][8][Cp]; pre fp32 [B][K] = m.W^T + b; backward:
 * dfeat [B/8][H][8][Cp], dfc_w [K][C], dfc_b [K] from dpre [B][K].                                 */
int sed_m5_head_fwd(int dtype, const void* feat, const float* fc_w, const float* fc_b, float* m,
                    float* pre, int B, int H, int C, int Cp, int K, void* stream);
int sed_m5_head_bwd(int dtype, const float* dpre, const float* m, const float* fc_w, float* dfc_w,
                    float* dfc_b, void* dfeat, int B, int H, int C, int Cp, int K, void* stream);

/* ---- PCEN front-end layer: csrc/sed_pcen.hip --------------------------------------------------
 * Per-channel energy normalisation (Wang et al., ICASSP 2017) with trainable per-bin parameters, forward
 * and backward.  x, y, gy, dx fp32 [B][T][F] (the models' (B, 1, T, F) layout), F in 1..256.
 * theta fp32 [4][F] = (a, d, rho, sigma):  alpha = e^a, delta = e^d, r = e^rho, s = 1/(1 + e^-sigma).
 * eps > 0 and gain > 0 are double constants.
 *   E_t = gain 10^((x_t std_f + mean_f)/10)     kind 0: dB log-mel; mean / std fp32 [F], both NULL = 0 / 1
 *   E_t = gain max(x_t, 0)                      kind 1: linear mel power (mean / std must be NULL)
 *   M_0 = E_0;  M_t = (1 - s) M_{t-1} + s E_t
 *   u_t = eps + M_t;  G_t = E_t u_t^-alpha;  y_t = (G_t + delta)^r - delta^r
 * Backward, g = dL/dy:
 *   q_t = g_t r (G_t + delta)^(r-1);  direct_t = q_t u_t^-alpha;  m_t = -q_t alpha G_t / u_t
 *   lambda_t = m_t + (1 - s) lambda_{t+1}, lambda_T = 0
 *   dE_t = direct_t + s lambda_t (t >= 1);  dE_0 = direct_0 + lambda_0
 *   dx_t = dE_t E_t (ln 10 / 10) std_f (kind 0);  gain dE_t [x_t > 0] (kind 1: exactly 0 where x_t <= 0)
 *   dtheta[0] = alpha sum -q_t G_t ln u_t
 *   dtheta[1] = delta sum g_t r ((G_t + delta)^(r-1) - delta^(r-1))
 *   dtheta[2] = r sum g_t ((G_t + delta)^r ln(G_t + delta) - delta^r ln delta)
 *   dtheta[3] = s (1 - s) sum_{t >= 1} lambda_t (E_t - M_{t-1})            (sums over b and t)
 * All arithmetic is double (a power p^e is exp(e ln p)), every output is rounded once to fp32, M is not
 * stored.  Time is cut into chunks of sed_pcen_chunk() frames whose carries go through the workspace
 * between launches, every sum is taken in a fixed order without atomics: the same bits on every run.
 * sed_pcen_bwd depends on its arguments only (it rebuilds M from x).  dx NULL: no input gradient; dtheta
 * NULL: a fixed layer; either leaves the other output's bits as they are with both; not both NULL.
 * y and dx must not overlap x (dx nor gy).  workspace: sed_pcen_ws_bytes() bytes, 8-byte aligned.
 * Launches: forward 2, backward 3 and one more with dtheta.                                        */
int sed_pcen_chunk(void);
size_t sed_pcen_ws_bytes(int B, int T, int F);
int sed_pcen_fwd(const float* x, const float* mean, const float* std, const float* theta, int kind, double eps,
                 double gain, float* y, void* workspace, int B, int T, int F, void* stream);
int sed_pcen_bwd(const float* x, const float* mean, const float* std, const float* theta, int kind, double eps,
                 double gain, const float* gy, float* dx, float* dtheta, void* workspace, int B, int T, int F,
                 void* stream);

/* ---- attention pooling head: csrc/sed_attn.hip -------------------------------------------------
 * Beside event_fc a second linear layer att_fc scores every frame per class (decision-level attention
 * of PANNs / the DCASE task-4 baseline CRNN); the clip probability is the attention-weighted average of
 * the frame probabilities, the weights a softmax over time, per class.  pre, att [B][t][K] fp32 are the
 * frame and attention logits before interpolate(): N = min(t*ratio, Tt) virtual frames, row i stands for
 * c_i = clamp(N - i*ratio, 0, ratio) of them; rows with c_i = 0 take no part, not in the maximum either.
 * For one (b, k), x_i = pre, a_i = att, all in double, every result rounded once to fp32:
 *   p_i = 1/(1+exp(-x_i)), q_i = 1/(1+exp(x_i));  e_i = exp(a_i - a_max), a_max over the rows with c_i > 0
 *   Z = sum c_i e_i,  P = sum c_i e_i p_i / Z,  Q = sum c_i e_i q_i / Z (from its own sum)
 *   SED_CRIT_BCE  l = -(w Y max(ln P, -100) + (1 - Y) max(ln Q, -100)),
 *                 dl/dP = -w Y / max(P, 1e-12) + (1 - Y) / max(Q, 1e-12)
 *   SED_CRIT_MSE  l = (P - Y)^2, dl/dP = 2 (P - Y); recall_factor is not used
 *   loss = weight * mean of l over B*K, or over S*K for the S clips clip_sel picks (counted on the
 *   device; S = 0: loss 0 and gradient 0);  coef = weight * grad_scale / (B*K), or / (S*K)
 *   dpre_i = coef * dl/dP * (c_i e_i / Z) * p_i q_i
 *   datt_i = coef * dl/dP * c_i e_i (p_i - P) / Z        (sum_i datt_i = 0 in exact arithmetic)
 * Rows with c_i = 0 and all rows of unselected clips get exact zeros; under accumulate = 1 their dpre cells
 * are left untouched.  Every sum is taken in a fixed order without atomics (the same bits on every run);
 * no host synchronisation.
 *
 * sed_att_logits_fwd: att[r][k] = att_b[k] + sum_c m[r][c] att_w[k][c] in fp32.  m [rows][Cp] fp32 is the
 *   mel-mean sed_head_fwd leaves behind (the padded channels [C, Cp) are not read), att_w [K][C], att
 *   [rows][K]; C <= 2048.  One launch that reads every row of m once, whatever K is.
 * sed_att_pool_fwd: clip_prob [B][K] = P only (inference); one launch.
 * sed_att_loss_fwd_bwd: target / target_frames / clip_sel / criterion / clip_prob as in
 *   sed_weak_bce_fwd_bwd_ex.  dpre and datt [B][t][K] are given together or both NULL (loss only).
 *   accumulate = 1 adds to loss[0] and dpre (one fp32 add per element); datt is always overwritten.
 *   workspace: sed_att_loss_ws_bytes() bytes, 8-byte aligned.  Two launches.
 * Backward of the two linear layers through sed_head_bwd: sed_att_bwd_pack writes dcat [rows][2K] =
 *   (dpre | datt) and wcat [2K][C] = (fc_w; att_w); sed_head_bwd on them with K' = 2K and ratio 1 gives the
 *   feature gradient (dpre@fc_w + datt@att_w)/Wf, summed in fp32 and rounded once, and [2K][C] / [2K]
 *   weight and bias gradients (size its workspace for 2K); sed_att_bwd_split copies those into dfc_w
 *   [K][C], dfc_b [K], datt_w [K][C], datt_b [K].  One launch each.                                   */
int sed_att_logits_fwd(const float* m, const float* att_w, const float* att_b, float* att, int rows, int C,
                       int Cp, int K, void* stream);
int sed_att_pool_fwd(const float* pre, const float* att, float* clip_prob, int B, int t, int K, int ratio,
                     int Tt, void* stream);
size_t sed_att_loss_ws_bytes(int B, int t, int K);
int sed_att_loss_fwd_bwd(const float* pre, const float* att, const float* target, int target_frames,
                         const unsigned char* clip_sel, int criterion, float* clip_prob, float* loss,
                         float* dpre, float* datt, int accumulate, int B, int t, int K, int ratio, int Tt,
                         float recall_factor, float weight, float grad_scale, void* workspace, void* stream);
int sed_att_bwd_pack(const float* dpre, const float* datt, const float* fc_w, const float* att_w, float* dcat,
                     float* wcat, int rows, int C, int K, void* stream);
int sed_att_bwd_split(const float* dwcat, const float* dbcat, float* dfc_w, float* dfc_b, float* datt_w,
                      float* datt_b, int C, int K, void* stream);

/* ---- self-attention temporal head (csrc/sed_mhsa.hip; its LayerNorms csrc/sed_layernorm.hip) ---------------------------------------
 * The attention core of torch.nn.MultiheadAttention(C, H, batch_first=True) between its two projections (those are
 * sed_gemm_nt launches), and the residual LayerNorm behind it.
 * qkv [B*t][3C] fp32 (q | k | v, head g = columns [g*dh, (g+1)*dh) of each third), C = H*dh, scale = 1/sqrt(dh).  Per clip b and
 * head g, i and j over the t frames of that clip (no mask, no dropout):
 *   s_ij = scale * sum_c q_ic k_jc,  lse_i = max_j s_ij + ln sum_j exp(s_ij - max_j s_ij),  p_ij = exp(s_ij - lse_i),
 *   ctx_ic = sum_j p_ij v_jc                                      ctx [B*t][C], lse [B][H][t] (NULL for inference: same ctx bits)
 * Backward, D_i = sum_c dctx_ic ctx_ic per head:
 *   dv_jc = sum_i p_ij dctx_ic,  dp_ij = sum_c dctx_ic v_jc,  ds_ij = p_ij (dp_ij - D_i),
 *   dq_ic = scale sum_j ds_ij k_jc,  dk_jc = scale sum_i ds_ij q_ic          dqkv [B*t][3C], every element overwritten
 * Flash form: the t x t scores never reach memory; a wave owns 32 queries (forward, dQ pass) or 32 keys (dK / dV pass) and walks
 * the other index in tiles of 32 with fp32 running maximum and sum; P is rebuilt from qkv and lse in the backward, which is
 * three launches (D into the workspace, the key-owner pass, the query-owner pass) in a fixed order: no atomics, the same bits
 * on every run.
 * dtype: SED_BF16 rounds q, k, v and dctx to bf16 (nearest even) as MFMA operands, and the probabilities as the operand of P.V
 * (backward: P for dV, dS for dK and dQ); scores, maximum, sum, lse, D, every accumulator and every stored tensor are fp32, and the
 * sum that normalises ctx is taken over the fp32 probabilities.  SED_F32: the fp32-input MFMA, exact products.  (The f16x3 / bf16x3
 * engines pass SED_F32, as they do for the recurrent head.)
 * Any t >= 1: ragged last tiles are masked, rows past B*t are never read or written.
 * Refused (non-zero, nothing launched): sizes <= 0, dh outside {32, 64}, a dtype other than those two, a NULL pointer other than
 * lse in the forward, qkv / ctx / dctx / dqkv not 16-byte aligned, t*3C*4 >= 2^31 bytes (offsets inside a clip are 32-bit; the
 * clip base is 64-bit, so B is not limited by it) and B*H*ceil(t/128) >= 2^31 workgroups.                                       */
int    sed_mhsa_fwd(int dtype, const float* qkv, float* ctx, float* lse, int B, int t, int H, int dh, void* stream);
size_t sed_mhsa_bwd_ws_floats(int B, int t, int H, int dh);
int    sed_mhsa_bwd(int dtype, const float* qkv, const float* ctx, const float* dctx, const float* lse,
                    float* dqkv, float* workspace, int B, int t, int H, int dh, void* stream);
/* y = ((x + a) - mean) * rstd * gamma + beta per row of C: mean, then the centred sum of squares (biased variance), both fp32 in a
 * fixed order, rstd = 1/sqrt(var + eps); stats [rows][2] = (mean, rstd), NULL for inference (same y bits).
 * Backward, g = dy * gamma, xhat = ((x + a) - mean) * rstd:  dres = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)) is the
 * gradient of x and of a alike; dgamma = sum_rows dy * xhat, dbeta = sum_rows dy, through per-workgroup partials (64 rows each) in the
 * workspace and a fixed-order reduction.  Refused: sizes <= 0, NULL pointers other than stats in the forward, rows > 65535 * 64
 * in the backward.                                                                                                               */
int    sed_add_layernorm_fwd(const float* x, const float* a, const float* gamma, const float* beta, float* y,
                             float* stats, size_t rows, int C, float eps, void* stream);
size_t sed_add_layernorm_bwd_ws_floats(size_t rows, int C);
int    sed_add_layernorm_bwd(const float* dy, const float* x, const float* a, const float* gamma, const float* stats,
                             float* dres, float* dgamma, float* dbeta, float* workspace,
                             size_t rows, int C, void* stream);

/* ---- feed-forward sub-layer of the self-attention head (csrc/sed_ffn.hip) ---------------------
 * The position-wise MLP of torch.nn.TransformerEncoderLayer(C, H, D, dropout=0) between its two LayerNorms (those are
 * sed_add_layernorm_fwd launches).  x [R][C], w1 [D][C] (linear1.weight), b1 [D], w2 [C][D] (linear2.weight), b2 [C], row-major fp32:
 *   u = x . w1^T + b1,   a = act(u),   y = a . w2^T + b2                        y [R][C], u [R][D] (NULL for inference: same y bits)
 *   act: SED_ACT_RELU max(u, 0);  SED_ACT_GELU the erf form 0.5 u (1 + erf(u / sqrt 2)), torch.nn.functional.gelu's default
 * One launch: a workgroup owns 32 rows, keeps its x tile in LDS and walks D in steps of 128; the hidden tensor a never reaches global
 * memory, and the fp32 pre-activation u (accumulator plus bias, before any rounding) only when u is given, once, for the backward.
 * dtype: SED_BF16 rounds x, w1, w2 and a to bf16 (nearest even) as MFMA operands only; both accumulations, the bias adds, the
 * activation and every stored value are fp32.  SED_F32: the fp32-input MFMA, exact products.  (The f16x3 / bf16x3 engines pass SED_F32.)
 * No atomics: the same bits on every run.  Rows past R are never read or written.
 * sed_ffn_act_bwd, elementwise fp32 over n values:  a = act(u),  du = da * act'(u);  ReLU: act' = 1 for u > 0, else 0 (torch's
 * convention at 0);  GELU: Phi(u) + u phi(u).  a may be u and du may be da (each element is read before it is written); 16-byte
 * accesses when the four pointers are 16-byte aligned.  The rest of the backward is existing launches: sed_transpose_shift of w2 +
 * sed_gemm_nt (da = dy . w2), sed_gemm_tn (dw2 = dy^T . a, db2 its column sums), sed_gemm_tn (dw1 = du^T . x, db1), sed_transpose_shift
 * of w1 + sed_gemm_nt (dx = du . w1).
 * Refused (non-zero, nothing launched): R <= 0, C or D not a multiple of 32, C > 512, D > 4096, an unknown dtype or act, a NULL
 * pointer other than u, x / w1 / w2 / y / u not 16-byte aligned; sed_ffn_act_bwd: n <= 0, a NULL pointer, a partly overlapping
 * (a, u) or (du, da) pair or any other overlap of an output with another buffer.                                                */
enum { SED_ACT_RELU = 0, SED_ACT_GELU = 1 };
int sed_ffn_fwd(int dtype, int act, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                float* y, float* u, size_t R, int C, int D, void* stream);
int sed_ffn_act_bwd(int act, const float* u, const float* da, float* a, float* du, size_t n, void* stream);

/* ---- dropout of the self-attention head (csrc/philox.h, sed_dropout.hip, the _drop twins in sed_mhsa.hip / sed_layernorm.hip / sed_ffn.hip) ---------
 * Masks are generated inside the fused kernels, forward and backward, from a counter-based generator (Philox4x32-10: multipliers
 * 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds), never stored:
 *   state  rng: four uint32 in DEVICE memory (seed_lo, seed_hi, step, 0); the kernels load it (a captured graph replays with the
 *          step word its own add advanced)
 *   key    (seed_lo, seed_hi ^ stream_id), stream_id = 8 * layer + site; sites: 0 attention probabilities, 1 attention output
 *          before its residual add, 2 convolution module output before its residual add, 3 FFN hidden activation, 4 FFN output
 *          before its residual add
 *   rows   [R][N], element (r, c): counter (c >> 2, r mod 2^32, r >> 32, step), output word c & 3
 *   attn   clip b, head g, query i, key j: counter (j >> 2, i, b*H + g, step), output word j & 3
 *   keep   m = 1 iff word >= thr, thr = min(2^32 - 1, floor(p * 2^32 + 1/2)) in double from the float p; kept values are
 *          multiplied in fp32 by s = (float)(1 / (1 - (double)p)).  p = 0: every cell kept, s = 1, the plain twin's bits.
 * Each twin takes its plain entry's arguments plus (float p, const uint32_t* rng, uint32_t stream_id):
 *   sed_mhsa_fwd_drop:  lse_i and p_ij as sed_mhsa_fwd (all keys, no renormalisation);  p~_ij = m_ij s p_ij,  ctx_ic = sum_j p~_ij v_jc
 *     (running form: exp(s_ij - m_run) times m_ij s in fp32 for the P V operand only -- SED_BF16: the operand is bf16(p m s) -- the
 *     normalising sum over the undropped fp32 probabilities)
 *   sed_mhsa_bwd_drop:  dv_jc = sum_i p~_ij dctx_ic,  dp_ij = m_ij s sum_c dctx_ic v_jc,  ds_ij = p_ij (dp_ij - D_i),  D_i = sum_c dctx_ic
 *     ctx_ic with the dropped ctx (launch 1 unchanged); dq, dk from ds as sed_mhsa_bwd
 *   sed_add_layernorm_fwd_drop:  y = LayerNorm(x + m s a)
 *   sed_add_layernorm_bwd_drop:  dres (the gradient of x) as sed_add_layernorm_bwd with xhat of the dropped sum, and the extra output
 *     da [rows][C] = m s dres (the gradient of a); dgamma / dbeta use xhat of the dropped sum
 *   sed_ffn_fwd_drop:  a = m s act(u) as the operand of the second product; u is stored undropped
 *   sed_ffn_act_bwd_drop:  u, da, a, du are [R][D] (D a multiple of 4):  a = m s act(u),  du = da m s act'(u)
 * sed_dropout_mask writes the 0 / 1 keep bytes themselves: kind SED_DROP_ROWS keep[n0][n1] (t ignored), kind SED_DROP_ATTN
 * keep[n0 = B][n1 = H][t][t] -- exactly the cells the fused kernels drop.
 * A twin called with thr = 0 (p = 0) launches its plain twin's kernels (sed_add_layernorm_bwd_drop then copies dres into da).
 * Refused (non-zero, nothing launched, outputs untouched): whatever the plain twin refuses; p < 0, p >= 1, NaN; rng NULL; da NULL;
 * sed_dropout_mask: an unknown kind, keep NULL, a size <= 0.                                                                      */
enum { SED_DROP_ROWS = 0, SED_DROP_ATTN = 1 };
int sed_mhsa_fwd_drop(int dtype, const float* qkv, float* ctx, float* lse, int B, int t, int H, int dh, float p,
                      const uint32_t* rng, uint32_t stream_id, void* stream);
int sed_mhsa_bwd_drop(int dtype, const float* qkv, const float* ctx, const float* dctx, const float* lse, float* dqkv,
                      float* workspace, int B, int t, int H, int dh, float p, const uint32_t* rng, uint32_t stream_id, void* stream);
int sed_add_layernorm_fwd_drop(const float* x, const float* a, const float* gamma, const float* beta, float* y, float* stats,
                               size_t rows, int C, float eps, float p, const uint32_t* rng, uint32_t stream_id, void* stream);
int sed_add_layernorm_bwd_drop(const float* dy, const float* x, const float* a, const float* gamma, const float* stats,
                               float* dres, float* da, float* dgamma, float* dbeta, float* workspace, size_t rows, int C, float p,
                               const uint32_t* rng, uint32_t stream_id, void* stream);
int sed_ffn_fwd_drop(int dtype, int act, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                     float* y, float* u, size_t R, int C, int D, float p, const uint32_t* rng, uint32_t stream_id, void* stream);
int sed_ffn_act_bwd_drop(int act, const float* u, const float* da, float* a, float* du, size_t R, int D, float p,
                         const uint32_t* rng, uint32_t stream_id, void* stream);
int sed_dropout_mask(unsigned char* keep, int kind, size_t n0, int n1, int t, float p, const uint32_t* rng, uint32_t stream_id,
                     void* stream);

/* ---- pre-LN residual LayerNorm of the self-attention head (csrc/sed_layernorm.hip) ------------------------------------------------
 * The residual add of one sub-layer and the LayerNorm in front of the next in one launch, row-major fp32, one wave per row:
 *   forward   xsum = fma(a, s m sd, x)   (the product s * (m sd) is taken in fp32 first; m sd is sed_add_layernorm_fwd_drop's row
 *             keep factor of stream stream_id, 1 for p = 0),   y = (xsum - mean) * rstd * gamma + beta,   stats [rows][2] = (mean, rstd),
 *             NULL for inference (same y bits).  mean, then the centred sum of squares, in sed_add_layernorm_fwd's order: with s = 1
 *             the bits of y and stats are that entry's (p = 0) or its _drop twin's (p > 0), and xsum is the IEEE fp32 sum.
 *             a == NULL: y = LayerNorm(x) gamma + beta; xsum is not written and s, p, rng, stream_id are ignored.
 *             xsum must not overlap x or a.
 *   backward  g = dy gamma, xhat = (xsum - mean) rstd from the STORED xsum (neither x nor a is read again):
 *             dxsum = dres_in + rstd (g - mean_c(g) - xhat mean_c(g xhat))    the gradient of the residual stream in front of the add
 *             da    = s m sd dxsum                                            the gradient of the sub-layer output that was added
 *             dres_in NULL: no gradient arrives on the stream (with s = 1 the bits of dxsum, dgamma, dbeta are
 *             sed_add_layernorm_bwd's on (xsum, zeros)); dxsum may alias dres_in; da NULL: not written, and s, p, rng, stream_id are
 *             ignored.  dgamma = sum_rows dy xhat, dbeta = sum_rows dy through 64-row partials in the workspace
 *             (sed_resid_layernorm_bwd_ws_floats floats) and a fixed-order reduction.  No atomics: the same bits on every run.
 * p = 0 is allowed with rng == NULL (one entry, no _drop twin).  Nothing outside the rows * C elements is read or written.
 * Refused (non-zero, nothing launched, outputs untouched): sizes <= 0; a NULL x, gamma, beta, y (forward), dy, xsum, gamma, stats,
 * dxsum, dgamma, dbeta, workspace (backward); rows > 65535 * 64 in the backward; and where a / da is given: a non-finite s, xsum NULL,
 * p < 0, p >= 1 or NaN, p > 0 with rng NULL.                                                                                       */
int    sed_resid_layernorm_fwd(const float* x, const float* a, float s, const float* gamma, const float* beta, float* xsum, float* y,
                               float* stats, size_t rows, int C, float eps, float p, const uint32_t* rng, uint32_t stream_id,
                               void* stream);
size_t sed_resid_layernorm_bwd_ws_floats(size_t rows, int C);
int    sed_resid_layernorm_bwd(const float* dy, const float* dres_in, const float* xsum, const float* gamma, const float* stats,
                               float s, float* dxsum, float* da, float* dgamma, float* dbeta, float* workspace, size_t rows, int C,
                               float p, const uint32_t* rng, uint32_t stream_id, void* stream);

/* ---- local attention window of the self-attention head (the WIN instantiations in csrc/sed_mhsa.hip) ---------------------------
 * Two integers for every head: key j of the same clip takes part for query i iff i - left <= j <= i + right (torch: attn_mask
 * M[i][j] = True where j < i - left or j > i + right).  In sed_mhsa_fwd's definitions lse_i, p_ij and ctx_i run over the in-window
 * keys only and p_ij = 0 outside; in the backward ds_ij = 0 outside, and dv, dq, dk and D_i are built from those.  The diagonal is
 * always inside, so no row is empty.  A side >= t - 1 is unbounded (SED_WIN_UNBOUNDED for short); right = 0 is causal attention
 * with a look-back of left.  Dropout composes: p~_ij = m_ij s p_ij with p over the window, the counters indexed by the absolute
 * (b H + g, i, j, step), so the dropped cells are the ones sed_dropout_mask reports.
 * A wave that owns queries [q0, q0 + 31] walks only the key tiles that meet [q0 - left, q0 + 31 + right] (the dK / dV pass: keys
 * [k0, k0 + 31], query tiles that meet [k0 - right, k0 + 31 + left]); inside a visited tile cells outside the window are masked by
 * select (score -inf; backward p = dS = 0 without taking the exponential).  Fixed order, no atomics, the same bits on every run.
 * One pair of entries: p = 0 is no dropout and allowed with rng NULL, p > 0 needs rng as the _drop twins do.  The workspace is
 * sed_mhsa_bwd_ws_floats.  Both sides unbounded (after clamping to t - 1) launches the kernels of sed_mhsa_fwd / _bwd (p = 0) or of
 * the _drop twins (p > 0): their bits by construction.
 * sed_mhsa_win_tiles: per (clip, head), the number of 32 x 32 tiles on which a wave of the pass (0 forward, 1 dK / dV, 2 dQ) issues
 * MFMAs -- the loop bounds the kernels use, from the same helper; a host function, nothing is launched.  All t x t: ceil(t/32)^2.
 * Refused (non-zero, nothing launched, outputs untouched): whatever sed_mhsa_fwd / _bwd refuse; left < 0, right < 0; p < 0, p >= 1,
 * NaN; p > 0 with rng NULL.  sed_mhsa_win_tiles returns -1 for t <= 0, a negative side or an unknown pass.                         */
#define SED_WIN_UNBOUNDED 0x7fffffff
int sed_mhsa_fwd_win(int dtype, const float* qkv, float* ctx, float* lse, int B, int t, int H, int dh, int left, int right, float p,
                     const uint32_t* rng, uint32_t stream_id, void* stream);
int sed_mhsa_bwd_win(int dtype, const float* qkv, const float* ctx, const float* dctx, const float* lse, float* dqkv,
                     float* workspace, int B, int t, int H, int dh, int left, int right, float p, const uint32_t* rng,
                     uint32_t stream_id, void* stream);
long long sed_mhsa_win_tiles(int t, int left, int right, int pass);

/* ---- learned relative-position bias of the self-attention head (the REL instantiations in csrc/sed_mhsa.hip) ---------------------
 * Per head g a table over the distance d = j - i (key minus query, frames of the same clip), rel[g][d + t - 1], d in [-(t-1), t-1],
 * fp32, [H][2t - 1]:
 *     s_ij = scale * q_i . k_j + rel[g][(j - i) + t - 1]
 * and everything downstream as in the windowed entries: lse, p and ctx over the in-window keys, dropout on p, cells outside the
 * window -inf / 0 by select.  Backward: ds_ij is the gradient of the biased score (as before), dq and dk carry `scale`, and
 *     drel[g][d + t - 1] = sum_b sum_{(i, j) in the window, j - i = d} ds_ij              (no `scale`)
 * The kernels never see buckets.  sed_relpos_expand builds the table from a learned w[H][nb] and an int32 map over the 2t - 1
 * distances (rel[g][x] = w[g][map[x]], a bit copy, one small launch), sed_relpos_fold folds the table's gradient back:
 * dw[g][n] = sum_{x: map[x] = n} drel[g][x] in fp64, ascending x, rounded once; a bucket no distance maps to gets exact 0.
 * sed_mhsa_fwd_rel / _bwd_rel: the argument lists of the _win entries and, before the stream, `const float* rel` (and `float* drel`).
 * They always launch the windowed kernels (both sides unbounded is a valid window; p = 0 is no dropout).  A wave stages the slice
 * of its head's table that its tile walk can reach in LDS -- (visited keys + 31) floats, 256 visited rows (8 tiles) at a time, one
 * coalesced load of 5 floats per lane and chunk instead of 16 scattered loads per lane and tile -- and adds it after the scaling in the forward and in both backward passes.  drel: the dQ pass reduces every visited
 * 32 x 32 tile of ds along its 63 diagonals with lane exchanges in a fixed order, carries the upper half of the diagonals to the
 * next tile in a register and stores per-wave partials; a last launch sums them over the waves and clips in fp64 in a fixed order
 * and rounds once.  No atomics, the same bits on every run.  Cells outside the window, the clip or t contribute exact 0 and no
 * exponential is taken there.  A zero table gives the _win kernels' ctx, lse and dqkv bits.
 * The backward's workspace is sed_mhsa_bwd_rel_ws_floats(B, t, H, dh, left, right) floats (0 for sizes the entries refuse).
 * sed_relpos_map_check(map on the HOST, nb, t): 0 iff every one of the 2t - 1 entries lies in [0, nb) -- to be called when the map
 * is built; the kernels do not validate it (the expand kernel clamps its read, so a bad map cannot read outside w).
 * Refused (non-zero, nothing launched, outputs untouched): whatever sed_mhsa_fwd_win / _bwd_win refuse; rel or drel NULL or not
 * 4-byte aligned; expand / fold: a NULL or misaligned pointer, H outside [1, 65535], nb outside [1, 4096], t outside [1, 2^30).  */
int sed_mhsa_fwd_rel(int dtype, const float* qkv, float* ctx, float* lse, int B, int t, int H, int dh, int left, int right, float p,
                     const uint32_t* rng, uint32_t stream_id, const float* rel, void* stream);
size_t sed_mhsa_bwd_rel_ws_floats(int B, int t, int H, int dh, int left, int right);
int sed_mhsa_bwd_rel(int dtype, const float* qkv, const float* ctx, const float* dctx, const float* lse, float* dqkv,
                     float* workspace, int B, int t, int H, int dh, int left, int right, float p, const uint32_t* rng,
                     uint32_t stream_id, const float* rel, float* drel, void* stream);
int sed_relpos_map_check(const int* map_host, int nb, int t);
int sed_relpos_expand(const float* w, const int* map, float* rel, int H, int nb, int t, void* stream);
int sed_relpos_fold(const float* drel, const int* map, float* dw, int H, int nb, int t, void* stream);

/* ---- Conformer convolution module of the self-attention head (csrc/sed_convmod.hip) ------------
 * Between the attention and the feed-forward sub-layer: pointwise Conv1d(C, 2C, 1) -> GLU -> depthwise Conv1d(C, C, k, padding
 * (k-1)/2, groups=C) -> BatchNorm1d(C) -> SiLU -> pointwise Conv1d(C, C, 1).  The pointwise convolutions are sed_gemm_nt launches, the
 * BatchNorm finalisation is sed_bn_train_finalize / sed_bn_eval_coeffs (forward) and sed_bn_bwd_finalize / sed_bn_eval_stats +
 * sed_bn_eval_bwd_finalize (backward) with Cp = C.  R = B*t rows, k odd in [3, 31], p = (k-1)/2, everything row-major fp32:
 *   v[r][c]  = g[r][c] * sigmoid(g[r][C+c])                                    g [R][2C]
 *   z[b,i,c] = bias[c] + sum_{j<k} w[c][j] * v[b, i+j-p, c]                    w [C][k]; frames outside [0, t) of the SAME clip are 0
 *   partial [nparts][2][C] = per-workgroup (sum z, sum z^2), nparts = sed_dwconv_nparts(B, t) (sed_dwconv_glu_fwd_ws_floats floats);
 *            NULL: the eval form, same z bits.  v [R][C] is written only when given (a training forward keeps it: the backward reads
 *            it for the filter gradient instead of recomputing the GLU with its halo).
 *   sed_bn_silu_fwd:  s = y * sigmoid(y), y = scale[c] * z + shift[c]          z, s [R][C]
 *   sed_bn_silu_bwd_reduce:  gz = ds * sigmoid(y) * (1 + y * (1 - sigmoid(y))) (gz may be ds itself);  partial [nparts][2][C] =
 *            per-workgroup (sum gz, sum gz * (z - mean[c]) * invstd[c]), nparts = sed_bn_silu_bwd_nparts(R) = ceil(R / 128): a workgroup
 *            owns 128 rows
 *   sed_dwconv_glu_bwd:  dz = ca[c]*gz + cb[c]*z + cc[c] on load;  dv[b,i,c] = sum_j w[c][j] * dz[b, i-j+p, c];
 *            dg[r][c] = dv * sigma, dg[r][C+c] = dv * g[r][c] * sigma * (1 - sigma), sigma = sigmoid(g[r][C+c])      dg [R][2C]
 *            dw[c][j] = sum_{b,i} dz[b,i,c] * v[b, i+j-p, c], dbias[c] = sum_{b,i} dz[b,i,c]: per-workgroup partials in the workspace
 *            (sed_dwconv_glu_bwd_ws_floats floats), summed in fp64 in a fixed order by the call's second launch.
 * sigmoid(x) = 1 / (1 + expf(-x)), IEEE division.  All of it is fp32 vector arithmetic whatever the engine's precision; no atomics,
 * fixed-order sums: the same bits on every run.  A workgroup owns sed_dwconv_tile() frames of one clip and 32 channels; frames of a
 * neighbouring clip and rows past R are never read; 16-byte accesses along the channel axis.
 * Refused (non-zero, nothing launched, outputs untouched): sizes <= 0, k even or outside [3, 31], C % 4 != 0, a NULL pointer other
 * than v and partial of the forward, g / z / v / s / ds / gz / dg / workspace not 16-byte aligned, t*2C*4 >= 2^31 bytes, B > 65535. */
int    sed_dwconv_tile(void);
int    sed_dwconv_nparts(int B, int t);
size_t sed_dwconv_glu_fwd_ws_floats(int B, int t, int C);
int    sed_dwconv_glu_fwd(const float* g, const float* w, const float* bias, float* z, float* v, float* partial, int B, int t, int C,
                          int k, void* stream);
int    sed_bn_silu_fwd(const float* z, const float* scale, const float* shift, float* s, size_t R, int C, void* stream);
int    sed_bn_silu_bwd_nparts(size_t R);
int    sed_bn_silu_bwd_reduce(const float* ds, const float* z, const float* scale, const float* shift, const float* mean,
                              const float* invstd, float* gz, float* partial, size_t R, int C, void* stream);
size_t sed_dwconv_glu_bwd_ws_floats(int B, int t, int C, int k);
int    sed_dwconv_glu_bwd(const float* gz, const float* z, const float* ca, const float* cb, const float* cc, const float* v,
                          const float* g, const float* w, float* dg, float* dw, float* dbias, float* workspace, int B, int t, int C,
                          int k, void* stream);

/* ---- utilities-----------------------------------------------------------------------------*/
/* out[i] = sum_{s<nparts} partial[s][i], i < n (fixed order: deterministic)                     */
int sed_sum_partials(const float* partial, int nparts, size_t n, float* out, void* stream);
/* fp32 [n] <-> dtype [n] casts (fp32 -> bf16 rounds to nearest even, NaN stays NaN);
 * NCHW fp32 (B,C,H,W) <-> NHWC dtype (B,H,W,Cp) re-layouts: sed_nchw_to_nhwc writes +0 to the padded
 * channels [C, Cp), sed_nhwc_to_nchw does not read them                                         */
int sed_cast(int dtype_dst, void* dst, int dtype_src, const void* src, size_t n, void* stream);
int sed_nchw_to_nhwc(int dtype, const float* src, void* dst, int B, int C, int H, int W, int Cp,
                     void* stream);
int sed_nhwc_to_nchw(int dtype, const void* src, float* dst, int B, int C, int H, int W, int Cp,
                     void* stream);

/* ---- weight-gradient reduction ---------------------------------------------------------------------------------------------
 * Every weight-gradient entry point (sed_conv3x3_wgrad*, sed_conv3x3_bwd_fused, sed_conv3x3_bwd_fused_c1) ends with a launch that sums its
 * per-workgroup slabs workspace[slab][9][Cinp][Coutp] into dwpack (and dw, torch layout, where the entry point takes one): dwpack is
 * required.  Changelog: the deferred form of round 6 (dwpack == NULL, then sed_wgrad_last_slabs / sed_wgrad_reduce /
 * sed_wgrad_reduce_batch) was measured neutral and is removed with its three functions.  sed_abi_version() stays 1: the library and
 * its only binding (_lib.py, which resolves every prototype at load) ship together.                                              */

/* ---- box-measured peaks (bench.py: roofline.peak_measured) ------------------------------------------------------------------
 * SURVEY.md 8(d) asks for box-measured peaks beside the spec ones.  Both are plain launches on `stream`; the caller times them.
 * sed_peak_mfma_bf16: every SIMD of every CU issues `iters` x 64 register-fed v_mfma_f32_32x32x16_bf16 on pseudo-random operands
 *   (four waves per SIMD, four independent accumulators each; no LDS, no global traffic); *flops_out (host, nullable) = the FLOPs
 *   the launch performs.  sink: one device float (never written; anchors the loop).
 * sed_peak_stream_copy: dst[0..bytes) = src[0..bytes) with 16-byte grid-stride accesses, four loads in flight per thread: moves
 *   2 x bytes through HBM when the buffers exceed the 256 MB Infinity Cache.                                                    */
int sed_peak_mfma_bf16(int iters, float* sink, double* flops_out, void* stream);
int sed_peak_stream_copy(const void* src, void* dst, size_t bytes, void* stream);
/* sed_peak_stream_read: reads src[0..bytes) with the same access pattern and writes nothing (sink: one device float, never written):
 * the ceiling of a read-dominated kernel.                                                                                        */
int sed_peak_stream_read(const void* src, size_t bytes, float* sink, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SED_HIP_H */
