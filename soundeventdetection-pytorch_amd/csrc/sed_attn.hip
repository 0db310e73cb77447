// Attention pooling head (decision-level attention of PANNs / the DCASE task-4 baseline CRNN): beside event_fc a second linear layer
// att_fc scores every frame per class, and the clip probability is the attention-weighted average of the frame probabilities, the
// weights a softmax over time of the attention logits, per class.  Like sed_weak.hip the kernels work on the pre-interpolation
// rows [B][t][K] and never materialise the x`ratio` interpolate(): with N = min(t*ratio, Tt) virtual frames, row i stands for
// c_i = clamp(N - i*ratio, 0, ratio) frames; rows with c_i = 0 take no part (not in the maximum either) and get gradient 0.
//
// For one (b, k), x_i = pre[b][i][k] the frame logit and a_i = att[b][i][k] the attention logit, everything in double:
//   p_i = 1/(1+exp(-x_i)),  q_i = 1/(1+exp(x_i))  (= 1 - p_i without the cancellation)
//   e_i = exp(a_i - a_max), a_max over the rows with c_i > 0
//   Z = sum c_i e_i,  P = sum c_i e_i p_i / Z,  Q = sum c_i e_i q_i / Z  (from its own sum)
//   SED_CRIT_BCE  l = -(w Y max(ln P, -100) + (1 - Y) max(ln Q, -100)),  dl/dP = -w Y / max(P, 1e-12) + (1 - Y) / max(Q, 1e-12)
//   SED_CRIT_MSE  l = (P - Y)^2,  dl/dP = 2 (P - Y)
//   loss = weight * mean of l over B*K, or over S*K for the S clips a selection picks (counted here; S = 0: loss 0, gradient 0)
//   coef = weight * grad_scale / (B*K) (or / (S*K))
//   dpre_i = coef * dl/dP * (c_i e_i / Z) * p_i q_i
//   datt_i = coef * dl/dP * c_i e_i (p_i - P) / Z          (sum_i datt_i = 0 in exact arithmetic)
// each rounded once to fp32 (tests/att_formula.py is the same in numpy).  Y is the clip label [B][K], or the maximum of the strong
// target over the first N frames, taken here.  Rows with c_i = 0 and every row of an unselected clip get exact zeros; under
// accumulate = 1 their dpre cells are left untouched.  datt is always overwritten.
//
// The loss has the two-launch shape of sed_weak.hip: one workgroup per (b, k) row (the maximum, then the three sums, strided partials
// in a fixed order and fixed LDS trees) leaves P, Q, Z and a_max in the workspace, with the label workgroups behind them; then one
// thread per logit.  No atomics; the same bits on every run.
//
// sed_att_logits_fwd, att[r][k] = att_b[k] + sum_c m[r][c] att_w[k][c] in fp32, streams m [rows][Cp] once: each group of 16 lanes
// holds one or two rows of m in registers (16-byte loads, 16 lanes x 4 channels = 256 contiguous bytes per load, four or eight rows
// per wave), the weights sit in LDS and are read once per group for its rows, and every (row, class) product is a per-lane partial
// over ascending channels followed by a fixed 16-lane reduction (four DPP steps, the wave's four groups at once).  When K*C floats do not fit the LDS budget the classes go in
// chunks while the rows stay in registers: a row of m is read once whatever K is.
//
// Backward of both linear layers: sed_att_bwd_pack writes the [rows][2K] gradients (dpre | datt) and the [2K][C] weight
// (event_fc; att_fc), sed_head_bwd runs on them with K' = 2K and ratio 1 -- its feature gradient is then (dpre@fc_w + datt@att_w)/Wf,
// summed in fp32 and rounded once -- and sed_att_bwd_split copies its [2K][C] / [2K] results into the four gradient tensors.
#include "loss_common.h"

#define ATT_SLICE_VALUES 8192       // target values per label workgroup (32 per thread)
#define ATT_MAX_SLICES 64           // per clip; sed_att_loss_ws_bytes() sizes the partial maxima for it
#define ATT_LDS_FLOATS 12288        // weight floats in LDS per class chunk (48 KB)
#define ATT_GPW 4                   // groups of 16 lanes per wave; each holds RG rows of m at a time

namespace {

struct AttParams {
    const float* pre;        // [B][t][K]
    const float* att;        // [B][t][K]
    const float* target;     // [B][K] (target_frames == 0) or [B][Tt][K]; NULL: pooling only
    float* clip_prob;        // [B][K] or NULL
    float* dpre;             // [B][t][K] or NULL
    float* datt;             // [B][t][K] or NULL (given with dpre)
    float* loss;
    double* stats;           // workspace [B*K][4]: P, Q, Z, a_max
    float* ypart;            // workspace [B][nslice][K]: maxima of the strong target over each slice of frames
    int t, K, ratio, Tt, N, nrows;       // nrows = ceil(N / ratio): the rows with c_i > 0
    int rows, nslice, slice_frames;      // rows = B*K
    int target_frames, accumulate, B, criterion;
    double wpos, wg, wt;                 // recall factor; weight * grad_scale; weight
    const unsigned char* clip_sel;       // [B] or NULL
    size_t total;                        // B*t*K
};

// maxima of one slice of a clip's strong target, for every class (the coalesced per-clip scan of sed_weak.hip: thread = (frame
// offset, class), so that a wave reads consecutive floats of the [Tt][K] slab)
__device__ __forceinline__ void att_label_slice(const AttParams& a, int b, int s, float* smf) {
    const int tid = threadIdx.x;
    const int Kc = a.K < 256 ? a.K : 256, G = 256 / Kc;
    const int kk = tid % Kc, fo = tid / Kc;
    const int f0 = s * a.slice_frames, f1 = f0 + a.slice_frames < a.N ? f0 + a.slice_frames : a.N;
    const float* __restrict__ y0 = a.target + (size_t)b * a.Tt * a.K;
    for (int k0 = 0; k0 < a.K; k0 += Kc) {
        const bool live = fo < G && k0 + kk < a.K;
        float m = -INFINITY;
        if (live)
            for (int f = f0 + fo; f < f1; f += G) m = fmaxf(m, y0[(size_t)f * a.K + k0 + kk]);
        __syncthreads();
        smf[tid] = m;
        __syncthreads();
#pragma unroll
        for (int st = 128; st > 0; st >>= 1) {
            if (fo < st && fo + st < G) smf[tid] = fmaxf(smf[tid], smf[tid + st * Kc]);      // (fo + st) * Kc + kk < G * Kc <= 256
            __syncthreads();
        }
        if (live && fo == 0) a.ypart[((size_t)b * a.nslice + s) * a.K + k0 + kk] = smf[tid];
    }
}

__global__ __launch_bounds__(256) void att_rows_kernel(const AttParams a) {
    __shared__ double sm[256];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= a.rows) {         // the label workgroups sit behind the row workgroups
        const int id = (int)blockIdx.x - a.rows;
        att_label_slice(a, id / a.nslice, id % a.nslice, reinterpret_cast<float*>(sm));
        return;
    }
    const int r = blockIdx.x, b = r / a.K, k = r - b * a.K;
    const float* __restrict__ x0 = a.pre + (size_t)b * a.t * a.K + k;
    const float* __restrict__ a0 = a.att + (size_t)b * a.t * a.K + k;

    // a_max over the rows that take part (a maximum: the same in any order)
    float am = -INFINITY;
    for (int i = tid; i < a.nrows; i += 256) am = fmaxf(am, a0[(size_t)i * a.K]);
    float* smf = reinterpret_cast<float*>(sm);
    smf[tid] = am;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) smf[tid] = fmaxf(smf[tid], smf[tid + s]);
        __syncthreads();
    }
    const double amax = (double)smf[0];

    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = tid; i < a.nrows; i += 256) {
        const int left = a.N - i * a.ratio;
        const double c = (double)(left < a.ratio ? left : a.ratio);
        double p, q;
        sigmoids((double)x0[(size_t)i * a.K], p, q);
        const double ce = c * exp((double)a0[(size_t)i * a.K] - amax);
        s0 += ce;
        s1 += ce * p;
        s2 += ce * q;
    }
    s0 = block_sum(s0, sm);      // Z >= 1: the row of a_max has e = 1 and c >= 1
    s1 = block_sum(s1, sm);
    s2 = block_sum(s2, sm);
    if (tid == 0) {
        const double P = s1 / s0, Q = s2 / s0;
        if (a.clip_prob) a.clip_prob[r] = (float)P;
        if (a.stats) {
            double* __restrict__ st = a.stats + (size_t)r * 4;
            st[0] = P;
            st[1] = Q;
            st[2] = s0;
            st[3] = amax;
        }
    }
}

// the clip label of row r = (b, k): given, or the maximum of the slices' maxima
__device__ __forceinline__ double att_clip_label(const AttParams& a, int r, int b, int k) {
    if (a.target_frames == 0) return (double)a.target[r];
    const float* __restrict__ yp = a.ypart + (size_t)b * a.nslice * a.K + k;
    float m = yp[0];
    for (int s = 1; s < a.nslice; ++s) m = fmaxf(m, yp[(size_t)s * a.K]);
    return (double)m;
}

__global__ __launch_bounds__(256) void att_grad_kernel(const AttParams a) {
    __shared__ double sm[256];
    __shared__ int smi[256];
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    // the mean over the clips that take part; S == 0: no loss, no gradient
    const int S = selected_count(a.clip_sel, a.B, smi);
    const double coef = S > 0 ? a.wg / ((double)S * (double)a.K) : 0.0;
    const double loss_scale = S > 0 ? a.wt / ((double)S * (double)a.K) : 0.0;
    if (a.dpre != nullptr && idx < a.total) {
        const int k = (int)(idx % a.K);
        const size_t bt = idx / a.K;
        const int i = (int)(bt % a.t), b = (int)(bt / a.t), r = b * a.K + k;
        const bool off = a.clip_sel != nullptr && a.clip_sel[b] == 0;      // not selected: exactly 0, or what was there
        double vx = 0.0, va = 0.0;
        if (i < a.nrows && !off) {
            const double* __restrict__ st = a.stats + (size_t)r * 4;
            const double P = st[0], Q = st[1], Z = st[2], amax = st[3];
            const double Y = att_clip_label(a, r, b, k);
            const double g = a.criterion == SED_CRIT_MSE
                                 ? coef * (2.0 * (P - Y))
                                 : coef * (-a.wpos * Y / fmax(P, 1e-12) + (1.0 - Y) / fmax(Q, 1e-12));       // coef * dl/dP
            double p, q;
            sigmoids((double)a.pre[idx], p, q);
            const int left = a.N - i * a.ratio;
            const double c = (double)(left < a.ratio ? left : a.ratio);
            const double ce = c * exp((double)a.att[idx] - amax);
            vx = g * (ce / Z) * (p * q);
            va = g * ce * (p - P) / Z;
        }
        const bool idle = off || i >= a.nrows;       // under accumulate these cells are left as they are
        if (!(idle && a.accumulate)) a.dpre[idx] = a.accumulate ? a.dpre[idx] + (float)vx : (float)vx;
        a.datt[idx] = (float)va;
    }
    if (blockIdx.x != 0) return;
    double s = 0.0;
    for (int r = threadIdx.x; r < a.rows; r += 256) {
        if (a.clip_sel != nullptr && a.clip_sel[r / a.K] == 0) continue;
        const double P = a.stats[(size_t)r * 4], Q = a.stats[(size_t)r * 4 + 1];
        const double Y = att_clip_label(a, r, r / a.K, r % a.K);
        if (a.criterion == SED_CRIT_MSE) s += (P - Y) * (P - Y);
        else s -= a.wpos * Y * fmax(log(P), -100.0) + (1.0 - Y) * fmax(log(Q), -100.0);
    }
    s = block_sum(s, sm);
    if (threadIdx.x == 0) {
        const float v = (float)(s * loss_scale);
        a.loss[0] = a.accumulate ? a.loss[0] + v : v;
    }
}

// the size checks the pooling and the loss share; fills the geometry of p
static int att_geometry(AttParams& p, int B, int t, int K, int ratio, int Tt) {
    SED_REQUIRE(B > 0 && t > 0 && K > 0 && ratio > 0 && Tt > 0, "bad sizes");
    SED_REQUIRE((long long)B * K < (1ll << 24), "too many (clip, class) rows for one launch");
    SED_REQUIRE((long long)t * ratio < (1ll << 31), "t * ratio does not fit an int");
    p.B = B; p.t = t; p.K = K; p.ratio = ratio; p.Tt = Tt;
    p.rows = B * K;
    p.total = (size_t)B * t * K;
    p.N = t * ratio < Tt ? t * ratio : Tt;
    p.nrows = (p.N + ratio - 1) / ratio;
    return 0;
}

// ---- the linear layer ------------------------------------------------------------------------------------------------------------
// NV: 16-byte loads per lane, 64 channels each (C <= 64 * NV); the LDS image of a class is 64 * NV floats, zero beyond C.
// vec: rows of m start 16-byte aligned (Cp % 4 == 0 and an aligned base); else the channels are loaded one by one.
template <int NV, int RG>
__global__ __launch_bounds__(256) void att_logits_kernel(const float* __restrict__ m, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ att, int rows, int C,
                                                         int Cp, int K, int kch, int vec) {
    extern __shared__ float wl[];                // [kch][64 * NV]
    constexpr int CQ = 64 * NV;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, grp = lane >> 4;
    constexpr int RPW = ATT_GPW * RG;            // rows per wave
    const int per_iter = (int)gridDim.x * 4 * RPW;
    const int iters = (rows + per_iter - 1) / per_iter;       // the same for every workgroup: the barriers below are uniform
    const int nch = (K + kch - 1) / kch;
    for (int it = 0; it < iters; ++it) {
        const int r0 = (it * (int)gridDim.x + (int)blockIdx.x) * 4 * RPW + wave * RPW + grp * RG;
        f32x4 mr[RG][NV];
#pragma unroll
        for (int j = 0; j < RG; ++j) {
            const bool live = r0 + j < rows;
            const float* __restrict__ row = m + (size_t)(live ? r0 + j : 0) * Cp;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int c0 = 4 * (l16 + 16 * v);
                f32x4 x = {0.f, 0.f, 0.f, 0.f};
                if (live) {
                    if (vec && c0 + 3 < C) {
                        x = *reinterpret_cast<const f32x4*>(row + c0);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (c0 + e < C) x[e] = row[c0 + e];       // the padded channels [C, Cp) are not read
                    }
                }
                mr[j][v] = x;
            }
        }
        for (int ch = 0; ch < nch; ++ch) {
            const int k0 = ch * kch, kn = K - k0 < kch ? K - k0 : kch;
            if (nch > 1 || it == 0) {
                __syncthreads();
                for (int o = tid; o < kn * CQ; o += 256) {
                    const int kk = o / CQ, c = o - kk * CQ;
                    wl[o] = c < C ? w[(size_t)(k0 + kk) * C + c] : 0.f;
                }
                __syncthreads();
            }
            for (int kk = 0; kk < kn; ++kk) {
                float acc[RG];
#pragma unroll
                for (int j = 0; j < RG; ++j) acc[j] = 0.f;
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(wl + kk * CQ + 4 * (l16 + 16 * v));
#pragma unroll
                    for (int j = 0; j < RG; ++j)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[j] = fmaf(mr[j][v][e], wv[e], acc[j]);
                }
                const float bk = bias[k0 + kk];
#pragma unroll
                for (int j = 0; j < RG; ++j) {
                    const float sum = row16_sum(acc[j]);      // (all 64 lanes take part: no branch around the DPP steps)
                    if (l16 == 0 && r0 + j < rows) att[(size_t)(r0 + j) * K + k0 + kk] = bk + sum;
                }
            }
        }
    }
}

template <int NV>
static int launch_att_logits(const float* m, const float* w, const float* b, float* att, int rows, int C, int Cp, int K, hipStream_t st) {
    constexpr int CQ = 64 * NV, RG = NV <= 8 ? 2 : 1;        // two rows per group while they fit the registers (C <= 512)
    const int kch = K < ATT_LDS_FLOATS / CQ ? K : ATT_LDS_FLOATS / CQ;
    const size_t lds = (size_t)kch * CQ * sizeof(float);
    if (int rc = sed_set_max_lds<att_logits_kernel<NV, RG>>(lds)) return rc;
    const int vec = Cp % 4 == 0 && (reinterpret_cast<uintptr_t>(m) & 15) == 0;
    size_t grid = cdivz((size_t)rows, 4 * ATT_GPW * RG);
    if (grid > 768) grid = 768;           // three workgroups per compute unit: the weights are staged a few times per unit, not per row
    att_logits_kernel<NV, RG><<<(unsigned)grid, 256, lds, st>>>(m, w, b, att, rows, C, Cp, K, kch, vec);
    return 0;
}

// [rows][2K] gradients (dpre | datt) and the [2K][C] weight (fc_w; att_w): one thread per element of either
__global__ __launch_bounds__(256) void att_bwd_pack_kernel(const float* __restrict__ dpre, const float* __restrict__ datt,
                                                           const float* __restrict__ fc_w, const float* __restrict__ att_w,
                                                           float* __restrict__ dcat, float* __restrict__ wcat, size_t nd, size_t nw,
                                                           int K, int C) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < nd) {
        const size_t r = idx / (2 * (size_t)K);
        const int k = (int)(idx - r * 2 * (size_t)K);
        dcat[idx] = k < K ? dpre[r * K + k] : datt[r * K + k - K];
    } else if (idx < nd + nw) {
        const size_t o = idx - nd, half = (size_t)K * C;
        wcat[o] = o < half ? fc_w[o] : att_w[o - half];
    }
}

// the [2K][C] / [2K] results of the head backward into the four gradient tensors
__global__ __launch_bounds__(256) void att_bwd_split_kernel(const float* __restrict__ dwcat, const float* __restrict__ dbcat,
                                                            float* __restrict__ dfc_w, float* __restrict__ dfc_b,
                                                            float* __restrict__ datt_w, float* __restrict__ datt_b, int K, int C) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, half = (size_t)K * C;
    if (idx < half) dfc_w[idx] = dwcat[idx];
    else if (idx < 2 * half) datt_w[idx - half] = dwcat[idx];
    else if (idx < 2 * half + K) dfc_b[idx - 2 * half] = dbcat[idx - 2 * half];
    else if (idx < 2 * half + 2 * (size_t)K) datt_b[idx - 2 * half - K] = dbcat[idx - 2 * half];
}

}   // namespace

extern "C" int sed_att_logits_fwd(const float* m, const float* att_w, const float* att_b, float* att, int rows, int C, int Cp, int K,
                                  void* stream) {
    SED_REQUIRE(rows > 0 && C > 0 && K > 0 && Cp >= C, "bad sizes");
    SED_REQUIRE(C <= 2048, "C must be <= 2048");
    SED_REQUIRE((long long)rows * K < (1ll << 31) && rows < (1 << 28), "too many rows for one launch");
    SED_REQUIRE(m != nullptr && att_w != nullptr && att_b != nullptr && att != nullptr, "m, att_w, att_b and att are needed (null)");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (C <= 64) rc = launch_att_logits<1>(m, att_w, att_b, att, rows, C, Cp, K, st);
    else if (C <= 128) rc = launch_att_logits<2>(m, att_w, att_b, att, rows, C, Cp, K, st);
    else if (C <= 256) rc = launch_att_logits<4>(m, att_w, att_b, att, rows, C, Cp, K, st);
    else if (C <= 512) rc = launch_att_logits<8>(m, att_w, att_b, att, rows, C, Cp, K, st);
    else if (C <= 1024) rc = launch_att_logits<16>(m, att_w, att_b, att, rows, C, Cp, K, st);
    else rc = launch_att_logits<32>(m, att_w, att_b, att, rows, C, Cp, K, st);
    if (rc) return rc;
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_att_pool_fwd(const float* pre, const float* att, float* clip_prob, int B, int t, int K, int ratio, int Tt,
                                void* stream) {
    AttParams p = {};
    if (int rc = att_geometry(p, B, t, K, ratio, Tt)) return rc;
    SED_REQUIRE(pre != nullptr && att != nullptr && clip_prob != nullptr, "pre, att and clip_prob are needed (null)");
    p.pre = pre; p.att = att; p.clip_prob = clip_prob;
    att_rows_kernel<<<(unsigned)p.rows, 256, 0, (hipStream_t)stream>>>(p);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t sed_att_loss_ws_bytes(int B, int t, int K) {
    (void)t;
    return B > 0 && K > 0 ? (size_t)B * K * (4 * sizeof(double) + ATT_MAX_SLICES * sizeof(float)) : 0;
}

extern "C" int sed_att_loss_fwd_bwd(const float* pre, const float* att, const float* target, int target_frames,
                                    const unsigned char* clip_sel, int criterion, float* clip_prob, float* loss, float* dpre,
                                    float* datt, int accumulate, int B, int t, int K, int ratio, int Tt, float recall_factor,
                                    float weight, float grad_scale, void* workspace, void* stream) {
    AttParams p = {};
    SED_REQUIRE(criterion == SED_CRIT_BCE || criterion == SED_CRIT_MSE, "criterion is SED_CRIT_BCE or SED_CRIT_MSE");
    p.clip_sel = clip_sel; p.criterion = criterion;
    if (int rc = att_geometry(p, B, t, K, ratio, Tt)) return rc;
    SED_REQUIRE(target_frames == 0 || target_frames == Tt, "target_frames is 0 (clip labels [B][K]) or Tt (strong labels [B][Tt][K])");
    SED_REQUIRE(accumulate == 0 || accumulate == 1, "accumulate is 0 or 1");
    SED_REQUIRE(pre != nullptr && att != nullptr && target != nullptr && loss != nullptr && workspace != nullptr,
                "pre, att, target, loss and workspace are needed (null)");
    SED_REQUIRE((dpre == nullptr) == (datt == nullptr), "dpre and datt are given together or both NULL");
    SED_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "workspace must be 8-byte aligned");
    const size_t nblk = dpre != nullptr ? cdivz(p.total, 256) : 1;
    SED_REQUIRE(nblk < ((size_t)1 << 31), "too many logits for one launch");
    p.pre = pre; p.att = att; p.target = target; p.clip_prob = clip_prob; p.dpre = dpre; p.datt = datt; p.loss = loss;
    p.stats = static_cast<double*>(workspace);
    p.ypart = reinterpret_cast<float*>(p.stats + (size_t)p.rows * 4);
    p.target_frames = target_frames; p.accumulate = accumulate;
    p.wpos = (double)recall_factor;
    p.wg = (double)weight * (double)grad_scale;
    p.wt = (double)weight;
    if (target_frames != 0) {        // slices of about ATT_SLICE_VALUES target values, none of them empty
        size_t ns = cdivz((size_t)p.N * K, ATT_SLICE_VALUES);
        if (ns > ATT_MAX_SLICES) ns = ATT_MAX_SLICES;
        if (ns > (size_t)p.N) ns = (size_t)p.N;
        p.slice_frames = (p.N + (int)ns - 1) / (int)ns;
        p.nslice = (p.N + p.slice_frames - 1) / p.slice_frames;
    }
    hipStream_t st = (hipStream_t)stream;
    att_rows_kernel<<<(unsigned)(p.rows + B * p.nslice), 256, 0, st>>>(p);
    SED_LAUNCH_CHECK();
    att_grad_kernel<<<(unsigned)nblk, 256, 0, st>>>(p);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_att_bwd_pack(const float* dpre, const float* datt, const float* fc_w, const float* att_w, float* dcat, float* wcat,
                                int rows, int C, int K, void* stream) {
    SED_REQUIRE(rows > 0 && C > 0 && K > 0, "bad sizes");
    SED_REQUIRE(dpre != nullptr && datt != nullptr && fc_w != nullptr && att_w != nullptr && dcat != nullptr && wcat != nullptr,
                "dpre, datt, fc_w, att_w, dcat and wcat are needed (null)");
    const size_t nd = (size_t)rows * 2 * K, nw = (size_t)2 * K * C;
    const size_t nblk = cdivz(nd + nw, 256);
    SED_REQUIRE(nblk < ((size_t)1 << 31), "too many elements for one launch");
    att_bwd_pack_kernel<<<(unsigned)nblk, 256, 0, (hipStream_t)stream>>>(dpre, datt, fc_w, att_w, dcat, wcat, nd, nw, K, C);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_att_bwd_split(const float* dwcat, const float* dbcat, float* dfc_w, float* dfc_b, float* datt_w, float* datt_b,
                                 int C, int K, void* stream) {
    SED_REQUIRE(C > 0 && K > 0, "bad sizes");
    SED_REQUIRE(dwcat != nullptr && dbcat != nullptr && dfc_w != nullptr && dfc_b != nullptr && datt_w != nullptr && datt_b != nullptr,
                "dwcat, dbcat and the four gradient tensors are needed (null)");
    const size_t n = (size_t)2 * K * C + 2 * (size_t)K;
    SED_REQUIRE(cdivz(n, 256) < ((size_t)1 << 31), "too many elements for one launch");
    att_bwd_split_kernel<<<(unsigned)cdivz(n, 256), 256, 0, (hipStream_t)stream>>>(dwcat, dbcat, dfc_w, dfc_b, datt_w, datt_b, K, C);
    SED_LAUNCH_CHECK();
    return 0;
}
