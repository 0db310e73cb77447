// Weak-label (clip-level) loss: the frame probabilities of a clip are pooled over time into one clip probability per class and the
// recall-weighted BCE of utils/common.py is taken against the clip label (multiple-instance learning; max, mean, linear-softmax
// and exp-softmax pooling of Wang, Li and Metze 2019).  Like sed_bce_fwd_bwd the kernels work on the pre-interpolation logits
// pre [B][t][K] and never materialise the x`ratio` interpolate(): with N = min(t*ratio, Tt) virtual frames, row i of pre stands
// for c_i = clamp(N - i*ratio, 0, ratio) frames; rows with c_i = 0 take no part (not in the max either) and get gradient 0.
//
// For one (b, k), x_i the logit, everything in double:
//   p_i = 1/(1+exp(-x_i)),  q_i = 1/(1+exp(x_i))  (= 1 - p_i without the cancellation)
//   mode    P                                 Q = 1 - P (from its own sums)   dP/dp_i
//   max     p_j, j = smallest index of the    q_j                             1 at j, else 0
//           largest x_i among c_i > 0
//   mean    sum c_i p_i / N                   sum c_i q_i / N                 c_i / N
//   linear  S2/S1, S1 = sum c_i p_i,          sum c_i p_i q_i / S1            c_i (2 p_i - P) / S1
//           S2 = sum c_i p_i^2                (S1 == 0, every logit below about -745: P = 0, Q = 1, gradient 0)
//   exp     sum c_i p_i e^{p_i} / E,          sum c_i q_i e^{p_i} / E         c_i e^{p_i} (1 + p_i - P) / E
//           E = sum c_i e^{p_i}
//   l      = -(w Y max(ln P, -100) + (1 - Y) max(ln Q, -100)),   loss = weight * mean over B*K of l
//   dl/dP  = -w Y / max(P, 1e-12) + (1 - Y) / max(Q, 1e-12)
//   dpre_i = weight * grad_scale / (B*K) * dl/dP * dP/dp_i * p_i q_i, rounded once to fp32
// (tests/weak_formula.py is the same in numpy).  Y is the clip label [B][K], or the maximum of the strong target over the first N
// frames, taken here; it may be soft.
// sed_weak_bce_fwd_bwd_ex adds two things to the same kernels.  A clip selection, clip_sel [B] bytes (nonzero: the clip takes part):
// the mean is then over S*K for the S selected clips, counted here; unselected clips get no loss term and gradient exactly 0 (under
// accumulate their cells are not touched); S = 0 gives loss term 0 and gradient 0.  And a criterion: SED_CRIT_BCE is the l above,
// SED_CRIT_MSE is l = (P - Y)^2, dl/dP = 2 (P - Y), without the recall factor (the clip-level consistency loss of a mean teacher,
// Y its clip probabilities).  Without a selection and with SED_CRIT_BCE every value takes the path it always took.
//
// Shape: the work is small (tens to hundreds of thousands of logits) and latency-bound, so it is spread wide and takes two launches.
// First launch: one workgroup of 256 threads per (b, k) row -- strided partial sums in a fixed order, a fixed LDS tree -- leaves the
// row's P, Q and sums in the workspace; beside them, when the target is the strong tensor, a few workgroups per clip scan slices
// of its [Tt][K] slab, coalesced, for the partial maxima of every class (one workgroup per row reading its own column would pull
// each 128-byte line K times).  Second launch: one thread per logit forms dpre from its row's workspace entries, and workgroup 0 adds
// the B*K row losses in a fixed order.  No atomics, and no sum depends on an order that could vary: the same bits on every run.
#include "loss_common.h"

#define WEAK_SLICE_VALUES 8192      // target values per label workgroup (32 per thread)
#define WEAK_MAX_SLICES 64          // per clip; sed_weak_bce_ws_bytes() sizes the partial maxima for it

namespace {

struct WeakParams {
    const float* pre;        // [B][t][K]
    const float* target;     // [B][K] (target_frames == 0) or [B][Tt][K]; NULL: pooling only
    float* clip_prob;        // [B][K] or NULL
    float* dpre;             // [B][t][K] or NULL
    float* loss;
    double* stats;           // workspace [B*K][4]: P, Q, the denominator (N, S1 or E), the winning row of max pooling
    float* ypart;            // workspace [B][nslice][K]: maxima of the strong target over each slice of frames
    int t, K, ratio, Tt, N, nrows;       // nrows = ceil(N / ratio): the rows of pre with c_i > 0
    int rows, nslice, slice_frames;      // rows = B*K; the first N target frames in nslice slices of slice_frames
    int target_frames, mode, accumulate;
    double wpos, coef, loss_scale;       // recall factor; weight * grad_scale / (B*K); weight / (B*K)
    const unsigned char* clip_sel;       // [B], nonzero: the clip takes part; NULL: all do, with coef and loss_scale as above
    int B, criterion;                    // SED_CRIT_BCE or SED_CRIT_MSE
    double wg, wt;                       // weight * grad_scale and weight: with clip_sel the mean is over S*K, S counted here
    size_t total;            // B*t*K
};

// maxima of one slice of a clip's strong target, for every class: thread = (frame offset fo, class kk), so that a wave reads
// consecutive floats of the [Tt][K] slab; classes beyond 256 take further passes
__device__ __forceinline__ void label_slice(const WeakParams& a, int b, int s, float* smf) {
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

__global__ __launch_bounds__(256) void weak_rows_kernel(const WeakParams a) {
    __shared__ double sm[256];
    __shared__ int smi[256];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= a.rows) {         // the label workgroups sit behind the row workgroups
        const int id = (int)blockIdx.x - a.rows;
        label_slice(a, id / a.nslice, id % a.nslice, reinterpret_cast<float*>(sm));
        return;
    }
    const int r = blockIdx.x, b = r / a.K, k = r - b * a.K;
    const float* __restrict__ x0 = a.pre + (size_t)b * a.t * a.K + k;

    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    float best = -INFINITY;
    int besti = 0x7fffffff;
    for (int i = tid; i < a.nrows; i += 256) {
        const float xf = x0[(size_t)i * a.K];
        if (a.mode == SED_POOL_MAX) {
            if (besti == 0x7fffffff || xf > best) { best = xf; besti = i; }      // ascending i: the first of equals stays
            continue;
        }
        const int left = a.N - i * a.ratio;
        const double c = (double)(left < a.ratio ? left : a.ratio);
        double p, q;
        sigmoids((double)xf, p, q);
        if (a.mode == SED_POOL_MEAN) {
            s0 += c * p;
            s1 += c * q;
        } else if (a.mode == SED_POOL_LINEAR) {
            s0 += c * p;
            s1 += c * p * p;
            s2 += c * p * q;
        } else {
            const double e = exp(p);
            s0 += c * e;
            s1 += c * p * e;
            s2 += c * q * e;
        }
    }

    double P, Q, den = 1.0;
    int jmax = 0;
    if (a.mode == SED_POOL_MAX) {
        // (value, index) pairs: larger value wins, equal values keep the smaller index -- the result does not depend on the order
        sm[tid] = (double)best;
        smi[tid] = besti;
        __syncthreads();
#pragma unroll
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) {
                const double v = sm[tid + s];
                const int j = smi[tid + s];
                if (j != 0x7fffffff && (smi[tid] == 0x7fffffff || v > sm[tid] || (v == sm[tid] && j < smi[tid]))) {
                    sm[tid] = v;
                    smi[tid] = j;
                }
            }
            __syncthreads();
        }
        sigmoids(sm[0], P, Q);
        jmax = smi[0];
    } else {
        s0 = block_sum(s0, sm);
        s1 = block_sum(s1, sm);
        if (a.mode == SED_POOL_MEAN) {
            den = (double)a.N;
            P = s0 / den;
            Q = s1 / den;
        } else {
            s2 = block_sum(s2, sm);
            den = s0;
            if (a.mode == SED_POOL_LINEAR && s0 == 0.0) {
                P = 0.0;
                Q = 1.0;
            } else {
                P = s1 / den;
                Q = s2 / den;
            }
        }
    }
    if (tid == 0) {
        if (a.clip_prob) a.clip_prob[r] = (float)P;
        if (a.stats) {
            double* __restrict__ st = a.stats + (size_t)r * 4;
            st[0] = P;
            st[1] = Q;
            st[2] = den;
            st[3] = (double)jmax;
        }
    }
}

// the clip label of row r = (b, k): given, or the maximum of the slices' maxima
__device__ __forceinline__ double clip_label(const WeakParams& a, int r, int b, int k) {
    if (a.target_frames == 0) return (double)a.target[r];
    const float* __restrict__ yp = a.ypart + (size_t)b * a.nslice * a.K + k;
    float m = yp[0];
    for (int s = 1; s < a.nslice; ++s) m = fmaxf(m, yp[(size_t)s * a.K]);
    return (double)m;
}

__global__ __launch_bounds__(256) void weak_grad_kernel(const WeakParams a) {
    __shared__ double sm[256];
    __shared__ int smi[256];
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    double coef = a.coef, loss_scale = a.loss_scale;
    if (a.clip_sel != nullptr) {             // the mean over the selected clips; S == 0: no loss, no gradient
        const int S = selected_count(a.clip_sel, a.B, smi);
        coef = S > 0 ? a.wg / ((double)S * (double)a.K) : 0.0;
        loss_scale = S > 0 ? a.wt / ((double)S * (double)a.K) : 0.0;
    }
    if (a.dpre != nullptr && idx < a.total) {
        const int k = (int)(idx % a.K);
        const size_t bt = idx / a.K;
        const int i = (int)(bt % a.t), b = (int)(bt / a.t), r = b * a.K + k;
        const bool off = a.clip_sel != nullptr && a.clip_sel[b] == 0;      // not selected: exactly 0, or what was there
        double v = 0.0;
        if (i < a.nrows && !off) {
            const double* __restrict__ st = a.stats + (size_t)r * 4;
            const double P = st[0], Q = st[1], den = st[2];
            const bool takes_part = a.mode == SED_POOL_MAX ? i == (int)st[3] : !(a.mode == SED_POOL_LINEAR && den == 0.0);
            if (takes_part) {
                const double Y = clip_label(a, r, b, k);
                const double g = a.criterion == SED_CRIT_MSE
                                     ? coef * (2.0 * (P - Y))
                                     : coef * (-a.wpos * Y / fmax(P, 1e-12) + (1.0 - Y) / fmax(Q, 1e-12));       // coef * dl/dP
                double p, q;
                sigmoids((double)a.pre[idx], p, q);
                const int left = a.N - i * a.ratio;
                const double c = (double)(left < a.ratio ? left : a.ratio);
                double dP;
                if (a.mode == SED_POOL_MAX) dP = 1.0;
                else if (a.mode == SED_POOL_MEAN) dP = c / den;
                else if (a.mode == SED_POOL_LINEAR) dP = c * (2.0 * p - P) / den;
                else dP = c * exp(p) * (1.0 + p - P) / den;
                v = g * dP * (p * q);
            }
        }
        if (!(off && a.accumulate)) a.dpre[idx] = a.accumulate ? a.dpre[idx] + (float)v : (float)v;
    }
    if (blockIdx.x != 0) return;
    double s = 0.0;
    for (int r = threadIdx.x; r < a.rows; r += 256) {
        if (a.clip_sel != nullptr && a.clip_sel[r / a.K] == 0) continue;
        const double P = a.stats[(size_t)r * 4], Q = a.stats[(size_t)r * 4 + 1];
        const double Y = clip_label(a, r, r / a.K, r % a.K);
        if (a.criterion == SED_CRIT_MSE) s += (P - Y) * (P - Y);
        else s -= a.wpos * Y * fmax(log(P), -100.0) + (1.0 - Y) * fmax(log(Q), -100.0);
    }
    s = block_sum(s, sm);
    if (threadIdx.x == 0) {
        const float v = (float)(s * loss_scale);
        a.loss[0] = a.accumulate ? a.loss[0] + v : v;
    }
}

// the size checks both entry points share; fills the geometry of p
static int weak_geometry(WeakParams& p, int B, int t, int K, int ratio, int Tt, int mode) {
    SED_REQUIRE(B > 0 && t > 0 && K > 0 && ratio > 0 && Tt > 0, "bad sizes");
    SED_REQUIRE(mode == SED_POOL_MAX || mode == SED_POOL_MEAN || mode == SED_POOL_LINEAR || mode == SED_POOL_EXP,
                "mode is SED_POOL_MAX, _MEAN, _LINEAR or _EXP");
    SED_REQUIRE((long long)B * K < (1ll << 24), "too many (clip, class) rows for one launch");
    SED_REQUIRE((long long)t * ratio < (1ll << 31), "t * ratio does not fit an int");
    p.t = t; p.K = K; p.ratio = ratio; p.Tt = Tt; p.mode = mode;
    p.rows = B * K;
    p.total = (size_t)B * t * K;
    p.N = t * ratio < Tt ? t * ratio : Tt;
    p.nrows = (p.N + ratio - 1) / ratio;
    return 0;
}

}   // namespace

extern "C" size_t sed_weak_bce_ws_bytes(int B, int t, int K) {
    (void)t;
    return B > 0 && K > 0 ? (size_t)B * K * (4 * sizeof(double) + WEAK_MAX_SLICES * sizeof(float)) : 0;
}

extern "C" int sed_clip_pool_fwd(const float* pre, float* clip_prob, int B, int t, int K, int ratio, int Tt, int mode, void* stream) {
    WeakParams p = {};
    if (int rc = weak_geometry(p, B, t, K, ratio, Tt, mode)) return rc;
    SED_REQUIRE(pre != nullptr && clip_prob != nullptr, "pre and clip_prob are needed (null)");
    p.pre = pre; p.clip_prob = clip_prob;
    weak_rows_kernel<<<(unsigned)p.rows, 256, 0, (hipStream_t)stream>>>(p);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_weak_bce_fwd_bwd_ex(const float* pre, const float* target, int target_frames, const unsigned char* clip_sel,
                                       int criterion, float* clip_prob, float* loss, float* dpre, int accumulate, int B, int t, int K,
                                       int ratio, int Tt, int mode, float recall_factor, float weight, float grad_scale,
                                       void* workspace, void* stream) {
    WeakParams p = {};
    SED_REQUIRE(criterion == SED_CRIT_BCE || criterion == SED_CRIT_MSE, "criterion is SED_CRIT_BCE or SED_CRIT_MSE");
    p.clip_sel = clip_sel; p.criterion = criterion;
    if (int rc = weak_geometry(p, B, t, K, ratio, Tt, mode)) return rc;
    SED_REQUIRE(target_frames == 0 || target_frames == Tt, "target_frames is 0 (clip labels [B][K]) or Tt (strong labels [B][Tt][K])");
    SED_REQUIRE(accumulate == 0 || accumulate == 1, "accumulate is 0 or 1");
    SED_REQUIRE(pre != nullptr && target != nullptr && loss != nullptr && workspace != nullptr,
                "pre, target, loss and workspace are needed (null)");
    SED_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "workspace must be 8-byte aligned");
    const size_t nblk = dpre != nullptr ? cdivz(p.total, 256) : 1;
    SED_REQUIRE(nblk < ((size_t)1 << 31), "too many logits for one launch");
    p.pre = pre; p.target = target; p.clip_prob = clip_prob; p.dpre = dpre; p.loss = loss;
    p.stats = static_cast<double*>(workspace);
    p.ypart = reinterpret_cast<float*>(p.stats + (size_t)p.rows * 4);
    p.target_frames = target_frames; p.accumulate = accumulate;
    p.wpos = (double)recall_factor;
    p.coef = (double)weight * (double)grad_scale / (double)p.rows;
    p.loss_scale = (double)weight / (double)p.rows;
    p.B = B;
    p.wg = (double)weight * (double)grad_scale;
    p.wt = (double)weight;
    if (target_frames != 0) {        // slices of about WEAK_SLICE_VALUES target values, none of them empty
        size_t ns = cdivz((size_t)p.N * K, WEAK_SLICE_VALUES);
        if (ns > WEAK_MAX_SLICES) ns = WEAK_MAX_SLICES;
        if (ns > (size_t)p.N) ns = (size_t)p.N;
        p.slice_frames = (p.N + (int)ns - 1) / (int)ns;
        p.nslice = (p.N + p.slice_frames - 1) / p.slice_frames;
    }
    hipStream_t st = (hipStream_t)stream;
    weak_rows_kernel<<<(unsigned)(p.rows + B * p.nslice), 256, 0, st>>>(p);
    SED_LAUNCH_CHECK();
    weak_grad_kernel<<<(unsigned)nblk, 256, 0, st>>>(p);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_weak_bce_fwd_bwd(const float* pre, const float* target, int target_frames, float* clip_prob, float* loss,
                                    float* dpre, int accumulate, int B, int t, int K, int ratio, int Tt, int mode,
                                    float recall_factor, float weight, float grad_scale, void* workspace, void* stream) {
    return sed_weak_bce_fwd_bwd_ex(pre, target, target_frames, nullptr, SED_CRIT_BCE, clip_prob, loss, dpre, accumulate, B, t, K, ratio, Tt,
                                   mode, recall_factor, weight, grad_scale, workspace, stream);
}
