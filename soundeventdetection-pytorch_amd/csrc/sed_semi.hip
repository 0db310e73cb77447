// Semi-supervised training (the DCASE task-4 baseline's recipe): batches that mix strongly labelled, weakly labelled and unlabelled
// clips, and a mean teacher.  Three pieces live here; the fourth, the clip-level loss with a clip selection and an MSE criterion, is
// sed_weak_bce_fwd_bwd_ex in sed_weak.hip.
//   sed_bce_sel_fwd_bwd    the strong recall-weighted BCE over the selected clips only
//   sed_frame_mse_fwd_bwd  frame-level consistency: MSE between the student's and the teacher's frame probabilities
//   sed_ema_update         teacher <- alpha * teacher + (1 - alpha) * student over a flat fp32 buffer
// The two losses work on the pre-interpolation logits pre [B][t][K] like sed_bce_fwd_bwd: with N = min(t*ratio, Tt) virtual frames,
// row i stands for the frames [i*ratio, i*ratio + c_i), c_i = clamp(N - i*ratio, 0, ratio).  clip_sel [B] (bytes, nonzero = the clip
// takes part, NULL = all) selects S clips; S is counted on the device.  Everything in double, p = 1/(1+e^-x) and q = 1/(1+e^x) each
// from its own expression, every result rounded once to fp32:
//   BCE   l_f = -(w y_f ln sigma(x) + (1 - y_f) ln sigma(-x)),  ln sigma(x) = min(x, 0) - log1p(e^-|x|)   (no -100 clamp)
//         loss = weight * sum_{b in sel} sum_{f < N} sum_k l_f / (S N K)
//         dpre[b,i,k] = weight * grad_scale / (S N K) * sum_{f of row i, f < N} ((1 - y_f) p - w y_f q)
//   MSE   loss = weight * sum_{b in sel} sum_i c_i sum_k (p - p_T)^2 / (S N K)
//         dpre[b,i,k] = weight * grad_scale / (S N K) * c_i * 2 (p - p_T) p q          (the teacher gets no gradient)
// (tests/semi_formula.py is the same in numpy).  Cells of unselected clips and of rows with c_i = 0 are written as exact 0, or left as
// they are under accumulate = 1; S = 0 gives loss term 0 and gradient 0.
//
// Shape: a few hundred thousand logits, latency-bound, two launches like sed_weak.hip.  Here the gradient of a logit needs no
// reduction result, so the first launch -- one thread per logit -- writes dpre and leaves its workgroup's loss sum (a fixed LDS
// tree) in the workspace, and the second, one workgroup, adds the partial sums in a fixed order.  No atomics: the same bits on every run.
#include "loss_common.h"

namespace {

struct SemiParams {
    const float* pre;                 // [B][t][K]
    const float* other;               // BCE: target [B][Tt][K]; MSE: the teacher's logits [B][t][K]
    const unsigned char* clip_sel;    // [B] or NULL
    float* dpre;                      // [B][t][K] or NULL
    float* loss;
    double* partial;                  // workspace [nblk]
    int B, t, K, ratio, Tt, N, accumulate;
    unsigned nblk;
    double wpos, wg, wt;              // recall factor; weight * grad_scale; weight
    size_t total;                     // B*t*K
};

// 1 / (S N K) times scale, 0 when nothing is selected
__device__ __forceinline__ double mean_factor(double scale, int S, const SemiParams& a) {
    return S > 0 ? scale / ((double)S * (double)a.N * (double)a.K) : 0.0;
}

template <bool MSE>
__global__ __launch_bounds__(256) void semi_elem_kernel(const SemiParams a) {
    __shared__ double sm[256];
    __shared__ int smi[256];
    const double coef = mean_factor(a.wg, selected_count(a.clip_sel, a.B, smi), a);
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    double lsum = 0.0;
    if (idx < a.total) {
        const int k = (int)(idx % a.K);
        const size_t bt = idx / a.K;
        const int i = (int)(bt % a.t), b = (int)(bt / a.t);
        const long long left = (long long)a.N - (long long)i * a.ratio;
        const int c = left <= 0 ? 0 : left < a.ratio ? (int)left : a.ratio;
        const bool on = c > 0 && (a.clip_sel == nullptr || a.clip_sel[b] != 0);
        double g = 0.0;
        if (on) {
            const double x = (double)a.pre[idx];
            double p, q;
            sigmoids(x, p, q);
            if (MSE) {
                const double pT = 1.0 / (1.0 + exp(-(double)a.other[idx]));
                const double d = p - pT;
                lsum = (double)c * (d * d);
                g = (double)c * (2.0 * d) * (p * q);
            } else {
                const double tail = log1p(exp(-fabs(x)));
                const double lsp = fmin(x, 0.0) - tail, lsn = fmin(-x, 0.0) - tail;
                const float* __restrict__ y0 = a.other + ((size_t)b * a.Tt + (size_t)i * a.ratio) * a.K + k;
                for (int j = 0; j < c; ++j) {
                    const double y = (double)y0[(size_t)j * a.K];
                    lsum -= a.wpos * y * lsp + (1.0 - y) * lsn;
                    g += (1.0 - y) * p - a.wpos * y * q;
                }
            }
        }
        if (a.dpre != nullptr && (on || !a.accumulate)) {
            const float v = (float)(coef * g);
            a.dpre[idx] = a.accumulate ? a.dpre[idx] + v : v;
        }
    }
    lsum = block_sum(lsum, sm);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = lsum;
}

__global__ __launch_bounds__(256) void semi_finalize_kernel(const SemiParams a) {
    __shared__ double sm[256];
    __shared__ int smi[256];
    const double scale = mean_factor(a.wt, selected_count(a.clip_sel, a.B, smi), a);
    double s = 0.0;
    for (unsigned i = threadIdx.x; i < a.nblk; i += 256) s += a.partial[i];
    s = block_sum(s, sm);
    if (threadIdx.x == 0) {
        const float v = (float)(s * scale);
        a.loss[0] = a.accumulate ? a.loss[0] + v : v;
    }
}

// the checks and the geometry both losses share
static int semi_setup(SemiParams& p, const float* pre, const float* other, const unsigned char* clip_sel, float* loss, float* dpre,
                      int accumulate, int B, int t, int K, int ratio, int Tt, float weight, float grad_scale, void* workspace) {
    SED_REQUIRE(B > 0 && t > 0 && K > 0 && ratio > 0 && Tt > 0, "bad sizes");
    SED_REQUIRE((long long)t * ratio < (1ll << 31), "t * ratio does not fit an int");
    SED_REQUIRE(accumulate == 0 || accumulate == 1, "accumulate is 0 or 1");
    SED_REQUIRE(pre != nullptr && other != nullptr && loss != nullptr && workspace != nullptr,
                "the logits, the target or teacher logits, loss and workspace are needed (null)");
    SED_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "workspace must be 8-byte aligned");
    p.total = (size_t)B * t * K;
    const size_t nblk = cdivz(p.total, 256);
    SED_REQUIRE(nblk < ((size_t)1 << 31), "too many logits for one launch");
    p.pre = pre; p.other = other; p.clip_sel = clip_sel; p.dpre = dpre; p.loss = loss;
    p.partial = static_cast<double*>(workspace);
    p.B = B; p.t = t; p.K = K; p.ratio = ratio; p.Tt = Tt; p.accumulate = accumulate;
    p.N = t * ratio < Tt ? t * ratio : Tt;
    p.nblk = (unsigned)nblk;
    p.wg = (double)weight * (double)grad_scale;
    p.wt = (double)weight;
    return 0;
}

static size_t semi_ws_bytes(int B, int t, int K) {
    return B > 0 && t > 0 && K > 0 ? cdivz((size_t)B * t * K, 256) * sizeof(double) : 0;
}

// alpha = 0 and alpha = 1 hand the student's and the teacher's value through as they are: 0 * t + s would turn an infinite t into NaN
// and a student's -0 into +0
__device__ __forceinline__ float ema_value(float t, float s, double alpha, double beta) {
    if (alpha == 0.0) return s;
    if (alpha == 1.0) return t;
    return (float)(alpha * (double)t + beta * (double)s);
}

__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ teacher, const float* __restrict__ student, size_t head,
                                                  size_t nvec, size_t nedge, double alpha, double beta) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nvec) {                  // the 16-byte aligned body
        f32x4* tp = reinterpret_cast<f32x4*>(teacher + head) + i;
        const f32x4 s = reinterpret_cast<const f32x4*>(student + head)[i];
        f32x4 v = *tp;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ema_value(v[j], s[j], alpha, beta);
        *tp = v;
        return;
    }
    size_t e = i - nvec;             // the elements before and after it
    if (e >= nedge) return;
    if (e >= head) e += nvec * 4;
    teacher[e] = ema_value(teacher[e], student[e], alpha, beta);
}

}   // namespace

extern "C" size_t sed_bce_sel_ws_bytes(int B, int t, int K) { return semi_ws_bytes(B, t, K); }

extern "C" int sed_bce_sel_fwd_bwd(const float* pre, const float* target, const unsigned char* clip_sel, float* loss, float* dpre,
                                   int accumulate, int B, int t, int K, int ratio, int Tt, float recall_factor, float weight,
                                   float grad_scale, void* workspace, void* stream) {
    SemiParams p = {};
    if (int rc = semi_setup(p, pre, target, clip_sel, loss, dpre, accumulate, B, t, K, ratio, Tt, weight, grad_scale, workspace)) return rc;
    p.wpos = (double)recall_factor;
    hipStream_t st = (hipStream_t)stream;
    semi_elem_kernel<false><<<p.nblk, 256, 0, st>>>(p);
    SED_LAUNCH_CHECK();
    semi_finalize_kernel<<<1, 256, 0, st>>>(p);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t sed_frame_mse_ws_bytes(int B, int t, int K) { return semi_ws_bytes(B, t, K); }

extern "C" int sed_frame_mse_fwd_bwd(const float* pre, const float* pre_teacher, const unsigned char* clip_sel, float* loss, float* dpre,
                                     int accumulate, int B, int t, int K, int ratio, int Tt, float weight, float grad_scale,
                                     void* workspace, void* stream) {
    SemiParams p = {};
    if (int rc = semi_setup(p, pre, pre_teacher, clip_sel, loss, dpre, accumulate, B, t, K, ratio, Tt, weight, grad_scale, workspace))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    semi_elem_kernel<true><<<p.nblk, 256, 0, st>>>(p);
    SED_LAUNCH_CHECK();
    semi_finalize_kernel<<<1, 256, 0, st>>>(p);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_ema_update(float* teacher, const float* student, size_t n, double alpha, void* stream) {
    SED_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "alpha lies in [0, 1]");
    SED_REQUIRE(teacher != nullptr && student != nullptr && n >= 1, "teacher, student and n >= 1 are needed");
    const uintptr_t ta = reinterpret_cast<uintptr_t>(teacher), sa = reinterpret_cast<uintptr_t>(student);
    SED_REQUIRE((ta & 3) == 0 && (sa & 3) == 0, "the buffers must be 4-byte aligned");
    // float4 accesses where both pointers reach a 16-byte boundary after the same number of elements; element-wise otherwise
    size_t head = n, nvec = 0;
    if (((ta ^ sa) & 15) == 0) {
        head = ((16 - (ta & 15)) & 15) / 4;
        if (head > n) head = n;
        nvec = (n - head) / 4;
    }
    const size_t nedge = n - nvec * 4, nblk = cdivz(nvec + nedge, 256);
    SED_REQUIRE(nblk < ((size_t)1 << 31), "too many elements for one launch");
    ema_kernel<<<(unsigned)nblk, 256, 0, (hipStream_t)stream>>>(teacher, student, head, nvec, nedge, alpha, 1.0 - alpha);
    SED_LAUNCH_CHECK();
    return 0;
}
