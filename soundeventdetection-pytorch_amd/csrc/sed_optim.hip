// The grouped optimizer step: Adam / AdamW over a TILE TABLE of the flat buffers, every tile belonging to one parameter group with its
// own learning-rate scale, weight decay and frozen flag, and the learning rate following a warm-up + decay schedule that is evaluated
// on the DEVICE from the step counter -- so an eager step and a replayed graph of it run the same two kernels on the same scalars.
//   tiles  int32 [NT][4] = {start4, count4, group, 0}   units of 4 floats, 1 <= count4 <= SED_OPT_TILE4, ascending, disjoint,
//                                                       none across a parameter (FlatParams pads every start to 4 floats)
//   groups float [NG][4] = {lr_scale, weight_decay, frozen (0/1), 0}
// One workgroup of 256 threads per tile: the group's scalars are uniform loads, every access is 16 bytes, the grid is NT.
// The element arithmetic is adam_ex_elem (adam_common.h), the one sed_adam_step_ex / _dev run.
#include <math.h>

#include "adam_common.h"

namespace {

// lr(s) = base_lr * w(s) * d(s), all fp64; s is the 1-based step (train.py's lr_at is the same in Python)
__device__ double sched_lr(double base_lr, int kind, int warmup, int total, int every, double gamma, double floor_lr, long long s) {
    const double W = (double)warmup, S = (double)s;
    const double w = warmup > 0 ? fmin(1.0, S / W) : 1.0;
    double d = 1.0;
    if (kind == SED_SCHED_STEP) {
        d = pow(gamma, (double)((s - 1) / every));
    } else if (kind == SED_SCHED_COSINE || kind == SED_SCHED_LINEAR) {
        const double u = fmin(1.0, fmax(0.0, (S - W) / ((double)total - W)));
        const double shape = kind == SED_SCHED_COSINE ? 0.5 * (1.0 + cos(M_PI * u)) : 1.0 - u;
        d = floor_lr + (1.0 - floor_lr) * shape;
    } else if (kind == SED_SCHED_INVSQRT) {
        d = sqrt(fmax(W, 1.0) / fmax(fmax(S, W), 1.0));
    }
    return base_lr * w * d;
}

// one workgroup, one thread per group: advance the counter, evaluate the schedule, derive every group's two scalars
__global__ __launch_bounds__(64) void adam_groups_hyper_kernel(float* __restrict__ hyper, int* __restrict__ step,
                                                              const float* __restrict__ groups, int ng, float* __restrict__ gh,
                                                              double base_lr, int kind, int warmup, int total, int every,
                                                              double gamma, double floor_lr, float beta1, float beta2) {
    const long long s = (long long)*step + 1;
    __syncthreads();                                    // every thread has read the old counter before it is replaced
    const double lr = sched_lr(base_lr, kind, warmup, total, every, gamma, floor_lr, s);
    const double bc1 = 1.0 - pow((double)beta1, (double)s), bc2 = 1.0 - pow((double)beta2, (double)s);
    const int g = threadIdx.x;
    if (g == 0) {
        *step = (int)s;
        hyper[0] = (float)lr;
        hyper[1] = (float)(1.0 / sqrt(bc2));
        hyper[2] = (float)sched_lr(base_lr, kind, warmup, total, every, gamma, floor_lr, s + 1);
    }
    if (g < ng) {
        const double lrg = lr * (double)groups[4 * g + 0];
        f32x4 o = {(float)(lrg / bc1), (float)(1.0 - lrg * (double)groups[4 * g + 1]), 0.f, 0.f};
        reinterpret_cast<f32x4*>(gh)[g] = o;
    }
}

template <bool AMS, int WD>
__device__ __forceinline__ void adam_tile(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, float* __restrict__ vmax, size_t start4, int count4, float gse,
                                          float wd, float decay, float one_minus_b1, float b2, float one_minus_b2, float eps,
                                          float step_size, float inv_sqrt_bc2) {
    for (int k = threadIdx.x; k < count4; k += 256) {
        const size_t i = start4 + (size_t)k;
        f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
        f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
        f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
        f32x4 xv = {0.f, 0.f, 0.f, 0.f};
        if (AMS) xv = reinterpret_cast<f32x4*>(vmax)[i];
        // One element at a time, the loop kept rolled: the file is compiled with -ffp-contract=fast, and which products the compiler
        // fuses depends on what surrounds them.  Unrolled, the four elements are packed across (v_pk_*) and v comes out as
        // fma(v, b2, (omb2 gr) gr), the host-scalar kernel's form; rolled, an element is compiled as adam_ex_dev_kernel's scalar body
        // is -- the two products of v rounded, then added -- and the bits are those of sed_adam_step_ex_dev, the step this one
        // replaces under a graph.  The selects that pick lane e cost VALU the kernel has to spare: it waits on memory.
#pragma clang loop unroll(disable)
        for (int e = 0; e < 4; ++e) {
            float pe = pv[e], me = mv[e], ve = vv[e], xe = xv[e];
            adam_ex_elem<AMS, WD>(pe, gv[e], me, ve, xe, gse, wd, decay, one_minus_b1, b2, one_minus_b2, eps, step_size,
                                  inv_sqrt_bc2);
            pv[e] = pe; mv[e] = me; vv[e] = ve; xv[e] = xe;
        }
        reinterpret_cast<f32x4*>(p)[i] = pv;
        reinterpret_cast<f32x4*>(m)[i] = mv;
        reinterpret_cast<f32x4*>(v)[i] = vv;
        if (AMS) reinterpret_cast<f32x4*>(vmax)[i] = xv;
    }
}

// A tile's extent clipped to the buffer and to SED_OPT_TILE4: the table is the caller's (sed_hip.h states the precondition), but a
// damaged one must not send a store outside the flat buffers.
__device__ __forceinline__ int tile_count(const int* __restrict__ tile, size_t n4) {
    const int s = tile[0], c = tile[1];
    if (s < 0 || c < 1 || (size_t)s >= n4) return 0;
    const size_t room = n4 - (size_t)s;
    const int cc = c > SED_OPT_TILE4 ? SED_OPT_TILE4 : c;
    return (size_t)cc > room ? (int)room : cc;
}

template <bool AMS>
__global__ __launch_bounds__(256) void adam_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, float* __restrict__ vmax, size_t n4,
                                                          const int* __restrict__ tiles, const float* __restrict__ groups, int ng,
                                                          const float* __restrict__ gh, const float* __restrict__ hyper,
                                                          float one_minus_b1, float b2, float one_minus_b2, float eps,
                                                          float grad_scale, int decoupled, const float* __restrict__ coef) {
    const int* tile = tiles + 4 * (size_t)blockIdx.x;
    const int grp = tile[2];
    if (grp < 0 || grp >= ng) return;
    const float wd = groups[4 * grp + 1];
    if (groups[4 * grp + 2] != 0.f) return;             // frozen: p, m, v, vmax keep their bits whatever g holds
    const int count4 = tile_count(tile, n4);
    const size_t start4 = (size_t)tile[0];
    const float step_size = gh[4 * grp + 0], decay = gh[4 * grp + 1], inv_sqrt_bc2 = hyper[1];
    const float gse = coef ? grad_scale * coef[0] : grad_scale;
    if (wd == 0.f)
        adam_tile<AMS, 0>(p, g, m, v, vmax, start4, count4, gse, wd, 1.0f, one_minus_b1, b2, one_minus_b2, eps, step_size, inv_sqrt_bc2);
    else if (decoupled)
        adam_tile<AMS, 2>(p, g, m, v, vmax, start4, count4, gse, wd, decay, one_minus_b1, b2, one_minus_b2, eps, step_size, inv_sqrt_bc2);
    else
        adam_tile<AMS, 1>(p, g, m, v, vmax, start4, count4, gse, wd, decay, one_minus_b1, b2, one_minus_b2, eps, step_size, inv_sqrt_bc2);
}

// ---- the gradient norm over the tiles of the non-frozen groups: one fp64 partial per tile through block256_sum_f64, then one workgroup
__global__ __launch_bounds__(256) void grad_sqsum_groups_kernel(const float* __restrict__ g, size_t n4, const int* __restrict__ tiles,
                                                                const float* __restrict__ groups, int ng, float grad_scale,
                                                                double* __restrict__ partial) {
    __shared__ double sh[256];
    const int* tile = tiles + 4 * (size_t)blockIdx.x;
    const int grp = tile[2];
    if (grp < 0 || grp >= ng || groups[4 * grp + 2] != 0.f) {   // a frozen parameter has no gradient: clip_grad_norm_ does not see it
        if (threadIdx.x == 0) partial[blockIdx.x] = 0.0;
        return;
    }
    const int count4 = tile_count(tile, n4);
    const size_t start4 = (size_t)tile[0];
    double t = 0.0;
    for (int k = threadIdx.x; k < count4; k += 256) {
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[start4 + (size_t)k];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double x = (double)(gv[e] * grad_scale);             // the fp32 value the optimizer sees
            t += x * x;
        }
    }
    t = block256_sum_f64(t, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// out[0] = norm, out[1] = clip factor: sed_grad_norm's protocol
__global__ __launch_bounds__(256) void grad_norm_groups_final_kernel(const double* __restrict__ partial, int nparts, float max_norm,
                                                                     float* __restrict__ out) {
    __shared__ double sh[256];
    double t = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) t += partial[i];
    t = block256_sum_f64(t, sh);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(t);
        float coef = 1.0f;
        if (max_norm > 0.0f) {
            const float c = max_norm / (norm + 1e-6f);                 // fp32, a NaN stays a NaN like torch.clamp's
            coef = c > 1.0f ? 1.0f : c;
        }
        out[0] = norm;
        out[1] = coef;
    }
}

}  // namespace

extern "C" int sed_opt_tile4(void) { return SED_OPT_TILE4; }

extern "C" int sed_adam_groups_step(float* p, const float* g, float* m, float* v, float* vmax, size_t n, const int* tiles, int nt,
                                    const float* groups, int ng, float* gh, float* hyper, int* step, double base_lr, int sched_kind,
                                    int warmup, int total, int every, double gamma, double floor_lr, float beta1, float beta2,
                                    float eps, float grad_scale, int decoupled, const float* coef, void* stream) {
    SED_REQUIRE(p && g && m && v && tiles && groups && gh && hyper && step, "null argument");
    SED_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vmax | (uintptr_t)tiles |
                  (uintptr_t)groups | (uintptr_t)gh) & 15) == 0, "flat buffers and tables must be 16-byte aligned");
    SED_REQUIRE(n >= 4 && n % 4 == 0, "n must be a positive multiple of 4 (every parameter start is padded to 4 floats)");
    SED_REQUIRE(nt >= 1, "nt must be >= 1");
    SED_REQUIRE(ng >= 1 && ng <= SED_OPT_MAX_GROUPS, "ng must lie in 1..64");
    SED_REQUIRE(sched_kind >= SED_SCHED_CONST && sched_kind <= SED_SCHED_INVSQRT, "unknown schedule kind");
    SED_REQUIRE(warmup >= 0, "warmup must be >= 0");
    SED_REQUIRE((sched_kind != SED_SCHED_COSINE && sched_kind != SED_SCHED_LINEAR) || total > warmup,
                "cosine and linear need total > warmup");
    SED_REQUIRE(sched_kind != SED_SCHED_STEP || every >= 1, "step needs every >= 1");
    SED_REQUIRE(floor_lr >= 0.0 && floor_lr <= 1.0, "floor must lie in [0, 1]");
    SED_REQUIRE(gamma > 0.0 && gamma < (double)INFINITY, "gamma must be finite and > 0");
    SED_REQUIRE(base_lr == base_lr && base_lr > -(double)INFINITY && base_lr < (double)INFINITY, "base_lr must be finite");
    hipStream_t st = (hipStream_t)stream;
    adam_groups_hyper_kernel<<<1, 64, 0, st>>>(hyper, step, groups, ng, gh, base_lr, sched_kind, warmup, total, every, gamma, floor_lr,
                                               beta1, beta2);
    SED_LAUNCH_CHECK();
    const float omb1 = (float)(1.0 - (double)beta1), omb2 = (float)(1.0 - (double)beta2);
    if (vmax)
        adam_groups_kernel<true><<<nt, 256, 0, st>>>(p, g, m, v, vmax, n >> 2, tiles, groups, ng, gh, hyper, omb1, beta2, omb2, eps,
                                                     grad_scale, decoupled, coef);
    else
        adam_groups_kernel<false><<<nt, 256, 0, st>>>(p, g, m, v, vmax, n >> 2, tiles, groups, ng, gh, hyper, omb1, beta2, omb2, eps,
                                                      grad_scale, decoupled, coef);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_grad_norm_groups(const float* g, size_t n, const int* tiles, int nt, const float* groups, float grad_scale,
                                    float max_norm, double* partial, float* out, void* stream) {
    SED_REQUIRE(g && tiles && groups && partial && out, "null argument");
    SED_REQUIRE((((uintptr_t)g | (uintptr_t)tiles | (uintptr_t)groups) & 15) == 0, "flat buffer and tables must be 16-byte aligned");
    SED_REQUIRE((((uintptr_t)partial) & 7) == 0, "partial must be 8-byte aligned");
    SED_REQUIRE(n >= 4 && n % 4 == 0, "n must be a positive multiple of 4 (every parameter start is padded to 4 floats)");
    SED_REQUIRE(nt >= 1, "nt must be >= 1");
    hipStream_t st = (hipStream_t)stream;
    grad_sqsum_groups_kernel<<<nt, 256, 0, st>>>(g, n >> 2, tiles, groups, SED_OPT_MAX_GROUPS, grad_scale, partial);
    SED_LAUNCH_CHECK();
    grad_norm_groups_final_kernel<<<1, 256, 0, st>>>(partial, nt, max_norm, out);
    SED_LAUNCH_CHECK();
    return 0;
}
