// The per-element Adam / AdamW arithmetic and the fixed fp64 LDS tree of the gradient norm, written once: sed_ops.hip (the flat
// step, host and device scalars) and sed_optim.hip (the grouped step) both compile these, so a tile of the grouped step and the
// same elements of the flat step run the same expressions.
#pragma once
#include "common.h"

// The decay terms are new arithmetic, and the files are compiled with -ffp-contract=fast: left to the compiler, gr + wd * p becomes
// fma(g, gse, wd * p) in the vectorised body and fma(wd, p, g * gse) in the scalar one, and the host and device forms disagree in
// the last bit of m.  rounded() hands a value through an empty asm, so it is an fp32 number of its own that nothing fuses across:
// the decay terms round where torch's do, in every form alike.  The WD 0 path does not use it.
__device__ __forceinline__ float rounded(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

//   WD 0: none   1: L2, gr += wd * p (torch.optim.Adam(weight_decay=))   2: decoupled, p *= 1 - lr * wd first (torch.optim.AdamW)
template <bool AMS, int WD>
__device__ __forceinline__ void adam_ex_elem(float& p, const float g, float& m, float& v, float& x, const float gse, const float wd,
                                             const float decay, const float one_minus_b1, const float b2, const float one_minus_b2,
                                             const float eps, const float step_size, const float inv_sqrt_bc2) {
    float gr = g * gse;
    if (WD == 1) gr = rounded(gr) + rounded(wd * p);                   // grad.add(param, alpha=wd): product and sum each rounded
    if (WD == 2) p = rounded(p * decay);                               // param.mul_(1 - lr * wd), rounded before the update
    m = m + one_minus_b1 * (gr - m);
    v = v * b2 + (one_minus_b2 * gr) * gr;
    if (AMS) x = fmaxf(x, v);
    const float denom = sqrtf(AMS ? x : v) * inv_sqrt_bc2 + eps;
    p = p - step_size * (m / denom);
}

__device__ __forceinline__ double block256_sum_f64(double t, double* sh) {
    sh[threadIdx.x] = t;
    __syncthreads();
#pragma unroll
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}
