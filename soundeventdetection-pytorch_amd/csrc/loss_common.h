// Device helpers the double-precision loss kernels share (sed_weak.hip, sed_semi.hip): workgroups of 256 threads, fixed-order LDS trees.
#pragma once
#include "common.h"

#include <math.h>

// fixed-order tree over the 256 threads' values; the total is valid in every thread
static __device__ __forceinline__ double block_sum(double v, double* sm) {
    const int tid = threadIdx.x;
    __syncthreads();                 // sm may still be read from the previous reduction
    sm[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sm[tid] += sm[tid + s];
        __syncthreads();
    }
    return sm[0];
}

static __device__ __forceinline__ void sigmoids(double x, double& p, double& q) {
    p = 1.0 / (1.0 + exp(-x));
    q = 1.0 / (1.0 + exp(x));
}

// S = the number of clips that take part: the nonzero bytes of clip_sel [B], or B for NULL; valid in every thread.
// smi: 256 ints of LDS.  An integer count: the same in any order.
static __device__ __forceinline__ int selected_count(const unsigned char* __restrict__ clip_sel, int B, int* smi) {
    if (clip_sel == nullptr) return B;
    const int tid = threadIdx.x;
    int c = 0;
    for (int b = tid; b < B; b += 256) c += clip_sel[b] != 0;
    __syncthreads();
    smi[tid] = c;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) smi[tid] += smi[tid + s];
        __syncthreads();
    }
    return smi[0];
}
