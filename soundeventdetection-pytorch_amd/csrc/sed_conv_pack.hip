// Weight packing and weight-gradient slab reduction for the 3x3 convolution kernels (gfx950).
//
// The reference keeps nn.Conv2d weights as [Cout][Cin][3][3] (ConvBlock, models/spectogram_models.py:132-140 of the reference) and
// autograd returns their gradient in the same layout.  The MFMA kernels read the operator as [chunk][tap][32/KR][Coutp][KR]
// (sed_conv.hip) -- transposed and tap-flipped for the data gradient, as two 16-bit images for the split-operand dtypes
// (sed_conv_x3.hip) -- and leave the weight gradient as one [9][Cinp][Coutp] slab per workgroup.  This file holds the pack / unpack
// kernels, the fixed-order slab reduction and their entry points.
#include "conv_common.h"

// =================================================================================================
// weight packing
// =================================================================================================
template <typename T>
__global__ void pack_weight_kernel(const float* __restrict__ w, T* __restrict__ out, int Cout, int Cin,
                                   int POp, int PIp, int tf) {
    constexpr int KR = EL<T>::KR;
    const size_t total = (size_t)PIp * 9 * POp;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * blockDim.x) {
        // idx = (((chunk*9 + tap)*(32/KR) + kq)*POp + po)*KR + kr
        size_t t = idx;
        const int kr = t % KR; t /= KR;
        const int po = t % POp; t /= POp;
        const int kq = t % (32 / KR); t /= (32 / KR);
        const int tap = t % 9;
        const int chunk = t / 9;
        const int pi = chunk * 32 + kq * KR + kr;
        float v = 0.f;
        if (!tf) {
            if (po < Cout && pi < Cin) v = w[((size_t)po * Cin + pi) * 9 + tap];
        } else {  // packed-out = conv Cin, packed-in = conv Cout, taps flipped
            if (po < Cin && pi < Cout) v = w[((size_t)pi * Cin + po) * 9 + (8 - tap)];
        }
        out[idx] = from_f<T>(v);
    }
}

// One launch for every conv layer of a step (forward and data-gradient operators): desc[i] = {w, out, Cout, Cin, POp, PIp,
// tf, first_block} as eight 64-bit words; block b serves 1024 elements of the descriptor whose block range holds b.
template <typename T>
__global__ __launch_bounds__(256) void pack_weight_batch_kernel(const long long* __restrict__ desc, int n) {
    constexpr int KR = EL<T>::KR;
    int d = 0;
    for (int i = 1; i < n; ++i)
        if ((int)desc[i * 8 + 7] <= (int)blockIdx.x) d = i;
    const long long* e = desc + d * 8;
    const float* __restrict__ w = reinterpret_cast<const float*>(e[0]);
    T* __restrict__ out = reinterpret_cast<T*>(e[1]);
    const int Cout = (int)e[2], Cin = (int)e[3], POp = (int)e[4], PIp = (int)e[5], tf = (int)e[6];
    const size_t total = (size_t)PIp * 9 * POp;
    const size_t base = (size_t)((int)blockIdx.x - (int)e[7]) * 1024;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const size_t idx = base + u * 256 + threadIdx.x;
        if (idx >= total) break;
        size_t t = idx;
        const int kr = t % KR; t /= KR;
        const int po = t % POp; t /= POp;
        const int kq = t % (32 / KR); t /= (32 / KR);
        const int tap = t % 9;
        const int chunk = t / 9;
        const int pi = chunk * 32 + kq * KR + kr;
        float v = 0.f;
        if (!tf) {
            if (po < Cout && pi < Cin) v = w[((size_t)po * Cin + pi) * 9 + tap];
        } else {
            if (po < Cin && pi < Cout) v = w[((size_t)pi * Cin + po) * 9 + (8 - tap)];
        }
        out[idx] = from_f<T>(v);
    }
}

// dtype SED_F32X3: the operator as two bf16 images in the bf16 layout, [hi = bf16(w)][lo = bf16(w - hi)] (sed_conv_x3.hip)
typedef _Float16 sed_half_t;
__device__ __forceinline__ void x3_pieces(float v, int half, unsigned short& hi, unsigned short& lo) {
    if (half) {                 // fp16 pieces, lo scaled by 2^11 (sed_conv_x3.hip)
        const sed_half_t h = (sed_half_t)v;
        const sed_half_t l = (sed_half_t)((v - (float)h) * 2048.f);
        hi = __builtin_bit_cast(unsigned short, h);
        lo = __builtin_bit_cast(unsigned short, l);
    } else {
        const bf16_t h = (bf16_t)v;
        const bf16_t l = (bf16_t)(v - (float)h);
        hi = __builtin_bit_cast(unsigned short, h);
        lo = __builtin_bit_cast(unsigned short, l);
    }
}
__global__ void pack_weight_x3_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, int Cout, int Cin, int POp, int PIp, int tf,
                                      int half) {
    const size_t total = (size_t)PIp * 9 * POp;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        size_t t = idx;
        const int kr = t % 8; t /= 8;
        const int po = t % POp; t /= POp;
        const int kq = t % 4; t /= 4;
        const int tap = t % 9;
        const int chunk = t / 9;
        const int pi = chunk * 32 + kq * 8 + kr;
        float v = 0.f;
        if (!tf) {
            if (po < Cout && pi < Cin) v = w[((size_t)po * Cin + pi) * 9 + tap];
        } else {
            if (po < Cin && pi < Cout) v = w[((size_t)pi * Cin + po) * 9 + (8 - tap)];
        }
        x3_pieces(v, half, out[idx], out[total + idx]);
    }
}
__global__ __launch_bounds__(256) void pack_weight_batch_x3_kernel(const long long* __restrict__ desc, int n, int half) {
    int d = 0;
    for (int i = 1; i < n; ++i)
        if ((int)desc[i * 8 + 7] <= (int)blockIdx.x) d = i;
    const long long* e = desc + d * 8;
    const float* __restrict__ w = reinterpret_cast<const float*>(e[0]);
    unsigned short* __restrict__ out = reinterpret_cast<unsigned short*>(e[1]);
    const int Cout = (int)e[2], Cin = (int)e[3], POp = (int)e[4], PIp = (int)e[5], tf = (int)e[6];
    const size_t total = (size_t)PIp * 9 * POp;
    const size_t base = (size_t)((int)blockIdx.x - (int)e[7]) * 1024;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const size_t idx = base + u * 256 + threadIdx.x;
        if (idx >= total) break;
        size_t t = idx;
        const int kr = t % 8; t /= 8;
        const int po = t % POp; t /= POp;
        const int kq = t % 4; t /= 4;
        const int tap = t % 9;
        const int chunk = t / 9;
        const int pi = chunk * 32 + kq * 8 + kr;
        float v = 0.f;
        if (!tf) {
            if (po < Cout && pi < Cin) v = w[((size_t)po * Cin + pi) * 9 + tap];
        } else {
            if (po < Cin && pi < Cout) v = w[((size_t)pi * Cin + po) * 9 + (8 - tap)];
        }
        x3_pieces(v, half, out[idx], out[total + idx]);
    }
}

__global__ void unpack_wgrad_kernel(const float* __restrict__ dwp, float* __restrict__ dw, int Cout, int Cin,
                                    int Coutp, int Cinp) {
    const int total = Cout * Cin * 9;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int tap = idx % 9;
        const int ci = (idx / 9) % Cin;
        const int co = idx / (9 * Cin);
        dw[idx] = dwp[((size_t)tap * Cinp + ci) * Coutp + co];
    }
}

// out[i] = sum_s ws[s][i]: a 1024-thread workgroup owns 64 consecutive outputs; its 16 waves each walk
// every 16th strip (coalesced 256-byte rows, 8 loads in flight), then a fixed-order LDS reduction.
__global__ __launch_bounds__(1024) void wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out,
                                                            int strips, size_t n, float* __restrict__ dw = nullptr, int Cout = 0,
                                                            int Cin = 0, int Cinp = 0, int Coutp = 0) {
    __shared__ float red[16][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t i = (size_t)blockIdx.x * 64 + lane;
    float t = 0.f;
    if (i < n) {
        int sidx = wv;
        for (; sidx + 16 * 7 < strips; sidx += 16 * 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = ws[(size_t)(sidx + 16 * u) * n + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) t += v[u];
        }
        for (; sidx < strips; sidx += 16) t += ws[(size_t)sidx * n + i];
    }
    red[wv][lane] = t;
    __syncthreads();
    if (wv == 0 && i < n) {
        float tot = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) tot += red[k][lane];
        out[i] = tot;
        if (dw != nullptr) {          // the same value in torch's [Cout][Cin][3][3] layout (what sed_unpack_conv_wgrad writes)
            const int co = (int)(i % Coutp), ci = (int)((i / Coutp) % Cinp), tap = (int)(i / ((size_t)Coutp * Cinp));
            if (co < Cout && ci < Cin) dw[((size_t)co * Cin + ci) * 9 + tap] = tot;
        }
    }
}

int reduce_wgrad_slabs(const float* ws, float* dwpack, int slabs, size_t n, float* dw, int Cout, int Cin, int Cinp, int Coutp, hipStream_t st) {
    wgrad_reduce_kernel<<<cdiv(n, 64), 1024, 0, st>>>(ws, dwpack, slabs, n, dw, Cout, Cin, Cinp, Coutp);
    return 0;
}

// =================================================================================================
// host launchers (C ABI)
// =================================================================================================

extern "C" int sed_pack_conv_weight(int dtype, const float* w, void* wpack, int Cout, int Cin, int Coutp,
                                    int Cinp, int transpose_flip, void* stream) {
    SED_REQUIRE(Coutp % 32 == 0 && Cinp % 32 == 0 && Coutp >= Cout && Cinp >= Cin, "padded channels must be multiples of 32");
    hipStream_t st = (hipStream_t)stream;
    // packed-out / packed-in padded sizes
    const int POp = transpose_flip ? Cinp : Coutp, PIp = transpose_flip ? Coutp : Cinp;
    const size_t total = (size_t)PIp * 9 * POp;
    const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    if (dtype == SED_BF16)
        pack_weight_kernel<bf16_t><<<grid, 256, 0, st>>>(w, (bf16_t*)wpack, Cout, Cin, POp, PIp, transpose_flip);
    else if (dtype == SED_F32)
        pack_weight_kernel<float><<<grid, 256, 0, st>>>(w, (float*)wpack, Cout, Cin, POp, PIp, transpose_flip);
    else if (dtype == SED_F32X3 || dtype == SED_F32H3)
        pack_weight_x3_kernel<<<grid, 256, 0, st>>>(w, (unsigned short*)wpack, Cout, Cin, POp, PIp, transpose_flip, dtype == SED_F32H3);
    else
        SED_REQUIRE(false, "bad dtype");
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_unpack_conv_wgrad(const float* dwpack, float* dw, int Cout, int Cin, int Coutp, int Cinp,
                                     void* stream) {
    const int total = Cout * Cin * 9;
    unpack_wgrad_kernel<<<cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(dwpack, dw, Cout, Cin, Coutp, Cinp);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_pack_conv_weights_batch(int dtype, const void* desc, int n, int total_blocks, void* stream) {
    SED_REQUIRE(desc && n > 0 && n <= 64 && total_blocks > 0, "descriptor table");
    if (dtype == SED_BF16)
        pack_weight_batch_kernel<bf16_t><<<total_blocks, 256, 0, (hipStream_t)stream>>>((const long long*)desc, n);
    else if (dtype == SED_F32)
        pack_weight_batch_kernel<float><<<total_blocks, 256, 0, (hipStream_t)stream>>>((const long long*)desc, n);
    else if (dtype == SED_F32X3 || dtype == SED_F32H3)
        pack_weight_batch_x3_kernel<<<total_blocks, 256, 0, (hipStream_t)stream>>>((const long long*)desc, n, dtype == SED_F32H3);
    else
        SED_REQUIRE(false, "bad dtype");
    SED_LAUNCH_CHECK();
    return 0;
}
