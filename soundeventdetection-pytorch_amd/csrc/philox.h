// Counter-based dropout masks: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the one mask
// definition that every fused kernel, sed_dropout_mask and tests/dropout_formula.py share.
//
//   state   rng[4] = (seed_lo, seed_hi, step, 0), uint32 in DEVICE memory: the kernels load it, so a captured graph sees the step word
//           that its own add advanced
//   key     (seed_lo, seed_hi ^ stream),  stream = 8 * layer + site
//   sites   0 attention probabilities, 1 attention output before its residual add, 2 convolution module output before its residual
//           add, 3 FFN hidden activation, 4 FFN output before its residual add
//   rows    [R][N], element (r, c):            counter (c >> 2, r mod 2^32, r >> 32, step), output word c & 3
//   attn    clip b, head g, query i, key j:    counter (j >> 2, i, b * H + g, step),        output word j & 3
//   keep    iff word >= thr, thr = min(2^32 - 1, floor(p * 2^32 + 1/2)) (host, double); a kept value is multiplied in fp32 by
//           s = (float)(1 / (1 - (double)p)).  p = 0: thr = 0, every cell kept, s = 1.
// Plain C++: integer multiplies, __umulhi and loads of the state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

struct PhiloxWords { uint32_t w[4]; };

__host__ __device__ __forceinline__ uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

__host__ __device__ __forceinline__ PhiloxWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = philox_mulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = philox_mulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return PhiloxWords{{c0, c1, c2, c3}};
}

// word i (0 ... 3, a run-time index) by selects: the words stay in registers
__host__ __device__ __forceinline__ uint32_t philox_pick(const PhiloxWords& p, int i) {
    const uint32_t lo = (i & 1) ? p.w[1] : p.w[0], hi = (i & 1) ? p.w[3] : p.w[2];
    return (i & 2) ? hi : lo;
}

// what a launch needs of the dropout: the state's address, the stream, the threshold and the scale
struct DropArgs {
    const uint32_t* rng;
    uint32_t stream_id, thr;
    float scale;
};

// the key and step of a launch, loaded once per thread (uniform addresses)
struct DropKey {
    uint32_t k0, k1, step;
    __device__ __forceinline__ explicit DropKey(const DropArgs& d) : k0(d.rng[0]), k1(d.rng[1] ^ d.stream_id), step(d.rng[2]) {}
    __device__ __forceinline__ DropKey() : k0(0), k1(0), step(0) {}
};
// the key where a kernel drops, nothing loaded where it does not
template <bool DROP> __device__ __forceinline__ DropKey drop_key(const DropArgs& d) { return DROP ? DropKey(d) : DropKey(); }

// the four words of columns 4 * (c >> 2) ... + 3 of row r of a row tensor
__device__ __forceinline__ PhiloxWords drop_row_words(const DropKey& k, size_t r, uint32_t cq) {
    return philox4x32_10(cq, (uint32_t)r, (uint32_t)((uint64_t)r >> 32), k.step, k.k0, k.k1);
}
// where four consecutive columns (or keys) sit on the four lanes of a quad, the quad shares the counter: lane L makes one call and takes
// word `word` of lane J's call (DPP quad permutes; every lane of the wave must be live)
template <int J> __device__ __forceinline__ uint32_t quad_bcast(uint32_t v) {      // lane J of the quad to its four lanes
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, J * 0x55, 0xF, 0xF, true);
}
template <int J> __device__ __forceinline__ uint32_t quad_word(const PhiloxWords& w, int word) {
    const PhiloxWords b = {{quad_bcast<J>(w.w[0]), quad_bcast<J>(w.w[1]), quad_bcast<J>(w.w[2]), quad_bcast<J>(w.w[3])}};
    return philox_pick(b, word);
}
// the four words of keys 4 * jq ... + 3 of query i of (clip, head) bh
__device__ __forceinline__ PhiloxWords drop_attn_words(const DropKey& k, uint32_t jq, uint32_t i, uint32_t bh) {
    return philox4x32_10(jq, i, bh, k.step, k.k0, k.k1);
}
// m * s of one word
__device__ __forceinline__ float drop_ms(uint32_t word, const DropArgs& d) { return word >= d.thr ? d.scale : 0.f; }
// m * s of element (r, c) of a row tensor: a whole call for one word (kernels that own four consecutive columns use drop_row_words)
__device__ __forceinline__ float drop_row_ms(const DropKey& k, const DropArgs& d, size_t r, int c) {
    return drop_ms(philox_pick(drop_row_words(k, r, (uint32_t)c >> 2), c & 3), d);
}

// host: thr and s of a probability; false for p outside [0, 1) or NaN
static inline bool drop_host_args(float p, const uint32_t* rng, uint32_t stream_id, DropArgs* out) {
    if (!(p >= 0.f) || !(p < 1.f)) return false;
    const double t = (double)p * 4294967296.0 + 0.5;
    const double f = t >= 4294967295.0 ? 4294967295.0 : (double)(uint64_t)t;
    out->rng = rng;
    out->stream_id = stream_id;
    out->thr = (uint32_t)f;
    out->scale = (float)(1.0 / (1.0 - (double)p));
    return true;
}
// the same behind an entry: the refusal and its error code
static inline int drop_require_args(float p, const uint32_t* rng, uint32_t stream_id, DropArgs* out) {
    SED_REQUIRE(drop_host_args(p, rng, stream_id, out), "the dropout probability must lie in [0, 1)");
    return 0;
}
