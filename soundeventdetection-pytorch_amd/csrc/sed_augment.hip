// Log-mel batch augmentation in one pass over the resident feature bank: crop gather, per-mel z-score, circular time shift,
// additive band gain, mixup with a partner sample, SpecAugment time / frequency masks -- and the same gather / shift / mix for
// the labels.  Every decision (starts, shifts, partners, lambdas, mask intervals, gains) is drawn on the host and arrives as a
// table; the kernels are element-wise, memory-bound and write no intermediate tensor.  Plain C++: no LDS, no atomics.
#include "common.h"

#include <math.h>

#define SED_AUG_MAX_MASKS 8

extern "C" int sed_logmel_augment_row_ints(int n_tmask, int n_fmask) { return 4 + 2 * (n_tmask + n_fmask); }

namespace {

struct AugParams {
    const float* bank;
    const float* mean;
    const float* stdv;
    const int* tab;          // [B][row_ints]: start, shift, partner, lam (float bits), (t0, w) x n_tmask, (f0, w) x n_fmask
    const float* gain;       // [B][n_mels] or NULL
    float* out;              // [B][crop][n_mels]
    float mask_value;
    int crop, n_mels, nq;    // nq = quads of mel bins per frame = ceil(n_mels / 4)
    int n_tmask, n_fmask, row_ints;
    int idx32;               // total < 2^32: the flat index splits with 32-bit divisions
    size_t total;            // B * crop * nq threads
};

// u_b[t][f0 .. f0 + nv) of the formula: the z-scored bank value at the shifted frame plus the sample's band gain
template <bool VEC>
__device__ __forceinline__ void aug_load_u(const AugParams& p, const int* __restrict__ row, int b, int t, int f0, int nv, float (&u)[4]) {
    int ts = t - row[1];                                   // (t - shift) mod crop: the shift wraps inside the crop
    if (ts < 0) ts += p.crop;
    const float* __restrict__ src = p.bank + ((size_t)row[0] + ts) * p.n_mels + f0;
    if (VEC) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = v[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = j < nv ? src[j] : 0.f;
    }
    if (p.mean) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) u[j] = (u[j] - p.mean[f0 + j]) / p.stdv[f0 + j];       // the expression of logmel_crops_kernel
    }
    if (p.gain) {
        const float* __restrict__ g = p.gain + (size_t)b * p.n_mels + f0;
        if (VEC) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(g);
#pragma unroll
            for (int j = 0; j < 4; ++j) u[j] += v[j];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nv) u[j] += g[j];
        }
    }
}

// one thread = four consecutive mel bins of one output frame
template <bool VEC>
__global__ __launch_bounds__(256) void logmel_augment_kernel(const AugParams p) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.total) return;
    unsigned fr, q;
    if (p.idx32) {
        const unsigned ii = (unsigned)i;
        fr = ii / (unsigned)p.nq;
        q = ii - fr * (unsigned)p.nq;
    } else {
        const size_t f = i / (size_t)p.nq;
        fr = (unsigned)f;
        q = (unsigned)(i - f * (size_t)p.nq);
    }
    const int b = (int)(fr / (unsigned)p.crop), t = (int)(fr - (unsigned)b * (unsigned)p.crop);
    const int f0 = (int)q * 4;
    const int nv = VEC ? 4 : (p.n_mels - f0 < 4 ? p.n_mels - f0 : 4);
    const int* __restrict__ row = p.tab + (size_t)b * p.row_ints;
    float* __restrict__ dst = p.out + (size_t)fr * p.n_mels + f0;

    bool tmasked = false;
    for (int j = 0; j < p.n_tmask; ++j) {
        const int t0 = row[4 + 2 * j], w = row[5 + 2 * j];
        tmasked |= t >= t0 && t < t0 + w;
    }
    float v[4];
    if (tmasked) {                                         // a masked frame reads nothing
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p.mask_value;
    } else {
        aug_load_u<VEC>(p, row, b, t, f0, nv, v);
        const int partner = row[2];
        if (partner != b) {
            const float lam = __builtin_bit_cast(float, row[3]), oml = 1.0f - lam;
            float w[4];
            aug_load_u<VEC>(p, p.tab + (size_t)partner * p.row_ints, partner, t, f0, nv, w);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = lam * v[j] + oml * w[j];
        }
        const int* __restrict__ fm = row + 4 + 2 * p.n_tmask;
        for (int j = 0; j < p.n_fmask; ++j) {
            const int lo = fm[2 * j], hi = lo + fm[2 * j + 1];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (f0 + e >= lo && f0 + e < hi) v[e] = p.mask_value;
        }
    }
    if (VEC) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = v[j];
        *reinterpret_cast<f32x4*>(dst) = o;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) dst[j] = v[j];
    }
}

// labels: the same gather / shift, and max (the rule of the complex-mode mix) or the convex combination in double; masks do not
// touch labels.  One thread per (b, t, k).
__global__ __launch_bounds__(256) void augment_labels_kernel(const double* __restrict__ events, const int* __restrict__ tab,
                                                             double* __restrict__ ev_out, int crop, int K, int row_ints,
                                                             int label_mix, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t f = i / (size_t)K;
    const int k = (int)(i - f * (size_t)K);
    const int b = (int)(f / (size_t)crop), t = (int)(f - (size_t)b * crop);
    const int* __restrict__ row = tab + (size_t)b * row_ints;
    int ts = t - row[1];
    if (ts < 0) ts += crop;
    double r = events[((size_t)row[0] + ts) * K + k];
    const int partner = row[2];
    if (partner != b) {
        const int* __restrict__ prow = tab + (size_t)partner * row_ints;
        int tp = t - prow[1];
        if (tp < 0) tp += crop;
        const double rp = events[((size_t)prow[0] + tp) * K + k];
        if (label_mix == 0) {
            r = fmax(r, rp);
        } else {
            const double lam = (double)__builtin_bit_cast(float, row[3]);
            r = lam * r + (1.0 - lam) * rp;
        }
    }
    ev_out[i] = r;
}

static inline bool ranges_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
    if (a == nullptr || b == nullptr) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + bbytes && b0 < a0 + abytes;
}
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}   // namespace

extern "C" int sed_logmel_augment(const float* bank, size_t bank_frames, const double* events, int K, const float* mean,
                                  const float* stdv, const int* tab_host, const int* tab, const float* gain, float mask_value,
                                  int label_mix, float* out, double* ev_out, int B, int crop, int n_mels, int n_tmask,
                                  int n_fmask, void* stream) {
    SED_REQUIRE(B > 0 && crop > 0 && n_mels > 0 && bank_frames > 0, "bad sizes");
    SED_REQUIRE((size_t)B * crop < (1u << 31), "too many frames for one launch");
    SED_REQUIRE(n_tmask >= 0 && n_tmask <= SED_AUG_MAX_MASKS && n_fmask >= 0 && n_fmask <= SED_AUG_MAX_MASKS,
                "at most 8 time masks and 8 frequency masks");
    SED_REQUIRE((mean == nullptr) == (stdv == nullptr), "mean/std must both be given or both NULL");
    SED_REQUIRE(events == nullptr || (ev_out != nullptr && K > 0), "a label bank needs ev_out and K > 0");
    SED_REQUIRE(label_mix == 0 || label_mix == 1, "label_mix is 0 (max) or 1 (convex)");
    SED_REQUIRE(bank != nullptr && tab_host != nullptr, "the bank and the host copy of the table are needed (null)");
    const int row_ints = sed_logmel_augment_row_ints(n_tmask, n_fmask);
    for (int b = 0; b < B; ++b) {       // every row is checked before anything is launched
        const int* row = tab_host + (size_t)b * row_ints;
        SED_REQUIRE(row[0] >= 0 && (size_t)row[0] + crop <= bank_frames, "crop outside the feature bank");
        SED_REQUIRE(row[1] >= 0 && row[1] < crop, "shift must lie in [0, crop)");
        SED_REQUIRE(row[2] >= 0 && row[2] < B, "partner must lie in [0, B)");
        const float lam = __builtin_bit_cast(float, row[3]);
        SED_REQUIRE(lam >= 0.0f && lam <= 1.0f, "lam must lie in [0, 1] (NaN refused)");
        for (int j = 0; j < n_tmask; ++j) {
            const int t0 = row[4 + 2 * j], w = row[5 + 2 * j];
            SED_REQUIRE(t0 >= 0 && w >= 0 && (long long)t0 + w <= crop, "time mask outside the crop");
        }
        for (int j = 0; j < n_fmask; ++j) {
            const int f0 = row[4 + 2 * n_tmask + 2 * j], w = row[5 + 2 * n_tmask + 2 * j];
            SED_REQUIRE(f0 >= 0 && w >= 0 && (long long)f0 + w <= n_mels, "frequency mask outside the mel axis");
        }
    }
    const size_t out_bytes = (size_t)B * crop * n_mels * sizeof(float);
    SED_REQUIRE(!ranges_overlap(out, out_bytes, bank, bank_frames * n_mels * sizeof(float)), "out overlaps the feature bank");
    SED_REQUIRE(!ranges_overlap(out, out_bytes, gain, (size_t)B * n_mels * sizeof(float)), "out overlaps the gain table");
    const size_t ltotal = events != nullptr ? (size_t)B * crop * K : 0, lblocks = cdivz(ltotal, 256);
    SED_REQUIRE(!ranges_overlap(ev_out, ltotal * sizeof(double), events, bank_frames * (size_t)(K > 0 ? K : 0) * sizeof(double)),
                "ev_out overlaps the label bank");
    SED_REQUIRE(lblocks < ((size_t)1 << 31), "too many label elements for one launch");
    const size_t blocks = cdivz((size_t)B * crop * ((n_mels + 3) / 4), 256);
    SED_REQUIRE(blocks < ((size_t)1 << 31), "too many elements for one launch");
    SED_REQUIRE(out != nullptr && tab != nullptr, "out and the device copy of the table are needed (null)");

    AugParams p;
    p.bank = bank; p.mean = mean; p.stdv = stdv; p.tab = tab; p.gain = gain; p.out = out;
    p.mask_value = mask_value;
    p.crop = crop; p.n_mels = n_mels; p.nq = (n_mels + 3) / 4;
    p.n_tmask = n_tmask; p.n_fmask = n_fmask; p.row_ints = row_ints;
    p.total = (size_t)B * crop * p.nq;
    p.idx32 = p.total < ((size_t)1 << 32);
    // float4 loads / stores: decided once per launch
    const bool vec = n_mels % 4 == 0 && aligned16(bank) && aligned16(out) && (gain == nullptr || aligned16(gain));
    hipStream_t st = (hipStream_t)stream;
    if (vec) logmel_augment_kernel<true><<<(unsigned)blocks, 256, 0, st>>>(p);
    else logmel_augment_kernel<false><<<(unsigned)blocks, 256, 0, st>>>(p);
    SED_LAUNCH_CHECK();
    if (events != nullptr) {
        augment_labels_kernel<<<(unsigned)lblocks, 256, 0, st>>>(events, tab, ev_out, crop, K, row_ints, label_mix, ltotal);
        SED_LAUNCH_CHECK();
    }
    return 0;
}
