// PSDS intersection counts for a whole threshold sweep in ONE launch: per (threshold, detected class) the true positives, false
// positives, detections and cross-triggers of the polyphonic sound detection score (Bilen et al., ICASSP 2020), on the frame grid.
// Everything is an integer, every addition an integer atomic: the same bits on every run.
//
// Definition (include/sed_hip.h has the same text).  prob fp32 [B][T][K], target fp32 [B][Tt][K], classes innermost; the first
// n = min(T, Tt) frames of a recording are scored.  th: nth (1..64) fp32 thresholds in any order.  Criteria as integer fractions
// num/den, 0 < num <= den <= 2^15: DTC, GTC, CTTC.
//   ground-truth event of class c in recording b: a maximal run of target[b][t][c] > 0.5 within [0, n).
//   detection of class k at threshold i:           a maximal run of prob[b][t][k] > th[i] within [0, n); strict, fp32, a NaN never
//                                                  detects (sed_decode_events with th_lo == th_hi, max_gap = 0, min_len = 1).
//   DTC   a detection d is relevant if I * den_dtc >= num_dtc * |d|, I = d's frames with target[..][k] > 0.5; otherwise it is a
//         false positive.
//   GTC   a ground-truth event g of class k is a true positive if J * den_gtc >= num_gtc * |g|, J = g's frames covered by RELEVANT
//         detections of class k.
//   CTTC  a false-positive detection d of class k cross-triggers class c != k if Ic * den_cttc >= num_cttc * |d|, Ic = d's frames
//         with target[..][c] > 0.5.  One detection may cross-trigger several classes and still is one false positive.
// counts int64 [nth][K][K + 3] = (tp, fp, ndet, ct[0..K-1]) for detected class k (ct[k] stays 0); gt int64 [K][2] = (ground-truth
// events, their frames), added once per call.  The call ADDS to both.
//
// Shape chosen (the one the issue suggested, with these decisions):
//   * One workgroup of 256 threads per (k, b).  Its LDS holds, as 64-frame bit words (bit j of word w = frame 64 w + j), the
//     target > 0.5 rows of ALL K classes of recording b, the prob > th[i] rows of class k for every threshold i, and nth * K
//     cross-trigger counters.  Row pitch Wp = W | 1 words (odd: threads that walk different rows at the same word index are on
//     different banks).  sed_psds_max_frames is what fits in PS_LDS_BUDGET.
//   * Building the words.  Wave v takes words v, v + 4, ...  Detections: lane j loads frame 64 w + j of column k once, then one
//     __ballot per threshold gives the word directly (th is a by-value kernel argument, so the compare takes a scalar operand).
//     Targets: the 64 frames x K classes of a word are ONE contiguous run of the [Tt][K] array; the wave reads it flat (whole
//     lines, every byte used) and each lane ORs its bit into the word of its class with a 32-bit LDS atomic (an OR is order-free).
//   * The global reads.  The target rows of all K classes are needed by every (b, k) workgroup, so each workgroup reads its
//     recording's whole target array: K workgroups pull each line, from L2 after the first.  The prob column read has a stride of K
//     floats: it touches the same number of lines once more, i.e. the workgroup's line traffic is 2x the target read, not K x on
//     top of it, and it needs 1/K of the load instructions a whole-line read with an LDS transpose would issue for the same lines.
//     At (100, 6001, 14) that is 1400 workgroups x 2 x 336 KB = 0.94 GB out of L2 for 33.6 MB + 33.6 MB out of HBM.  Measured
//     (tools/psds_time.py, profiles/psds_time.json): the launch takes 3.1 ms there with 50 thresholds, 303 GB/s on that model, far
//     below what L2 delivers, and at K = 1, where nothing is strided, 100 workgroups take 0.55 ms: the walks below bound the
//     launch, not these reads (the two phases were not timed separately).
//   * The walks.  Thread (lane l, wave v) owns threshold i = 4 l + v, so the thresholds spread over the four SIMDs.  It walks its
//     detection row with ctz over words; per run it popcounts the target row of class k under the run (DTC).  A false positive is
//     popcounted against the other K - 1 target rows (CTTC) and then CLEARED from the row, so that after the walk the row holds the
//     relevant detections only; the walk over class k's ground-truth runs popcounts that row (GTC).  The thread that owns
//     threshold 0 also counts the ground-truth events and frames.  No barrier follows the build; every __syncthreads() is outside
//     divergent control flow.
//   * Output: one 64-bit integer atomic per non-zero count.
#include "common.h"

namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_MAX_K = 64;
constexpr int PS_MAX_TH = 64;
constexpr int PS_MAX_B = 65535;
constexpr int PS_MAX_DEN = 1 << 15;
constexpr size_t PS_LDS_BUDGET = 144 * 1024;      // of the CU's 160 KB

typedef unsigned long long u64;

struct PsdsTh {
    float v[PS_MAX_TH];
};

struct PsdsCrit {
    int dtc_num, dtc_den, gtc_num, gtc_den, cttc_num, cttc_den;
};

// first set bit of row[0 .. W) at or after pos; 64 W if there is none
__device__ __forceinline__ int next_set(const u64* row, int pos, int W) {
    int w = pos >> 6;
    if (w >= W) return W << 6;
    u64 m = row[w] & (~0ull << (pos & 63));
    while (m == 0) {
        if (++w >= W) return W << 6;
        m = row[w];
    }
    return (w << 6) + __builtin_ctzll(m);
}

// first clear bit at or after pos; 64 W if there is none
__device__ __forceinline__ int next_clear(const u64* row, int pos, int W) {
    int w = pos >> 6;
    if (w >= W) return W << 6;
    u64 m = ~row[w] & (~0ull << (pos & 63));
    while (m == 0) {
        if (++w >= W) return W << 6;
        m = ~row[w];
    }
    return (w << 6) + __builtin_ctzll(m);
}

// the bits of word w that lie in [s, e), s < e, w in [s >> 6, (e - 1) >> 6]
__device__ __forceinline__ u64 range_mask(int w, int s, int e) {
    u64 m = ~0ull;
    if (w == (s >> 6)) m &= ~0ull << (s & 63);
    if (w == ((e - 1) >> 6)) m &= ~0ull >> (63 - ((e - 1) & 63));
    return m;
}

__device__ __forceinline__ int count_range(const u64* row, int s, int e) {
    int c = 0;
    for (int w = s >> 6; w <= ((e - 1) >> 6); ++w) c += __builtin_popcountll(row[w] & range_mask(w, s, e));
    return c;
}

__device__ __forceinline__ void clear_range(u64* row, int s, int e) {
    for (int w = s >> 6; w <= ((e - 1) >> 6); ++w) row[w] &= ~range_mask(w, s, e);
}

__global__ __launch_bounds__(PS_THREADS) void psds_counts_kernel(const float* __restrict__ prob, const float* __restrict__ target,
                                                                 int T, int Tt, int K, int n, int W, int Wp, PsdsTh th, int nth,
                                                                 PsdsCrit cr, u64* __restrict__ counts, u64* __restrict__ gt) {
    extern __shared__ u64 ps_lds[];
    u64* tg = ps_lds;                                            // [K][Wp]   target > 0.5
    u64* det = tg + (size_t)K * Wp;                              // [nth][Wp] prob[..][k] > th[i]
    unsigned* ct = reinterpret_cast<unsigned*>(det + (size_t)nth * Wp);   // [nth][K]
    unsigned* tg32 = reinterpret_cast<unsigned*>(tg);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int k = blockIdx.x, b = blockIdx.y;

    for (int i = tid; i < K * Wp; i += PS_THREADS) tg[i] = 0;
    for (int i = tid; i < nth * K; i += PS_THREADS) ct[i] = 0;
    __syncthreads();

    const float* __restrict__ pb = prob + (size_t)b * (size_t)T * (size_t)K + (size_t)k;
    const float* __restrict__ tb = target + (size_t)b * (size_t)Tt * (size_t)K;
    for (int w = wave; w < W; w += PS_THREADS / 64) {
        const int t0 = w << 6, t = t0 + lane;
        const bool valid = t < n;
        const float p = valid ? pb[(size_t)t * (size_t)K] : 0.f;
        u64 mine = 0;
        for (int i = 0; i < nth; ++i) {
            const u64 m = __builtin_amdgcn_ballot_w64(valid && p > th.v[i]);
            if (lane == i) mine = m;
        }
        if (lane < nth) det[lane * Wp + w] = mine;
        const int rn = n - t0 < 64 ? n - t0 : 64;
        const int items = rn * K;
        const float* __restrict__ src = tb + (size_t)t0 * (size_t)K;
        for (int idx = lane; idx < items; idx += 64) {
            const int r = idx / K, c = idx - r * K;
            if (src[idx] > 0.5f) atomicOr(&tg32[2 * (c * Wp + w) + (r >> 5)], 1u << (r & 31));
        }
    }
    __syncthreads();

    const int i = 4 * lane + wave;
    if (i >= nth) return;
    u64* D = det + (size_t)i * Wp;
    const u64* G = tg + (size_t)k * Wp;
    unsigned* myct = ct + i * K;
    long long tp = 0, fp = 0, ndet = 0;
    for (int pos = next_set(D, 0, W); pos < n;) {
        const int end = next_clear(D, pos, W);          // <= n: no bit at or past n is set
        const long long len = end - pos;
        ++ndet;
        if ((long long)count_range(G, pos, end) * cr.dtc_den < cr.dtc_num * len) {
            ++fp;
            for (int c = 0; c < K; ++c) {
                if (c == k) continue;
                if ((long long)count_range(tg + (size_t)c * Wp, pos, end) * cr.cttc_den >= cr.cttc_num * len) ++myct[c];
            }
            clear_range(D, pos, end);
        }
        pos = next_set(D, end, W);
    }
    long long n_gt = 0, gt_frames = 0;
    for (int pos = next_set(G, 0, W); pos < n;) {
        const int end = next_clear(G, pos, W);
        const long long len = end - pos;
        ++n_gt;
        gt_frames += len;
        if ((long long)count_range(D, pos, end) * cr.gtc_den >= cr.gtc_num * len) ++tp;
        pos = next_set(G, end, W);
    }
    u64* out = counts + ((size_t)i * K + k) * (size_t)(K + 3);
    if (tp) atomicAdd(&out[0], (u64)tp);
    if (fp) atomicAdd(&out[1], (u64)fp);
    if (ndet) atomicAdd(&out[2], (u64)ndet);
    for (int c = 0; c < K; ++c)
        if (myct[c]) atomicAdd(&out[3 + c], (u64)myct[c]);
    if (i == 0 && n_gt) {
        atomicAdd(&gt[2 * k], (u64)n_gt);
        atomicAdd(&gt[2 * k + 1], (u64)gt_frames);
    }
}

inline bool psds_kth_ok(int K, int nth) { return K >= 1 && K <= PS_MAX_K && nth >= 1 && nth <= PS_MAX_TH; }
inline bool psds_frac_ok(int num, int den) { return num > 0 && num <= den && den <= PS_MAX_DEN; }
inline size_t psds_lds_bytes(int K, int nth, int Wp) { return (size_t)(K + nth) * Wp * sizeof(u64) + (size_t)nth * K * sizeof(unsigned); }

// the largest word count W whose pitch W | 1 fits the budget
inline int psds_max_words(int K, int nth) {
    const size_t wmax = (PS_LDS_BUDGET - (size_t)nth * K * sizeof(unsigned)) / ((size_t)(K + nth) * sizeof(u64));
    return (int)((wmax & 1) ? wmax : wmax - 1);
}

}  // namespace

extern "C" int sed_psds_max_frames(int K, int nth) {
    if (!psds_kth_ok(K, nth)) return 0;
    return psds_max_words(K, nth) * 64;
}

extern "C" int sed_psds_counts(const float* prob, const float* target, int B, int T, int Tt, int K, const float* th, int nth,
                               int dtc_num, int dtc_den, int gtc_num, int gtc_den, int cttc_num, int cttc_den, long long* counts,
                               long long* gt, void* stream) {
    SED_REQUIRE(psds_kth_ok(K, nth), "K in 1..64, nth in 1..64");
    SED_REQUIRE(B >= 0 && B <= PS_MAX_B && T >= 0 && Tt >= 0, "B in 0..65535, T >= 0, Tt >= 0");
    SED_REQUIRE(psds_frac_ok(dtc_num, dtc_den) && psds_frac_ok(gtc_num, gtc_den) && psds_frac_ok(cttc_num, cttc_den),
                "criteria are fractions with 0 < num <= den <= 2^15");
    const int n = T < Tt ? T : Tt;
    SED_REQUIRE(n <= sed_psds_max_frames(K, nth), "min(T, Tt) exceeds sed_psds_max_frames(K, nth)");
    SED_REQUIRE(th != nullptr, "null pointer");
    if (n == 0 || B == 0) return 0;
    SED_REQUIRE(prob != nullptr && target != nullptr && counts != nullptr && gt != nullptr, "null pointer");
    PsdsTh tv;
    for (int i = 0; i < PS_MAX_TH; ++i) tv.v[i] = i < nth ? th[i] : 0.f;
    const PsdsCrit cr{dtc_num, dtc_den, gtc_num, gtc_den, cttc_num, cttc_den};
    const int W = (n + 63) >> 6, Wp = W | 1;
    const size_t lds = psds_lds_bytes(K, nth, Wp);
    if (int rc = sed_set_max_lds<psds_counts_kernel>(lds)) return rc;
    psds_counts_kernel<<<dim3((unsigned)K, (unsigned)B), PS_THREADS, lds, (hipStream_t)stream>>>(
        prob, target, T, Tt, K, n, W, Wp, tv, nth, cr, reinterpret_cast<u64*>(counts), reinterpret_cast<u64*>(gt));
    SED_LAUNCH_CHECK();
    return 0;
}
