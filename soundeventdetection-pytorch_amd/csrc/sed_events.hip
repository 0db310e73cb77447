// Event decoding between the model's frame probabilities and the event metrics: median filter along time, double-threshold
// (hysteresis) decisions with gap merging and minimum length, the (b, k, onset, offset) event list, and segment-based counts.
// Tensors are contiguous [B][T][K], time in the middle and classes innermost, as the models hand them over.  Every output is a
// selection or an integer: nothing here rounds.
//
// sed_median_time   one workgroup per (b, k, tile of MED_TILE outputs).  It stages the tile plus a halo of h = win/2 frames per side,
//   already reflected (half-sample symmetric, scipy's mode='reflect'), in LDS as ORDER KEYS: the fp32 bit pattern mapped to an
//   unsigned integer whose order is the order of the floats (and -0 < +0, so the order is total and the result unique).  Thread i
//   then selects the key of rank h among ks[i .. i + win) by radix selection, most significant bit first: 32 passes over the window
//   that each count the keys sharing the bits found so far whose next bit is 0.  32 * win LDS reads per output where counting the
//   rank of every candidate takes win^2; lanes read consecutive words, so no pass has a bank conflict.  The answer is a key that is
//   in the window: one of the input values, bit for bit, wherever the tile boundaries fall.  LDS: (512 + 510) * 4 = 4 KB.
//
// sed_decode_events  one wave per (b, k) row, twice: a counting pass, a prefix sum over the rows, and a writing pass that repeats the
//   walk with the row's offset in hand, so that the event order is (b, k, onset) by construction and no atomic decides anything.
//   The wave walks the row in chunks of DEC_CHUNK = 512 frames: every lane loads 8 frames (8 loads in flight per lane), each group of
//   64 frames becomes two 64-bit ballots (p > th_lo, p > th_hi), and the run logic works on those masks with count-trailing-zeros:
//   one step per run boundary, not per frame, the same scalar work in every lane.  Carried from word to word and chunk to chunk: the
//   open candidate run (start, "seen hi"), and the pending event (onset, offset) that the next kept run either extends (gap <=
//   max_gap) or closes.  Frames past T count as inactive, so a run that reaches the end closes at T.
//
// sed_segment_counts  grid (item blocks, K): a thread takes (b, segment) items of one class, ORs the segment's frames of the decisions
//   and of target > 0.5, and counts TP / FP / FN; one LDS tree per block, three integer atomics per block.
#include "common.h"

namespace {

constexpr int MED_THREADS = 256;
constexpr int MED_TILE = 512;        // outputs per workgroup (sed_median_time_tile)
constexpr int MED_MAX_WIN = 511;
constexpr int DEC_WORDS = 8;         // 64-frame words per chunk
constexpr int DEC_CHUNK = 64 * DEC_WORDS;
constexpr int MAX_FRAMES = 1 << 30;

// fp32 -> unsigned with the same order (negative: all bits flipped; positive: sign bit set), and back
__device__ __forceinline__ unsigned order_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ __launch_bounds__(MED_THREADS) void median_time_kernel(const float* __restrict__ in, float* __restrict__ out, int T, int K,
                                                                  int h) {
    __shared__ unsigned ks[MED_TILE + MED_MAX_WIN - 1];
    const int tid = threadIdx.x;
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);       // the K rows of one tile share cache lines: neighbours on one XCD
    const int k = (int)(lb % (unsigned)K);
    const int t0 = (int)(lb / (unsigned)K) * MED_TILE;
    const int tn = T - t0 < MED_TILE ? T - t0 : MED_TILE;
    const size_t row = (size_t)blockIdx.y * (size_t)T * (size_t)K + (size_t)k;
    const long long two_t = 2LL * T;
    for (int i = tid; i < tn + 2 * h; i += MED_THREADS) {
        long long m = ((long long)t0 - h + i) % two_t;
        if (m < 0) m += two_t;
        const long long src = m < T ? m : two_t - 1 - m;
        ks[i] = order_key(in[row + (size_t)src * K]);
    }
    __syncthreads();
    const int win = 2 * h + 1;
    for (int i = tid; i < tn; i += MED_THREADS) {
        unsigned prefix = 0;         // the bits of the answer found so far, the others 0
        int want = h;                // rank of the answer among the keys that share them
        for (int bit = 31; bit >= 0; --bit) {
            int c0 = 0;              // keys that share the found bits and have a 0 at `bit`
            for (int j = 0; j < win; ++j) c0 += (((ks[i + j] ^ prefix) >> bit) == 0u) ? 1 : 0;
            if (want >= c0) { want -= c0; prefix |= 1u << bit; }
        }
        out[row + (size_t)(t0 + i) * K] = key_value(prefix);
    }
}

struct DecodeArgs {
    const float* prob;
    unsigned char* decisions;
    int* events;
    int* row_counts;
    const int* offsets;
    int T, K;
    float th_hi, th_lo;
    int max_gap, min_len, max_events;
};

__device__ __forceinline__ void fill_frames(unsigned char* dec, int K, int from, int to, unsigned char v, int lane) {
    for (int t = from + lane; t < to; t += 64) dec[(size_t)t * K] = v;
}

template <bool WRITE>
__global__ __launch_bounds__(64) void decode_rows_kernel(const DecodeArgs a) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const int b = row / a.K, k = row - b * a.K;
    const int T = a.T;
    const size_t base = (size_t)b * (size_t)T * (size_t)a.K + (size_t)k;
    const float* __restrict__ p = a.prob + base;
    unsigned char* dec = (WRITE && a.decisions) ? a.decisions + base : nullptr;
    const int first = WRITE ? a.offsets[row] : 0;

    bool in_run = false, run_hi = false, pending = false;
    int run_start = 0, ev_on = 0, ev_off = 0, n_ev = 0, dec_pos = 0;

    // the pending event is final: keep it if it is long enough
    auto flush = [&]() {
        if (ev_off - ev_on >= a.min_len) {
            if (WRITE) {
                if (lane == 0 && first + n_ev < a.max_events) {
                    int* e = a.events + 4 * (size_t)(first + n_ev);
                    e[0] = b; e[1] = k; e[2] = ev_on; e[3] = ev_off;
                }
                if (dec) {
                    fill_frames(dec, a.K, dec_pos, ev_on, 0, lane);
                    fill_frames(dec, a.K, ev_on, ev_off, 1, lane);
                    dec_pos = ev_off;
                }
            }
            ++n_ev;
        }
        pending = false;
    };
    // the candidate run [run_start, end) is complete: without a hi frame it counts as inactive
    auto close_run = [&](int end) {
        in_run = false;
        if (!run_hi) return;
        if (pending && run_start - ev_off <= a.max_gap) { ev_off = end; return; }
        if (pending) flush();
        pending = true; ev_on = run_start; ev_off = end;
    };

    for (int t0 = 0; t0 < T; t0 += DEC_CHUNK) {
        float v[DEC_WORDS];
#pragma unroll
        for (int w = 0; w < DEC_WORDS; ++w) {
            const int t = t0 + w * 64 + lane;
            v[w] = t < T ? p[(size_t)t * a.K] : 0.f;
        }
#pragma unroll
        for (int w = 0; w < DEC_WORDS; ++w) {
            const int tw = t0 + w * 64;
            const bool valid = tw + lane < T;
            const unsigned long long lo = __builtin_amdgcn_ballot_w64(valid && v[w] > a.th_lo);
            const unsigned long long hi = __builtin_amdgcn_ballot_w64(valid && v[w] > a.th_hi);
            int pos = 0;
            for (int it = 0; it < 130 && pos < 64; ++it) {      // one step per run boundary: at most 65 steps for a word's 64 boundaries
                const unsigned long long from = ~0ull << pos;
                if (in_run) {
                    const unsigned long long m = ~lo & from;
                    if (m == 0) { run_hi = run_hi || (hi & from) != 0; pos = 64; }
                    else {
                        const int z = __builtin_ctzll(m);
                        run_hi = run_hi || (hi & from & ((1ull << z) - 1)) != 0;
                        close_run(tw + z);
                        pos = z;
                    }
                } else {
                    const unsigned long long m = lo & from;
                    if (m == 0) pos = 64;
                    else { pos = __builtin_ctzll(m); in_run = true; run_hi = false; run_start = tw + pos; }
                }
            }
        }
    }
    if (in_run) close_run(T);
    if (pending) flush();
    if (WRITE) {
        if (dec) fill_frames(dec, a.K, dec_pos, T, 0, lane);
    } else if (lane == 0) {
        a.row_counts[row] = n_ev;
    }
}

// exclusive prefix sum of the row counts in row order: thread i owns rows [i * per, (i + 1) * per)
__global__ __launch_bounds__(256) void decode_scan_kernel(const int* __restrict__ counts, int* __restrict__ offsets,
                                                          int* __restrict__ total, int n) {
    __shared__ int part[256];
    const int tid = threadIdx.x;
    const long long per = ((long long)n + 255) / 256;
    const int lo = (int)(tid * per < n ? tid * per : n), hi = (int)((tid + 1) * per < n ? (tid + 1) * per : n);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += counts[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int i = 0; i < 256; ++i) { const int c = part[i]; part[i] = acc; acc += c; }
        total[0] = acc;
    }
    __syncthreads();
    int acc = part[tid];
    for (int i = lo; i < hi; ++i) { offsets[i] = acc; acc += counts[i]; }
}

__global__ __launch_bounds__(256) void segment_counts_kernel(const unsigned char* __restrict__ dec, const float* __restrict__ tgt,
                                                             long long items, int T, int Tt, int K, int L, int n, int S,
                                                             unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long sm[3][256];
    const int tid = threadIdx.x, k = blockIdx.y;
    unsigned long long c[3] = {0, 0, 0};        // TP, FP, FN
    for (long long i = (long long)blockIdx.x * 256 + tid; i < items; i += (long long)gridDim.x * 256) {
        const long long b = i / S;
        const long long f0 = (i - b * S) * L, f1 = f0 + L < n ? f0 + L : n;
        bool pa = false, ra = false;
        for (long long f = f0; f < f1; ++f) {
            pa = pa || dec[((size_t)b * T + (size_t)f) * K + k] != 0;
            ra = ra || tgt[((size_t)b * Tt + (size_t)f) * K + k] > 0.5f;
        }
        c[0] += (pa && ra) ? 1 : 0;
        c[1] += (pa && !ra) ? 1 : 0;
        c[2] += (!pa && ra) ? 1 : 0;
    }
    for (int j = 0; j < 3; ++j) sm[j][tid] = c[j];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
            for (int j = 0; j < 3; ++j) sm[j][tid] += sm[j][tid + s];
        __syncthreads();
    }
    if (tid < 3 && sm[tid][0] != 0) atomicAdd(&counts[(size_t)k * 3 + tid], sm[tid][0]);
}

bool decode_shape_ok(int B, int T, int K) {
    if (B < 1 || T < 1 || K < 1 || T > MAX_FRAMES) return false;
    if ((long long)B * K > 0x7fffffffLL) return false;
    return (long long)B * K * ((T + 1) / 2) <= 0x7fffffffLL;      // the largest possible event count fits int32
}

}  // namespace

extern "C" int sed_median_time_tile(void) { return MED_TILE; }

extern "C" int sed_median_time(const float* in, float* out, int B, int T, int K, int win, void* stream) {
    SED_REQUIRE(in != nullptr && out != nullptr, "null pointer");
    SED_REQUIRE(in != out, "the filter does not run in place");
    SED_REQUIRE(win >= 1 && win <= MED_MAX_WIN && (win & 1) == 1, "win must be odd, 1..511");
    SED_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= MAX_FRAMES && K >= 1, "B in 1..65535, T in 1..2^30, K >= 1");
    const long long blocks = (long long)cdiv(T, MED_TILE) * K;
    SED_REQUIRE(blocks <= 0x7fffffffLL, "too many (tile, class) pairs for one grid");
    median_time_kernel<<<dim3((unsigned)blocks, (unsigned)B), MED_THREADS, 0, (hipStream_t)stream>>>(in, out, T, K, win / 2);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_decode_events_chunk(void) { return DEC_CHUNK; }

extern "C" size_t sed_decode_events_ws_bytes(int B, int T, int K) {
    if (!decode_shape_ok(B, T, K)) return 0;
    return (size_t)B * (size_t)K * sizeof(int);
}

extern "C" int sed_decode_events(const float* prob, int B, int T, int K, float th_hi, float th_lo, int max_gap, int min_len,
                                 unsigned char* decisions, int* events, int max_events, int* row_counts, int* total, void* workspace,
                                 void* stream) {
    SED_REQUIRE(prob != nullptr && row_counts != nullptr && total != nullptr && workspace != nullptr, "null pointer");
    SED_REQUIRE(max_events >= 0 && (events != nullptr || max_events == 0), "events must hold max_events >= 0 rows");
    SED_REQUIRE(th_lo <= th_hi, "th_lo must not exceed th_hi");
    SED_REQUIRE(max_gap >= 0, "max_gap must be >= 0");
    SED_REQUIRE(min_len >= 1, "min_len must be >= 1");
    SED_REQUIRE(decode_shape_ok(B, T, K), "B, T, K >= 1, T <= 2^30, B*K*ceil(T/2) below 2^31");
    DecodeArgs a;
    a.prob = prob; a.decisions = decisions; a.events = events; a.row_counts = row_counts;
    a.offsets = reinterpret_cast<const int*>(workspace);
    a.T = T; a.K = K; a.th_hi = th_hi; a.th_lo = th_lo; a.max_gap = max_gap; a.min_len = min_len; a.max_events = max_events;
    const int rows = B * K;
    hipStream_t st = (hipStream_t)stream;
    decode_rows_kernel<false><<<rows, 64, 0, st>>>(a);
    SED_LAUNCH_CHECK();
    decode_scan_kernel<<<1, 256, 0, st>>>(row_counts, reinterpret_cast<int*>(workspace), total, rows);
    SED_LAUNCH_CHECK();
    decode_rows_kernel<true><<<rows, 64, 0, st>>>(a);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_segment_counts(const unsigned char* decisions, const float* target, int B, int T, int Tt, int K, int seg_frames,
                                  long long* counts, void* stream) {
    SED_REQUIRE(decisions != nullptr && target != nullptr && counts != nullptr, "null pointer");
    SED_REQUIRE(B >= 1 && T >= 1 && Tt >= 1 && K >= 1 && K <= 65535, "B, T, Tt >= 1, K in 1..65535");
    SED_REQUIRE(seg_frames >= 1, "seg_frames must be >= 1");
    const int n = T < Tt ? T : Tt;
    const int S = cdiv(n, seg_frames);
    const long long items = (long long)B * S;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)K * 3 * sizeof(long long), st) != hipSuccess) {
        sed_set_error("sed_segment_counts: clearing counts failed");
        return 2;
    }
    const long long want = (items + 255) / 256;
    const unsigned gx = (unsigned)(want < 64 ? want : 64);
    segment_counts_kernel<<<dim3(gx, (unsigned)K), 256, 0, st>>>(decisions, target, items, T, Tt, K, seg_frames, n, S,
                                                               reinterpret_cast<unsigned long long*>(counts));
    SED_LAUNCH_CHECK();
    return 0;
}
