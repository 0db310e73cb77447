// Audio ingest: PCM decode + channel downmix + polyphase-FIR resampling in one launch (read_multichannel_audio,
// dataset/dataset_utils.py:65-91 of the reference, with scipy.signal.resample_poly's defaults in place of librosa.resample).
//
//   y[m] = sum_k h[m*down + half - k*up] * x[k],  half = 10*max(up, down), h = up * (Kaiser-5 windowed sinc of 2*half + 1 taps)
//
// With t = m*down + half = q*up + p (0 <= p < up) the taps of output m are h[p], h[p + up], h[p + 2 up], ... against
// x[q], x[q - 1], x[q - 2], ...: the host hands the filter over PHASE-MAJOR, taps[p][i] = (float)h[p + i*up] (0 past the end of h),
// rows padded to an odd length Tp, so that one output reads one contiguous row and a wave's rows start on distinct banks for up <= 32.
//
// One workgroup per (row, output channel, tile of `tile` consecutive outputs).  It stages
//   - the input span the tile needs, decoded and downmixed on the way in, zero outside [0, n_in): lane l takes frame l of the span,
//     so a wave's loads cover one contiguous run of the interleaved PCM (one 4 / 8 / 16-byte load per frame where the frame has that
//     size and alignment); the workgroups of one tile's output channels are neighbours on one XCD (xcd_remap) and share those lines
//     in its L2;
//   - the whole phase table.
// Taps come from LDS, not from L2: the table is at most 640 rows x 21 taps (up = 640) or 1 x 12801 (up = 1, down = 640), under 54 KB,
// and the span buffer is 16 KB, so the largest workgroup holds 70 KB of the CU's 160 KB and two workgroups still fit per CU; for the
// everyday ratios (2/3, 3/2, 160/147, 147/160) the table is 0.2 .. 14 KB.  Every output reads its T taps once, so from L2 they
// would cost tile * T * 4 bytes of L1 misses per workgroup -- for tile >= up never less than staging the table once -- at L2 latency
// inside the FMA chain.  The tile is sized so that span = tile * down / up + T fits the 4096-sample buffer (at most 4096 outputs);
// where it cannot (T > 4096: down / up above ~190), the workgroup walks the span in 4096-sample chunks and each thread adds a
// chunk's partial sum to the output it owns.
// Accumulation: one fp32 fmaf chain per output, taps in ascending order.  m * down and every offset are 64-bit.
#include "common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_SPAN = 4096;        // staged input samples per chunk
constexpr int RS_TILE_MAX = 4096;    // outputs per workgroup, a multiple of RS_THREADS
constexpr int RS_MAX_RATIO = 640;
constexpr int RS_MAX_CH = 64;

template <typename T> struct Pcm;
template <> struct Pcm<int16_t> { typedef long long sum_t; static constexpr double scale = 1.0 / 32768.0; };
template <> struct Pcm<int32_t> { typedef long long sum_t; static constexpr double scale = 1.0 / 2147483648.0; };
template <> struct Pcm<float> { typedef double sum_t; static constexpr double scale = 1.0; };

// One output-channel sample of one interleaved frame.  pick >= 0: that channel.  pick < 0: the mean over the ch_in channels, the sum
// formed exactly (integers) or in fp64 (float), scaling and division in fp64, ONE rounding to fp32: float32(host path) bit for bit
// for integer PCM.  vec = 2 / 4: the frame is one aligned vector load.
template <typename T>
__device__ __forceinline__ float ingest_sample(const T* __restrict__ f, int ch_in, int pick, int vec) {
    typedef typename Pcm<T>::sum_t sum_t;
    typedef T vec2_t __attribute__((ext_vector_type(2)));
    typedef T vec4_t __attribute__((ext_vector_type(4)));
    if (pick >= 0) return (float)((double)f[pick] * Pcm<T>::scale);
    sum_t s = 0;
    if (vec == 2) {
        const vec2_t v = *reinterpret_cast<const vec2_t*>(f);
        s = (sum_t)v[0] + (sum_t)v[1];
    } else if (vec == 4) {
        const vec4_t v = *reinterpret_cast<const vec4_t*>(f);
        s = (sum_t)v[0] + (sum_t)v[1] + (sum_t)v[2] + (sum_t)v[3];
    } else {
        for (int c = 0; c < ch_in; ++c) s += (sum_t)f[c];
    }
    return (float)((double)s * Pcm<T>::scale / (double)ch_in);
}

struct ResampleArgs {
    const void* x;        // [B][n_in][ch_in] PCM
    const float* taps;    // [up][Tp]
    float* y;             // [B][ch_out][n_out]
    int n_in, n_out, ch_in, ch_out;
    int nch;              // workgroups per tile: ch_out, or 1 when every output channel is the same mean
    int pick_base;        // -1: mean of all channels; 0: output channel c picks input channel c
    int vec;
    int up, down, half, T, Tp, tile;
};

template <typename T>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    const int tid = threadIdx.x;
    const int tab = (a.up * a.Tp + 3) & ~3;
    float* hs = rs_lds;
    float* xs = rs_lds + tab;
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int c = (int)(lb % (unsigned)a.nch);
    const long long m0 = (long long)(lb / (unsigned)a.nch) * a.tile;
    const int b = blockIdx.y;
    const int tm = (int)(a.n_out - m0 < a.tile ? a.n_out - m0 : a.tile);
    const int pick = a.pick_base < 0 ? -1 : c;

    for (int i = tid; i < a.up * a.Tp; i += RS_THREADS) hs[i] = a.taps[i];

    const long long t0 = m0 * a.down + a.half;
    const long long q0 = t0 / a.up;
    const unsigned p0 = (unsigned)(t0 - q0 * a.up);
    const long long k_first = q0 - (a.T - 1);
    const long long k_last = (t0 + (long long)(tm - 1) * a.down) / a.up;
    const T* __restrict__ xrow = reinterpret_cast<const T*>(a.x) + (size_t)b * (size_t)a.n_in * (size_t)a.ch_in;
    const int ncopy = a.nch == 1 ? a.ch_out : 1;
    float* __restrict__ yrow = a.y + ((size_t)b * a.ch_out + (a.nch == 1 ? 0 : c)) * (size_t)a.n_out + (size_t)m0;

    for (long long c0 = k_first; c0 <= k_last; c0 += RS_SPAN) {
        const int len = (int)(k_last - c0 + 1 < RS_SPAN ? k_last - c0 + 1 : RS_SPAN);
        __syncthreads();                                   // the previous chunk has been consumed
        for (int i = tid; i < len; i += RS_THREADS) {
            const long long k = c0 + i;
            xs[i] = (k >= 0 && k < a.n_in) ? ingest_sample<T>(xrow + (size_t)k * a.ch_in, a.ch_in, pick, a.vec) : 0.f;
        }
        __syncthreads();
        const int qrel = (int)(q0 - c0);                   // x[q0] sits at xs[qrel] (may lie outside this chunk)
        const bool first = c0 == k_first;
        for (int mi = tid; mi < tm; mi += RS_THREADS) {
            const unsigned rel = p0 + (unsigned)mi * (unsigned)a.down;      // < 640 + 4096 * 640
            const unsigned q = rel / (unsigned)a.up;
            const int p = (int)(rel - q * (unsigned)a.up);
            const int kx = qrel + (int)q;                  // tap i multiplies xs[kx - i]
            const int ilo = kx - (len - 1) > 0 ? kx - (len - 1) : 0;
            const int ihi = kx < a.T - 1 ? kx : a.T - 1;
            if (!first && ilo > ihi) continue;
            const float* __restrict__ hrow = hs + p * a.Tp;
            float acc = 0.f;
#pragma unroll 4
            for (int i = ilo; i <= ihi; ++i) acc = fmaf(hrow[i], xs[kx - i], acc);
            for (int cc = 0; cc < ncopy; ++cc) {
                float* dst = yrow + (size_t)cc * a.n_out + mi;
                *dst = first ? acc : *dst + acc;           // (later chunks: the same thread wrote *dst)
            }
        }
    }
}

// up == down == 1: decode + downmix alone, one thread per (row, output channel, frame)
template <typename T>
__global__ __launch_bounds__(RS_THREADS) void ingest_kernel(const ResampleArgs a) {
    const long long k = (long long)blockIdx.x * RS_THREADS + threadIdx.x;
    if (k >= a.n_in) return;
    const int c = blockIdx.y % a.nch, b = blockIdx.y / a.nch;
    const int pick = a.pick_base < 0 ? -1 : c;
    const T* f = reinterpret_cast<const T*>(a.x) + ((size_t)b * (size_t)a.n_in + (size_t)k) * (size_t)a.ch_in;
    const float v = ingest_sample<T>(f, a.ch_in, pick, a.vec);
    const int ncopy = a.nch == 1 ? a.ch_out : 1;
    float* dst = a.y + ((size_t)b * a.ch_out + (a.nch == 1 ? 0 : c)) * (size_t)a.n_out + (size_t)k;
    for (int cc = 0; cc < ncopy; ++cc) dst[(size_t)cc * a.n_out] = v;
}

int gcd_int(int x, int y) {
    while (y) { const int t = x % y; x = y; y = t; }
    return x;
}

int taps_per_phase(int up, int down) { return 20 * (up > down ? up : down) / up + 1; }

int tile_outputs(int up, int down) {
    const long long fit = (long long)(RS_SPAN - taps_per_phase(up, down) - 2) * up / down;
    if (fit >= RS_TILE_MAX) return RS_TILE_MAX;
    if (fit < RS_THREADS) return RS_THREADS;               // the span no longer fits one chunk: the kernel walks it
    return (int)(fit / RS_THREADS) * RS_THREADS;
}

template <typename T>
int launch(const ResampleArgs& a, int B, hipStream_t s) {
    if (a.up == 1 && a.down == 1) {
        const long long gy = (long long)B * a.nch;
        ingest_kernel<T><<<dim3((unsigned)cdiv(a.n_in, RS_THREADS), (unsigned)gy), RS_THREADS, 0, s>>>(a);
        return 0;
    }
    const size_t lds = ((size_t)((a.up * a.Tp + 3) & ~3) + RS_SPAN) * sizeof(float);
    if (int rc = sed_set_max_lds<resample_kernel<T>>(lds)) return rc;
    const long long ntiles = ((long long)a.n_out + a.tile - 1) / a.tile;       // <= 2^31 / 256 tiles x 64 channels: fits the grid
    resample_kernel<T><<<dim3((unsigned)(ntiles * a.nch), (unsigned)B), RS_THREADS, lds, s>>>(a);
    return 0;
}

}  // namespace

extern "C" int sed_resample_plan(int up, int down, int* h_phase_len, int* h_tile) {
    SED_REQUIRE(up >= 1 && down >= 1 && up <= RS_MAX_RATIO && down <= RS_MAX_RATIO, "up and down must lie in 1..640");
    SED_REQUIRE(gcd_int(up, down) == 1, "up and down must be coprime");
    if (h_phase_len) *h_phase_len = taps_per_phase(up, down) | 1;
    if (h_tile) *h_tile = tile_outputs(up, down);
    return 0;
}

extern "C" int sed_resample_poly(int pcm_dtype, const void* pcm, const float* taps, float* out, int B, int n_in, int n_out, int ch_in,
                                 int ch_out, int up, int down, void* stream) {
    SED_REQUIRE(pcm_dtype == SED_PCM_I16 || pcm_dtype == SED_PCM_I32 || pcm_dtype == SED_PCM_F32, "unknown PCM dtype");
    SED_REQUIRE(up >= 1 && down >= 1 && up <= RS_MAX_RATIO && down <= RS_MAX_RATIO, "up and down must lie in 1..640");
    SED_REQUIRE(gcd_int(up, down) == 1, "up and down must be coprime");
    SED_REQUIRE(pcm != nullptr && out != nullptr, "null pointer");
    SED_REQUIRE(taps != nullptr || (up == 1 && down == 1), "null phase table");
    SED_REQUIRE(B >= 1 && B <= 65535 && n_in >= 1, "B in 1..65535 rows of at least one frame");
    SED_REQUIRE(ch_in >= 1 && ch_in <= RS_MAX_CH && ch_out >= 1 && ch_out <= RS_MAX_CH, "1..64 channels");
    const long long want = ((long long)n_in * up + down - 1) / down;
    SED_REQUIRE(want <= 0x7fffffffLL && (long long)n_out == want, "n_out must be ceil(n_in * up / down)");

    ResampleArgs a;
    a.x = pcm; a.taps = taps; a.y = out;
    a.n_in = n_in; a.n_out = n_out; a.ch_in = ch_in; a.ch_out = ch_out;
    const bool mean = ch_out == 1 || ch_in < ch_out;       // the rule of read_multichannel_audio
    a.nch = mean ? 1 : ch_out;
    a.pick_base = (mean && ch_in > 1) ? -1 : 0;
    const size_t esz = pcm_dtype == SED_PCM_I16 ? 2 : 4, fsz = esz * (size_t)ch_in;
    a.vec = (a.pick_base < 0 && (ch_in == 2 || ch_in == 4) && (uintptr_t)pcm % fsz == 0) ? ch_in : 0;
    a.up = up; a.down = down; a.half = 10 * (up > down ? up : down);
    a.T = taps_per_phase(up, down); a.Tp = a.T | 1; a.tile = tile_outputs(up, down);
    SED_REQUIRE((long long)B * a.nch <= 65535 || !(up == 1 && down == 1), "B * ch_out above 65535");

    int rc;
    if (pcm_dtype == SED_PCM_I16) rc = launch<int16_t>(a, B, (hipStream_t)stream);
    else if (pcm_dtype == SED_PCM_I32) rc = launch<int32_t>(a, B, (hipStream_t)stream);
    else rc = launch<float>(a, B, (hipStream_t)stream);
    if (rc) return rc;
    SED_LAUNCH_CHECK();
    return 0;
}
