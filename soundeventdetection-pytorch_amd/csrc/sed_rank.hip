// Corpus-level rank metrics without leaving the device: average precision, ROC-AUC (as an integer), and the best-F1 operating point
// per class, from ONE key-only segmented radix sort and one scan.  A probability is a non-negative fp32, so its bit pattern is its
// order key and its sign bit is free: key = (bits(p) << 1) | positive, below 2^31, ordered like (p, label).  Equal keys are
// indistinguishable, so the sorted row is unique; every count is an integer and AP is a fixed-shape sum: the same bits on every run.
//
// sed_rank_pack   the append step.  Reads the models' [frames][K] layout (classes innermost) and writes class-major keys at
//   keys[k][offset .. offset + n).  A workgroup takes PK_ROWS frames x up to PK_COLS classes: the read walks whole lines of the
//   [frames][K] arrays (for K <= 32 one contiguous run), the keys are transposed through LDS (row pitch PK_ROWS + 1 words: the
//   transposing write is conflict-free, the read is consecutive), and every class row is written as one PK_ROWS * 4 B run.  Scores
//   outside [0, 1] or NaN are packed as key 0 and counted in invalid[k] (one integer atomic per wave that saw one).
//
// sed_rank_sort   LSD radix sort of the first n keys of each of the K rows, four 8-bit passes (bits 0..30), ping-pong between the
//   rows and the workspace (an even number of passes: the result is back in the rows).  A pass is three launches over a grid of
//   (tiles, K), tile = RK_TILE keys:
//     histogram  per-tile digit counts (LDS integer atomics; a count, not a position) -> table[k][tile][digit];
//     scan       one workgroup of 4 x 256 threads per row: thread (g, d) sums digit d over the g-th quarter of the tiles, an
//                exclusive scan over the 256 digit totals, then the exclusive prefix in (digit, tile) order in place -- the
//                global base of every (tile, digit);
//     scatter    wave w owns keys [512 w, 512 w + 512) of the tile, eight rounds of 64.  Per-wave digit counts give each wave its
//                base inside the tile; inside a round a key's rank among the wave's equal digits comes from eight ballots (one per
//                digit bit) and a popcount below the lane: stable by construction, no atomic decides a position.  The keys go to
//                LDS in digit order first, so that the global writes of one digit are consecutive.
//
// sed_rank_curve  the walk "from the highest score down" as a suffix scan over the ascending rows.  A tie group is a maximal run of
//   equal key >> 1; inside it the negatives come first.  For the group that starts at index i: n_g = n - i, TP_g = S(i) (the
//   positives at or after i), tp_g = S(i) - S(i'), i' the next group's start (n after the last), fp_g = i' - i - tp_g,
//   TP_{g-1} = S(i').  So a group start needs (S(i), i', S(i')): an associative suffix scan of (positives, first start, positives at
//   or after that start), run inside a thread's 8 consecutive keys, across the 256 threads of a tile (LDS), and across the tiles of a
//   row (one workgroup per row) -- a group may span any number of tiles.  Four launches: tile summaries, the row scan, the terms
//   (AP in double: (tp_g / P) * (TP_g / n_g), two divisions and a product, never contracted; auc2 and the F1 comparison in 64-bit
//   integers) reduced per tile by a fixed tree, and a per-row reduction of the tile partials by a fixed tree.
#include "common.h"

namespace {

constexpr int RK_THREADS = 256;
constexpr int RK_ITEMS = 8;
constexpr int RK_TILE = RK_THREADS * RK_ITEMS;      // keys one workgroup takes per pass (sed_rank_tile)
constexpr int RK_WAVE_KEYS = RK_TILE / 4;           // keys of one of the four waves
constexpr int RK_SCAN_GROUPS = 4;                   // the table scan splits a row's tiles over this many groups of 256 threads
constexpr size_t RK_MAX_N = (size_t)1 << 30;
constexpr unsigned RK_NONE = 0xffffffffu;
constexpr int PK_ROWS = 256;
constexpr int PK_COLS = 32;

typedef unsigned long long u64;

// ---- pack ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RK_THREADS) void rank_pack_kernel(const float* __restrict__ score, const float* __restrict__ target,
                                                               size_t n, int K, unsigned* __restrict__ keys, size_t capacity,
                                                               size_t offset, u64* __restrict__ invalid) {
    __shared__ unsigned tile[PK_COLS * (PK_ROWS + 1)];
    const int tid = threadIdx.x;
    const size_t r0 = (size_t)blockIdx.x * PK_ROWS;
    const int c0 = (int)blockIdx.y * PK_COLS;
    const int kc = K - c0 < PK_COLS ? K - c0 : PK_COLS;
    const int rn = n - r0 < (size_t)PK_ROWS ? (int)(n - r0) : PK_ROWS;
    const int items = rn * kc;
    for (int i = tid; i < items; i += RK_THREADS) {
        const int r = i / kc, c = i - r * kc;
        const size_t g = (r0 + (size_t)r) * (size_t)K + (size_t)(c0 + c);
        const float p = score[g], t = target[g];
        unsigned key = RK_NONE;
        if (p >= 0.f && p <= 1.f) key = ((__float_as_uint(p) & 0x7fffffffu) << 1) | (t > 0.5f ? 1u : 0u);     // -0 -> +0
        tile[c * (PK_ROWS + 1) + r] = key;
    }
    __syncthreads();
    for (int c = 0; c < kc; ++c) {
        bool inv = false;
        if (tid < rn) {
            const unsigned key = tile[c * (PK_ROWS + 1) + tid];
            inv = key == RK_NONE;
            keys[(size_t)(c0 + c) * capacity + offset + r0 + (size_t)tid] = inv ? 0u : key;
        }
        const u64 b = __builtin_amdgcn_ballot_w64(inv);
        if (b != 0 && (tid & 63) == 0) atomicAdd(&invalid[c0 + c], (u64)__builtin_popcountll(b));
    }
}

// ---- sort ------------------------------------------------------------------------------------------------------------------------
// exclusive scan of one value per thread over the first 256 threads of the block (the others only keep the barriers company)
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned (*s)[RK_THREADS]) {
    const int tid = threadIdx.x;
    const bool on = tid < RK_THREADS;
    int cur = 0;
    if (on) s[0][tid] = v;
    __syncthreads();
    for (int off = 1; off < RK_THREADS; off <<= 1) {
        if (on) {
            unsigned x = s[cur][tid];
            if (tid >= off) x += s[cur][tid - off];
            s[cur ^ 1][tid] = x;
        }
        __syncthreads();
        cur ^= 1;
    }
    const unsigned incl = on ? s[cur][tid] : 0u;
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(RK_THREADS) void rank_hist_kernel(const unsigned* __restrict__ src, size_t stride, unsigned n,
                                                               unsigned tiles, int shift, unsigned* __restrict__ table) {
    __shared__ unsigned h[256];
    const int tid = threadIdx.x;
    const unsigned tile = blockIdx.x;
    const unsigned* __restrict__ row = src + (size_t)blockIdx.y * stride;
    const unsigned t0 = tile * (unsigned)RK_TILE;
    h[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RK_ITEMS; ++j) {
        const unsigned e = t0 + (unsigned)(j * RK_THREADS + tid);
        if (e < n) atomicAdd(&h[(row[e] >> shift) & 255u], 1u);
    }
    __syncthreads();
    table[((size_t)blockIdx.y * tiles + tile) * 256 + (size_t)tid] = h[tid];
}

// one workgroup of RK_SCAN_GROUPS x 256 threads per row: thread (g, d) owns digit d of the g-th quarter of the tiles, so a step of its
// loops reads one 1 KB line of the table with its 255 neighbours and the loops are a quarter as long
__global__ __launch_bounds__(RK_SCAN_GROUPS * 256) void rank_scan_kernel(unsigned* __restrict__ table, unsigned tiles) {
    __shared__ unsigned s[2][RK_THREADS];
    __shared__ unsigned gsum[RK_SCAN_GROUPS][256];
    const int d = threadIdx.x & 255, g = threadIdx.x >> 8;
    unsigned* row = table + (size_t)blockIdx.x * tiles * 256 + d;
    const unsigned per = (tiles + RK_SCAN_GROUPS - 1) / RK_SCAN_GROUPS;
    const unsigned lo = (unsigned)g * per < tiles ? (unsigned)g * per : tiles;
    const unsigned hi = lo + per < tiles ? lo + per : tiles;
    unsigned sum = 0;
#pragma unroll 8
    for (unsigned t = lo; t < hi; ++t) sum += row[(size_t)t * 256];
    gsum[g][d] = sum;
    __syncthreads();
    unsigned tot = 0;
    if (g == 0)
        for (int i = 0; i < RK_SCAN_GROUPS; ++i) tot += gsum[i][d];
    const unsigned ex = block_excl_scan(tot, s);          // g == 0: where digit d starts in the sorted row
    if (g == 0) s[0][d] = ex;
    __syncthreads();
    unsigned acc = s[0][d];
    for (int i = 0; i < g; ++i) acc += gsum[i][d];
#pragma unroll 8
    for (unsigned t = lo; t < hi; ++t) {
        const unsigned c = row[(size_t)t * 256];
        row[(size_t)t * 256] = acc;
        acc += c;
    }
}

__global__ __launch_bounds__(RK_THREADS) void rank_scatter_kernel(const unsigned* __restrict__ src, size_t src_stride,
                                                                  unsigned* __restrict__ dst, size_t dst_stride, unsigned n,
                                                                  unsigned tiles, int shift, const unsigned* __restrict__ table) {
    __shared__ unsigned wbase[4][256];          // per-wave digit counts, then each wave's running position inside the tile
    __shared__ unsigned sc[2][RK_THREADS];
    __shared__ unsigned lstart[256];            // where a digit starts inside the sorted tile
    __shared__ unsigned gbase[256];             // where this tile's keys of a digit start in the destination row
    __shared__ unsigned sorted[RK_TILE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned tile = blockIdx.x;
    const unsigned* __restrict__ row = src + (size_t)blockIdx.y * src_stride;
    unsigned* __restrict__ out = dst + (size_t)blockIdx.y * dst_stride;
    const unsigned t0 = tile * (unsigned)RK_TILE;
    const unsigned tn = n - t0 < (unsigned)RK_TILE ? n - t0 : (unsigned)RK_TILE;
#pragma unroll
    for (int w = 0; w < 4; ++w) wbase[w][tid] = 0;
    __syncthreads();
    unsigned key[RK_ITEMS];
#pragma unroll
    for (int j = 0; j < RK_ITEMS; ++j) {
        const unsigned el = (unsigned)(wave * RK_WAVE_KEYS + j * 64 + lane);
        key[j] = el < tn ? row[t0 + el] : 0u;
        if (el < tn) atomicAdd(&wbase[wave][(key[j] >> shift) & 255u], 1u);
    }
    __syncthreads();
    {
        const unsigned c0 = wbase[0][tid], c1 = wbase[1][tid], c2 = wbase[2][tid], c3 = wbase[3][tid];
        const unsigned ex = block_excl_scan(c0 + c1 + c2 + c3, sc);
        lstart[tid] = ex;
        gbase[tid] = table[((size_t)blockIdx.y * tiles + tile) * 256 + (size_t)tid];
        wbase[0][tid] = ex;
        wbase[1][tid] = ex + c0;
        wbase[2][tid] = ex + c0 + c1;
        wbase[3][tid] = ex + c0 + c1 + c2;
    }
    __syncthreads();
    const u64 below = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < RK_ITEMS; ++j) {
        const unsigned el = (unsigned)(wave * RK_WAVE_KEYS + j * 64 + lane);
        const bool valid = el < tn;
        const unsigned d = (key[j] >> shift) & 255u;
        u64 same = __builtin_amdgcn_ballot_w64(valid);        // the lanes of this round that hold the same digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = ((d >> b) & 1u) != 0;
            const u64 bal = __builtin_amdgcn_ballot_w64(bit);
            same &= bit ? bal : ~bal;
        }
        const unsigned rank = (unsigned)__builtin_popcountll(same & below);
        const unsigned cnt = (unsigned)__builtin_popcountll(same);
        const unsigned base = valid ? wbase[wave][d] : 0u;
        if (valid) sorted[base + rank] = key[j];
        __syncthreads();
        if (valid && rank == 0) wbase[wave][d] = base + cnt;
        __syncthreads();
    }
    for (unsigned i = (unsigned)tid; i < tn; i += RK_THREADS) {
        const unsigned kv = sorted[i];
        const unsigned d = (kv >> shift) & 255u;
        out[gbase[d] + (i - lstart[d])] = kv;
    }
}

// ---- curve -----------------------------------------------------------------------------------------------------------------------
// what a range of an ascending row tells the ranges on its left: its positives, its first (lowest) group start, the positives at or
// after that start, and its number of group starts.  first == RK_NONE: the range holds no start.
struct Agg {
    unsigned sum, first, pge, cnt;
};
__device__ __forceinline__ Agg agg_none() { return Agg{0u, RK_NONE, 0u, 0u}; }
__device__ __forceinline__ Agg combine(const Agg& l, const Agg& r) {
    Agg o;
    o.sum = l.sum + r.sum;
    o.cnt = l.cnt + r.cnt;
    const bool has = l.first != RK_NONE;
    o.first = has ? l.first : r.first;
    o.pge = has ? l.pge + r.sum : r.pge;
    return o;
}

// suffix scan over the block's 256 threads: excl = everything to the right of this thread, total = the whole block
__device__ __forceinline__ void block_suffix_scan(const Agg& v, unsigned (*s)[4][RK_THREADS], Agg& excl, Agg& total) {
    const int tid = threadIdx.x;
    int cur = 0;
    s[0][0][tid] = v.sum; s[0][1][tid] = v.first; s[0][2][tid] = v.pge; s[0][3][tid] = v.cnt;
    __syncthreads();
    for (int off = 1; off < RK_THREADS; off <<= 1) {
        Agg x = Agg{s[cur][0][tid], s[cur][1][tid], s[cur][2][tid], s[cur][3][tid]};
        if (tid + off < RK_THREADS) {
            const int o = tid + off;
            x = combine(x, Agg{s[cur][0][o], s[cur][1][o], s[cur][2][o], s[cur][3][o]});
        }
        s[cur ^ 1][0][tid] = x.sum; s[cur ^ 1][1][tid] = x.first; s[cur ^ 1][2][tid] = x.pge; s[cur ^ 1][3][tid] = x.cnt;
        __syncthreads();
        cur ^= 1;
    }
    total = Agg{s[cur][0][0], s[cur][1][0], s[cur][2][0], s[cur][3][0]};
    excl = agg_none();
    if (tid + 1 < RK_THREADS) excl = Agg{s[cur][0][tid + 1], s[cur][1][tid + 1], s[cur][2][tid + 1], s[cur][3][tid + 1]};
    __syncthreads();
}

// a thread's 8 consecutive keys of the tile and the key before them (v[0]); keys past n read as 0 and are never used
__device__ __forceinline__ void load_run(const unsigned* __restrict__ row, unsigned e0, unsigned n, unsigned (&v)[RK_ITEMS + 1]) {
    v[0] = (e0 > 0 && e0 - 1 < n) ? row[e0 - 1] : 0u;
#pragma unroll
    for (int j = 0; j < RK_ITEMS; ++j) v[j + 1] = e0 + (unsigned)j < n ? row[e0 + (unsigned)j] : 0u;
}
__device__ __forceinline__ bool starts_group(const unsigned (&v)[RK_ITEMS + 1], unsigned e0, int j) {
    return (e0 + (unsigned)j == 0) || ((v[j] >> 1) != (v[j + 1] >> 1));
}
__device__ __forceinline__ Agg run_agg(const unsigned (&v)[RK_ITEMS + 1], unsigned e0, unsigned n) {
    Agg a = agg_none();
#pragma unroll
    for (int j = RK_ITEMS - 1; j >= 0; --j) {
        const unsigned e = e0 + (unsigned)j;
        if (e < n) {
            a.sum += v[j + 1] & 1u;
            if (starts_group(v, e0, j)) { a.first = e; a.pge = a.sum; a.cnt += 1; }
        }
    }
    return a;
}

__global__ __launch_bounds__(RK_THREADS) void rank_summary_kernel(const unsigned* __restrict__ keys, size_t capacity, unsigned n,
                                                                  unsigned tiles, sed_u32x4* __restrict__ tsum) {
    __shared__ unsigned s[2][4][RK_THREADS];
    const unsigned* __restrict__ row = keys + (size_t)blockIdx.y * capacity;
    const unsigned e0 = blockIdx.x * (unsigned)RK_TILE + (unsigned)threadIdx.x * RK_ITEMS;
    unsigned v[RK_ITEMS + 1];
    load_run(row, e0, n, v);
    Agg excl, total;
    block_suffix_scan(run_agg(v, e0, n), s, excl, total);
    if (threadIdx.x == 0) tsum[(size_t)blockIdx.y * tiles + blockIdx.x] = sed_u32x4{total.sum, total.first, total.pge, total.cnt};
}

// per row: carry[t] = what the tiles right of t hold, the end of the row counting as a start at n with nothing after it
__global__ __launch_bounds__(RK_THREADS) void rank_rowscan_kernel(const sed_u32x4* __restrict__ tsum, sed_u32x4* __restrict__ tcarry,
                                                                  unsigned* __restrict__ rowinfo, unsigned n, unsigned tiles) {
    __shared__ unsigned s[2][4][RK_THREADS];
    const int tid = threadIdx.x;
    const sed_u32x4* __restrict__ in = tsum + (size_t)blockIdx.x * tiles;
    sed_u32x4* __restrict__ out = tcarry + (size_t)blockIdx.x * tiles;
    const unsigned per = (tiles + RK_THREADS - 1) / RK_THREADS;
    const u64 lo64 = (u64)tid * per, hi64 = lo64 + per;
    const unsigned lo = lo64 < tiles ? (unsigned)lo64 : tiles, hi = hi64 < tiles ? (unsigned)hi64 : tiles;
    Agg a = agg_none();
    for (unsigned t = hi; t > lo; --t) {
        const sed_u32x4 q = in[t - 1];
        a = combine(Agg{q[0], q[1], q[2], q[3]}, a);
    }
    Agg excl, total;
    block_suffix_scan(a, s, excl, total);
    const Agg end = Agg{0u, n, 0u, 0u};
    Agg c = combine(excl, end);
    for (unsigned t = hi; t > lo; --t) {
        out[t - 1] = sed_u32x4{c.sum, c.first, c.pge, 0u};
        const sed_u32x4 q = in[t - 1];
        c = combine(Agg{q[0], q[1], q[2], q[3]}, c);
    }
    if (tid == 0) {
        rowinfo[2 * (size_t)blockIdx.x] = total.sum;          // P
        rowinfo[2 * (size_t)blockIdx.x + 1] = total.cnt;      // tie groups
    }
}

// the operating point (TP, npred) with the larger F1 = 2 TP / (npred + P), by cross-multiplication (TP <= 2^30, npred + P <= 2^31);
// equal F1: the higher score, i.e. the smaller npred.  npred == 0: no candidate.
__device__ __forceinline__ bool better_point(unsigned tp_a, unsigned n_a, unsigned tp_b, unsigned n_b, unsigned P) {
    if (n_a == 0) return false;
    if (n_b == 0) return true;
    const u64 l = (u64)tp_a * ((u64)n_b + P), r = (u64)tp_b * ((u64)n_a + P);
    return l > r || (l == r && n_a < n_b);
}

struct Part {
    double ap;
    u64 auc;
    unsigned btp, bn;
};

// fixed-shape tree over the block's 256 threads; the result is valid in thread 0
__device__ __forceinline__ Part block_reduce_part(Part p, unsigned P, double* sa, u64* su, unsigned* st, unsigned* sn) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    sa[tid] = p.ap; su[tid] = p.auc; st[tid] = p.btp; sn[tid] = p.bn;
    __syncthreads();
    for (int h = RK_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            sa[tid] = sa[tid] + sa[tid + h];
            su[tid] = su[tid] + su[tid + h];
            if (better_point(st[tid + h], sn[tid + h], st[tid], sn[tid], P)) { st[tid] = st[tid + h]; sn[tid] = sn[tid + h]; }
        }
        __syncthreads();
    }
    Part o = Part{sa[0], su[0], st[0], sn[0]};
    __syncthreads();
    return o;
}

__global__ __launch_bounds__(RK_THREADS) void rank_terms_kernel(const unsigned* __restrict__ keys, size_t capacity, unsigned n,
                                                                unsigned tiles, const sed_u32x4* __restrict__ tcarry,
                                                                const unsigned* __restrict__ rowinfo, double* __restrict__ tile_ap,
                                                                u64* __restrict__ tile_auc, unsigned* __restrict__ tile_best) {
#pragma clang fp contract(off)
    __shared__ unsigned s[2][4][RK_THREADS];
    __shared__ double sa[RK_THREADS];
    __shared__ u64 su[RK_THREADS];
    __shared__ unsigned st[RK_THREADS], sn[RK_THREADS];
    const unsigned* __restrict__ row = keys + (size_t)blockIdx.y * capacity;
    const unsigned e0 = blockIdx.x * (unsigned)RK_TILE + (unsigned)threadIdx.x * RK_ITEMS;
    const size_t slot = (size_t)blockIdx.y * tiles + blockIdx.x;
    const unsigned P = rowinfo[2 * (size_t)blockIdx.y];
    unsigned v[RK_ITEMS + 1];
    load_run(row, e0, n, v);
    Agg excl, total;
    block_suffix_scan(run_agg(v, e0, n), s, excl, total);
    const sed_u32x4 q = tcarry[slot];
    const Agg c = combine(excl, Agg{q[0], q[1], q[2], 0u});
    unsigned right = c.sum, next = c.first, snext = c.pge;      // S(e + 1), the next group's start i', S(i')
    Part p = Part{0.0, 0ull, 0u, 0u};
    const double dP = (double)P;
#pragma unroll
    for (int j = RK_ITEMS - 1; j >= 0; --j) {
        const unsigned e = e0 + (unsigned)j;
        if (e < n) {
            const unsigned S = right + (v[j + 1] & 1u);
            if (starts_group(v, e0, j)) {
                const unsigned tp = S - snext, fp = (next - e) - tp, ng = n - e;
                if (tp != 0) {
                    const double a = (double)tp / dP;
                    const double b = (double)S / (double)ng;
                    const double term = a * b;
                    p.ap = p.ap + term;
                }
                p.auc += (u64)fp * (2ull * (u64)snext + (u64)tp);
                if (better_point(S, ng, p.btp, p.bn, P)) { p.btp = S; p.bn = ng; }
                next = e;
                snext = S;
            }
            right = S;
        }
    }
    const Part o = block_reduce_part(p, P, sa, su, st, sn);
    if (threadIdx.x == 0) {
        tile_ap[slot] = o.ap;
        tile_auc[slot] = o.auc;
        tile_best[2 * slot] = o.btp;
        tile_best[2 * slot + 1] = o.bn;
    }
}

__global__ __launch_bounds__(RK_THREADS) void rank_finish_kernel(const unsigned* __restrict__ keys, size_t capacity, unsigned n,
                                                                 unsigned tiles, const unsigned* __restrict__ rowinfo,
                                                                 const double* __restrict__ tile_ap, const u64* __restrict__ tile_auc,
                                                                 const unsigned* __restrict__ tile_best, double* __restrict__ ap,
                                                                 u64* __restrict__ counts, float* __restrict__ best_score) {
#pragma clang fp contract(off)
    __shared__ double sa[RK_THREADS];
    __shared__ u64 su[RK_THREADS];
    __shared__ unsigned st[RK_THREADS], sn[RK_THREADS];
    const int k = blockIdx.x;
    const unsigned P = tiles ? rowinfo[2 * (size_t)k] : 0u;
    const unsigned groups = tiles ? rowinfo[2 * (size_t)k + 1] : 0u;
    Part p = Part{0.0, 0ull, 0u, 0u};
    for (unsigned t = threadIdx.x; t < tiles; t += RK_THREADS) {
        const size_t slot = (size_t)k * tiles + t;
        p.ap = p.ap + tile_ap[slot];
        p.auc += tile_auc[slot];
        if (better_point(tile_best[2 * slot], tile_best[2 * slot + 1], p.btp, p.bn, P)) {
            p.btp = tile_best[2 * slot];
            p.bn = tile_best[2 * slot + 1];
        }
    }
    const Part o = block_reduce_part(p, P, sa, su, st, sn);
    if (threadIdx.x == 0) {
        u64* c = counts + 6 * (size_t)k;
        c[0] = P; c[1] = n; c[2] = o.auc; c[5] = groups;
        if (P == 0) {                          // no positive: AP undefined, the empty decision p >= 1 scores nothing
            ap[k] = __longlong_as_double(0x7ff8000000000000ll);
            c[3] = 0; c[4] = 0;
            best_score[k] = 1.0f;
        } else {
            ap[k] = o.ap;
            c[3] = o.btp; c[4] = o.bn;
            best_score[k] = __uint_as_float(keys[(size_t)k * capacity + (size_t)(n - o.bn)] >> 1);
        }
    }
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline bool rank_shape_ok(int K, size_t n) { return K >= 1 && K <= 65535 && n <= RK_MAX_N; }
inline size_t rank_tiles(size_t n) { return (n + RK_TILE - 1) / RK_TILE; }

// workspace of the sort: the second key buffer [K][n], then the (tile, digit) table [K][tiles][256]
inline size_t sort_table_offset(int K, size_t n) { return align256((size_t)K * n * sizeof(unsigned)); }
inline size_t sort_ws_bytes(int K, size_t n) { return sort_table_offset(K, n) + (size_t)K * 256 * rank_tiles(n) * sizeof(unsigned); }
// workspace of the curve, per (row, tile) slot: summary (16), carry (16), AP partial (8), auc2 partial (8), best point (8); then [K][2]
inline size_t curve_ws_bytes(int K, size_t n) { return align256((size_t)K * rank_tiles(n) * 56) + (size_t)K * 8; }

}  // namespace

extern "C" int sed_rank_tile(void) { return RK_TILE; }

extern "C" size_t sed_rank_ws_bytes(int K, size_t n) {
    if (!rank_shape_ok(K, n)) return 0;
    const size_t a = sort_ws_bytes(K, n), b = curve_ws_bytes(K, n);
    return align256((a > b ? a : b) + 1);
}

extern "C" int sed_rank_pack(const float* score, const float* target, size_t n_score, size_t n_tgt, int K, unsigned* keys,
                             size_t capacity, size_t offset, unsigned long long* invalid, void* stream) {
    const size_t n = n_score < n_tgt ? n_score : n_tgt;
    SED_REQUIRE(rank_shape_ok(K, n), "K in 1..65535, min(n_score, n_tgt) <= 2^30");
    SED_REQUIRE(offset <= capacity && n <= capacity - offset, "offset + n exceeds the capacity of a key row");
    SED_REQUIRE(capacity <= RK_MAX_N, "capacity <= 2^30");
    if (n == 0) return 0;
    SED_REQUIRE(score != nullptr && target != nullptr && keys != nullptr && invalid != nullptr, "null pointer");
    const dim3 grid((unsigned)cdivz(n, PK_ROWS), (unsigned)cdiv(K, PK_COLS));
    rank_pack_kernel<<<grid, RK_THREADS, 0, (hipStream_t)stream>>>(score, target, n, K, keys, capacity, offset, invalid);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_rank_sort(unsigned* keys, int K, size_t n, size_t capacity, void* workspace, void* stream) {
    SED_REQUIRE(rank_shape_ok(K, n), "K in 1..65535, n <= 2^30");
    SED_REQUIRE(n <= capacity, "n exceeds the capacity of a key row");
    if (n == 0) return 0;
    SED_REQUIRE(keys != nullptr && workspace != nullptr, "null pointer");
    SED_REQUIRE(((uintptr_t)workspace & 15) == 0, "the workspace must be 16-byte aligned");
    unsigned* alt = reinterpret_cast<unsigned*>(workspace);
    unsigned* table = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(workspace) + sort_table_offset(K, n));
    const unsigned tiles = (unsigned)rank_tiles(n);
    const dim3 grid(tiles, (unsigned)K);
    hipStream_t st = (hipStream_t)stream;
    for (int pass = 0; pass < 4; ++pass) {
        const bool fwd = (pass & 1) == 0;               // even passes: rows -> workspace; odd: back
        const unsigned* src = fwd ? keys : alt;
        unsigned* dst = fwd ? alt : keys;
        const size_t ss = fwd ? capacity : n, ds = fwd ? n : capacity;
        rank_hist_kernel<<<grid, RK_THREADS, 0, st>>>(src, ss, (unsigned)n, tiles, 8 * pass, table);
        SED_LAUNCH_CHECK();
        rank_scan_kernel<<<(unsigned)K, RK_SCAN_GROUPS * 256, 0, st>>>(table, tiles);
        SED_LAUNCH_CHECK();
        rank_scatter_kernel<<<grid, RK_THREADS, 0, st>>>(src, ss, dst, ds, (unsigned)n, tiles, 8 * pass, table);
        SED_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int sed_rank_curve(const unsigned* keys_sorted, int K, size_t n, size_t capacity, double* ap, unsigned long long* counts,
                              float* best_score, void* workspace, void* stream) {
    SED_REQUIRE(rank_shape_ok(K, n), "K in 1..65535, n <= 2^30");
    SED_REQUIRE(n <= capacity, "n exceeds the capacity of a key row");
    SED_REQUIRE(ap != nullptr && counts != nullptr && best_score != nullptr, "null pointer");
    SED_REQUIRE(n == 0 || (keys_sorted != nullptr && workspace != nullptr), "null pointer");
    SED_REQUIRE(((uintptr_t)workspace & 15) == 0, "the workspace must be 16-byte aligned");
    const unsigned tiles = (unsigned)rank_tiles(n);
    const size_t slots = (size_t)K * tiles;
    char* w = reinterpret_cast<char*>(workspace);
    sed_u32x4* tsum = nullptr;
    sed_u32x4* tcarry = nullptr;
    double* tile_ap = nullptr;
    u64* tile_auc = nullptr;
    unsigned* tile_best = nullptr;
    unsigned* rowinfo = nullptr;
    if (n > 0) {
        tsum = reinterpret_cast<sed_u32x4*>(w);
        tcarry = reinterpret_cast<sed_u32x4*>(w + slots * 16);
        tile_ap = reinterpret_cast<double*>(w + slots * 32);
        tile_auc = reinterpret_cast<u64*>(w + slots * 40);
        tile_best = reinterpret_cast<unsigned*>(w + slots * 48);
        rowinfo = reinterpret_cast<unsigned*>(w + align256(slots * 56));
    }
    hipStream_t st = (hipStream_t)stream;
    if (n > 0) {
        const dim3 grid(tiles, (unsigned)K);
        rank_summary_kernel<<<grid, RK_THREADS, 0, st>>>(keys_sorted, capacity, (unsigned)n, tiles, tsum);
        SED_LAUNCH_CHECK();
        rank_rowscan_kernel<<<(unsigned)K, RK_THREADS, 0, st>>>(tsum, tcarry, rowinfo, (unsigned)n, tiles);
        SED_LAUNCH_CHECK();
        rank_terms_kernel<<<grid, RK_THREADS, 0, st>>>(keys_sorted, capacity, (unsigned)n, tiles, tcarry, rowinfo, tile_ap, tile_auc,
                                                      tile_best);
        SED_LAUNCH_CHECK();
    }
    // n == 0: the finishing kernel reads nothing and writes the empty row's values
    rank_finish_kernel<<<(unsigned)K, RK_THREADS, 0, st>>>(keys_sorted, capacity, (unsigned)n, tiles, rowinfo, tile_ap, tile_auc,
                                                          tile_best, ap, counts, best_score);
    SED_LAUNCH_CHECK();
    return 0;
}
