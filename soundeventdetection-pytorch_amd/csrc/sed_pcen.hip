// Per-channel energy normalisation (PCEN; Wang et al., ICASSP 2017; for sound event detection Lostanlen et al. 2019) as a trainable
// front-end layer: forward and backward over x fp32 [B][T][F], the models' (B, 1, T, F) layout, mel bins innermost.
//
// Definition (include/sed_hip.h has the same text).  theta fp32 [4][F] = (a, d, rho, sigma) per bin:
//   alpha = e^a, delta = e^d, r = e^rho, s = 1 / (1 + e^-sigma);  two double constants eps > 0, gain > 0.
//   E_t = gain * 10^((x_t std_f + mean_f) / 10)     kind 0: dB log-mel; mean / std NULL = 0 / 1
//   E_t = gain * max(x_t, 0)                        kind 1: linear mel power
//   M_0 = E_0;  M_t = (1 - s) M_{t-1} + s E_t
//   u_t = eps + M_t;  G_t = E_t u_t^-alpha;  y_t = (G_t + delta)^r - delta^r
// Backward, g = dL/dy:
//   q_t = g_t r (G_t + delta)^(r-1);  direct_t = q_t u_t^-alpha;  m_t = -q_t alpha G_t / u_t
//   lambda_t = m_t + (1 - s) lambda_{t+1}, lambda_T = 0
//   dE_t = direct_t + s lambda_t (t >= 1);  dE_0 = direct_0 + lambda_0
//   dx_t = dE_t E_t (ln 10 / 10) std_f (kind 0);  gain dE_t [x_t > 0] (kind 1)
//   da = alpha sum -q_t G_t ln u_t
//   dd = delta sum g_t r ((G_t + delta)^(r-1) - delta^(r-1))
//   drho = r sum g_t ((G_t + delta)^r ln(G_t + delta) - delta^r ln delta)
//   dsigma = s (1 - s) sum_{t >= 1} lambda_t (E_t - M_{t-1})            (sums over b and t)
//
// Arithmetic: everything is double and every output is rounded once to fp32.  A power p^e is taken as exp(e ln p), both in
// double, so that the logarithm the parameter gradients need anyway is computed once; 10^(v/10) is exp(v ln 10 / 10).  M is
// never stored as a tensor: the backward rebuilds it from x and needs nothing a forward left behind.
//
// Time is parallel.  A thread per bin walking all T frames would be B F threads (2048 at (32, 6001, 64)); instead the frames are cut
// into chunks of PC_CHUNK and a thread owns one (b, chunk, f), f fastest, so that the 64 lanes of a wave read 64 neighbouring bins
// of one frame.  Both recurrences are first order and linear with the constant factor 1 - s, hence
//   forward   launch 1: L[b][c][f] = the smoother at the chunk's last frame when it enters the chunk as 0 (chunk 0 starts at E_0)
//             launch 2: the state entering chunk c is S_c = (1-s)^PC_CHUNK S_{c-1} + L[c-1], S_0 = 0, which each thread folds from
//                       L[0 .. c) in that fixed order; then it walks its chunk and writes y
//   backward  launch 1: L as above
//             launch 2: carry as above, walk the chunk, R[b][c][f] = sum_t (1-s)^(t - t0) m_t = lambda at the chunk's first frame
//                       when it enters the chunk (from the right) as 0
//             launch 3: carry as above, the walk again with M_t kept in LDS (PC_CHUNK doubles per thread), the state entering from
//                       the right folded from R(c .. nc) in fixed order, then the walk in reverse: lambda, dx, and the four
//                       parameter sums of this (b, chunk, f) into part[b nc + c][4][f]
//             launch 4: dtheta[j][f] = factor * sum over rows of part, 16 interleaved slices summed in row order and the 16 slice
//                       sums in slice order (only with dtheta)
// The carries go through the workspace between launches; no workgroup waits on another inside a launch.  No floating-point atomics:
// the same input gives the same bits on every run.  dx == NULL or dtheta == NULL skips the stores, not the arithmetic, so that the
// other output keeps its bits.
#include <math.h>

#include "common.h"

namespace {

constexpr int PC_CHUNK = 32;          // frames per time chunk (sed_pcen_chunk)
constexpr int PC_THREADS = 128;       // LDS of launch 3: PC_CHUNK * PC_THREADS doubles = 32 KB
constexpr int PC_MAX_F = 256;
constexpr int PC_RED_SLICES = 16;
constexpr double PC_LN10_10 = 0.23025850929940456840;      // ln 10 / 10

struct PcenArgs {
    const float* x;
    const float* mean;
    const float* std;
    const float* theta;
    int kind;
    double eps, gain;
    int B, T, F, nc;
    size_t n;                 // B * nc * F threads
};

// the per-bin constants
struct PcenBin {
    double alpha, delta, r, s, a;      // a = 1 - s
    double aC;                         // a^PC_CHUNK
    double sc, sh;                     // kind 0: the exponent is (x sc + sh) ln 10 / 10
};

__device__ __forceinline__ PcenBin pcen_bin(const PcenArgs& A, int f) {
    PcenBin p;
    p.alpha = exp((double)A.theta[f]);
    p.delta = exp((double)A.theta[A.F + f]);
    p.r = exp((double)A.theta[2 * A.F + f]);
    p.s = 1.0 / (1.0 + exp(-(double)A.theta[3 * A.F + f]));
    p.a = 1.0 - p.s;
    double w = 1.0;
    for (int i = 0; i < PC_CHUNK; ++i) w *= p.a;
    p.aC = w;
    p.sc = A.std != nullptr ? (double)A.std[f] : 1.0;
    p.sh = A.mean != nullptr ? (double)A.mean[f] : 0.0;
    return p;
}

__device__ __forceinline__ double pcen_energy(const PcenArgs& A, const PcenBin& p, float xv) {
    if (A.kind == 0) return A.gain * exp(((double)xv * p.sc + p.sh) * PC_LN10_10);
    return A.gain * fmax((double)xv, 0.0);
}

// thread -> (b, c, f), the chunk's frames [t0, t1) and the offset of x[b][t0][f]
struct PcenWho {
    int b, c, f, t0, t1;
    size_t off, row;          // row = b * nc + c
};

__device__ __forceinline__ bool pcen_who(const PcenArgs& A, PcenWho& w) {
    const size_t id = (size_t)blockIdx.x * PC_THREADS + threadIdx.x;
    if (id >= A.n) return false;
    w.f = (int)(id % (size_t)A.F);
    w.row = id / (size_t)A.F;
    w.c = (int)(w.row % (size_t)A.nc);
    w.b = (int)(w.row / (size_t)A.nc);
    w.t0 = w.c * PC_CHUNK;
    w.t1 = w.t0 + PC_CHUNK < A.T ? w.t0 + PC_CHUNK : A.T;
    w.off = ((size_t)w.b * (size_t)A.T + (size_t)w.t0) * (size_t)A.F + (size_t)w.f;
    return true;
}

// the smoother's state entering chunk c: S_0 = 0, S_{k+1} = a^PC_CHUNK S_k + L[k]
__device__ __forceinline__ double pcen_carry(const PcenArgs& A, const PcenWho& w, const PcenBin& p, const double* __restrict__ Ls) {
    const double* __restrict__ lp = Ls + ((size_t)w.b * (size_t)A.nc) * (size_t)A.F + (size_t)w.f;
    double S = 0.0;
    for (int k = 0; k < w.c; ++k) S = p.aC * S + lp[(size_t)k * (size_t)A.F];
    return S;
}

// launch 1 of both directions
__global__ __launch_bounds__(PC_THREADS) void pcen_local_kernel(PcenArgs A, double* __restrict__ Ls) {
    PcenWho w;
    if (!pcen_who(A, w)) return;
    const PcenBin p = pcen_bin(A, w.f);
    const float* __restrict__ xp = A.x + w.off;
    double M = 0.0;
    for (int t = w.t0; t < w.t1; ++t) {
        const double E = pcen_energy(A, p, xp[(size_t)(t - w.t0) * (size_t)A.F]);
        M = t == 0 ? E : p.a * M + p.s * E;
    }
    Ls[w.row * (size_t)A.F + (size_t)w.f] = M;
}

__global__ __launch_bounds__(PC_THREADS) void pcen_fwd_kernel(PcenArgs A, const double* __restrict__ Ls, float* __restrict__ y) {
    PcenWho w;
    if (!pcen_who(A, w)) return;
    const PcenBin p = pcen_bin(A, w.f);
    const float* __restrict__ xp = A.x + w.off;
    float* __restrict__ yp = y + w.off;
    const double dr = exp(p.r * log(p.delta));
    double M = pcen_carry(A, w, p, Ls);
    for (int t = w.t0; t < w.t1; ++t) {
        const size_t o = (size_t)(t - w.t0) * (size_t)A.F;
        const double E = pcen_energy(A, p, xp[o]);
        M = t == 0 ? E : p.a * M + p.s * E;
        const double lnu = log(A.eps + M);
        const double G = E * exp(-p.alpha * lnu);
        yp[o] = (float)(exp(p.r * log(G + p.delta)) - dr);
    }
}

// what both backward walks need of one frame, from E_t, M_t and g_t: the same expressions in both, so the same bits
struct PcenPoint {
    double u, lnu, upa, G, Gd, lnGd, Gdr1, q, m;
};

__device__ __forceinline__ PcenPoint pcen_point(const PcenArgs& A, const PcenBin& p, double E, double M, double g) {
    PcenPoint k;
    k.u = A.eps + M;
    k.lnu = log(k.u);
    k.upa = exp(-p.alpha * k.lnu);
    k.G = E * k.upa;
    k.Gd = k.G + p.delta;
    k.lnGd = log(k.Gd);
    k.Gdr1 = exp((p.r - 1.0) * k.lnGd);
    k.q = g * p.r * k.Gdr1;
    k.m = -k.q * p.alpha * k.G / k.u;
    return k;
}

// backward launch 2: R[b][c][f] = sum_t a^(t - t0) m_t
__global__ __launch_bounds__(PC_THREADS) void pcen_bwd_local_kernel(PcenArgs A, const float* __restrict__ gy, const double* __restrict__ Ls,
                                                                    double* __restrict__ Rs) {
    PcenWho w;
    if (!pcen_who(A, w)) return;
    const PcenBin p = pcen_bin(A, w.f);
    const float* __restrict__ xp = A.x + w.off;
    const float* __restrict__ gp = gy + w.off;
    double M = pcen_carry(A, w, p, Ls);
    double R = 0.0, pw = 1.0;
    for (int t = w.t0; t < w.t1; ++t) {
        const size_t o = (size_t)(t - w.t0) * (size_t)A.F;
        const double E = pcen_energy(A, p, xp[o]);
        M = t == 0 ? E : p.a * M + p.s * E;
        const PcenPoint k = pcen_point(A, p, E, M, (double)gp[o]);
        R += pw * k.m;
        pw *= p.a;
    }
    Rs[w.row * (size_t)A.F + (size_t)w.f] = R;
}

// backward launch 3
__global__ __launch_bounds__(PC_THREADS) void pcen_bwd_apply_kernel(PcenArgs A, const float* __restrict__ gy, const double* __restrict__ Ls,
                                                                    const double* __restrict__ Rs, float* __restrict__ dx,
                                                                    double* __restrict__ part) {
    __shared__ double Ms[PC_CHUNK][PC_THREADS];     // M_t of this thread's chunk; column threadIdx.x only: no barrier needed
    PcenWho w;
    if (!pcen_who(A, w)) return;
    const int tid = threadIdx.x;
    const PcenBin p = pcen_bin(A, w.f);
    const float* __restrict__ xp = A.x + w.off;
    const float* __restrict__ gp = gy + w.off;
    const double S = pcen_carry(A, w, p, Ls);
    double M = S;
    for (int t = w.t0; t < w.t1; ++t) {
        const double E = pcen_energy(A, p, xp[(size_t)(t - w.t0) * (size_t)A.F]);
        M = t == 0 ? E : p.a * M + p.s * E;
        Ms[t - w.t0][tid] = M;
    }
    // lambda entering from the right: Lam_{nc-1} = 0, Lam_{k-1} = R[k] + a^PC_CHUNK Lam_k
    double lam = 0.0;
    {
        const double* __restrict__ rp = Rs + ((size_t)w.b * (size_t)A.nc) * (size_t)A.F + (size_t)w.f;
        for (int k = A.nc - 1; k > w.c; --k) lam = rp[(size_t)k * (size_t)A.F] + p.aC * lam;
    }
    const double lnd = log(p.delta);
    const double dr = exp(p.r * lnd), dr1 = exp((p.r - 1.0) * lnd);
    double pa = 0.0, pd = 0.0, pr = 0.0, ps = 0.0;
    for (int t = w.t1 - 1; t >= w.t0; --t) {
        const int i = t - w.t0;
        const size_t o = (size_t)i * (size_t)A.F;
        const float xv = xp[o];
        const double g = (double)gp[o];
        const double E = pcen_energy(A, p, xv);
        const double Mt = Ms[i][tid];
        const double Mprev = i > 0 ? Ms[i - 1][tid] : S;
        const PcenPoint k = pcen_point(A, p, E, Mt, g);
        lam = k.m + p.a * lam;
        const double dE = k.q * k.upa + (t == 0 ? lam : p.s * lam);
        if (dx != nullptr) {
            float v;
            if (A.kind == 0) v = (float)(dE * E * PC_LN10_10 * p.sc);
            else v = xv > 0.f ? (float)(A.gain * dE) : 0.f;
            dx[w.off + o] = v;
        }
        pa += -k.q * k.G * k.lnu;
        pd += g * p.r * (k.Gdr1 - dr1);
        pr += g * (exp(p.r * k.lnGd) * k.lnGd - dr * lnd);
        if (t >= 1) ps += lam * (E - Mprev);
    }
    if (part != nullptr) {
        double* __restrict__ pp = part + w.row * (size_t)(4 * A.F) + (size_t)w.f;
        pp[0] = pa;
        pp[(size_t)A.F] = pd;
        pp[(size_t)2 * A.F] = pr;
        pp[(size_t)3 * A.F] = ps;
    }
}

// backward launch 4: block (64 bins, PC_RED_SLICES), grid (ceil(F / 64), 4 parameters)
__global__ __launch_bounds__(64 * PC_RED_SLICES) void pcen_reduce_kernel(const double* __restrict__ part, const float* __restrict__ theta,
                                                                         size_t rows, int F, float* __restrict__ dtheta) {
    __shared__ double sl[PC_RED_SLICES][64];
    const int lane = threadIdx.x, sidx = threadIdx.y, j = blockIdx.y;
    const int f = blockIdx.x * 64 + lane;
    double acc = 0.0;
    if (f < F)
        for (size_t r = (size_t)sidx; r < rows; r += PC_RED_SLICES) acc += part[(r * 4 + (size_t)j) * (size_t)F + (size_t)f];
    sl[sidx][lane] = acc;
    __syncthreads();
    if (sidx != 0 || f >= F) return;
    double tot = 0.0;
    for (int k = 0; k < PC_RED_SLICES; ++k) tot += sl[k][lane];
    double fac;
    if (j == 3) {
        const double s = 1.0 / (1.0 + exp(-(double)theta[3 * F + f]));
        fac = s * (1.0 - s);
    } else {
        fac = exp((double)theta[j * F + f]);
    }
    dtheta[j * F + f] = (float)(fac * tot);
}

inline int pcen_nchunks(int T) { return (T + PC_CHUNK - 1) / PC_CHUNK; }

inline bool pcen_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + bytes && pb < pa + bytes;
}

}  // namespace

extern "C" int sed_pcen_chunk(void) { return PC_CHUNK; }

extern "C" size_t sed_pcen_ws_bytes(int B, int T, int F) {
    if (B <= 0 || T <= 0 || F <= 0 || F > PC_MAX_F) return 0;
    return (size_t)B * (size_t)pcen_nchunks(T) * (size_t)F * 6 * sizeof(double);      // L, R, part[4]
}

// the checks both directions share; fills A
static int pcen_check(const char* who, const float* x, const float* mean, const float* std, const float* theta, int kind, double eps,
                      double gain, const void* ws, int B, int T, int F, PcenArgs& A) {
#define PC_REQUIRE(cond, msg)                                                    \
    do {                                                                         \
        if (!(cond)) {                                                           \
            sed_set_error(std::string(who) + ": " + (msg) + " [" #cond "]");     \
            return 1;                                                            \
        }                                                                        \
    } while (0)
    PC_REQUIRE(B > 0 && T > 0 && F > 0 && F <= PC_MAX_F, "B > 0, T > 0, F in 1..256");
    PC_REQUIRE(eps > 0.0 && gain > 0.0, "eps and gain must be > 0");          // (a NaN fails both comparisons)
    PC_REQUIRE(kind == 0 || kind == 1, "kind is 0 (dB log-mel) or 1 (linear power)");
    PC_REQUIRE((mean == nullptr) == (std == nullptr), "mean and std come together");
    PC_REQUIRE(kind == 0 || mean == nullptr, "mean / std belong to the dB input (kind 0)");
    PC_REQUIRE(x != nullptr && theta != nullptr && ws != nullptr, "null pointer");
    PC_REQUIRE(((uintptr_t)ws & 7) == 0, "workspace must be 8-byte aligned");
    A.x = x; A.mean = mean; A.std = std; A.theta = theta;
    A.kind = kind; A.eps = eps; A.gain = gain;
    A.B = B; A.T = T; A.F = F; A.nc = pcen_nchunks(T);
    A.n = (size_t)B * (size_t)A.nc * (size_t)F;
    PC_REQUIRE(cdivz(A.n, PC_THREADS) <= 0x7fffffffu, "too many (b, chunk, f) for one grid");
#undef PC_REQUIRE
    return 0;
}

extern "C" int sed_pcen_fwd(const float* x, const float* mean, const float* std, const float* theta, int kind, double eps, double gain,
                            float* y, void* ws, int B, int T, int F, void* stream) {
    PcenArgs A;
    if (int rc = pcen_check(__func__, x, mean, std, theta, kind, eps, gain, ws, B, T, F, A)) return rc;
    SED_REQUIRE(y != nullptr, "null pointer");
    SED_REQUIRE(!pcen_overlap(x, y, (size_t)B * (size_t)T * (size_t)F * sizeof(float)), "y must not overlap x");
    double* Ls = static_cast<double*>(ws);
    const unsigned grid = (unsigned)cdivz(A.n, PC_THREADS);
    hipStream_t st = (hipStream_t)stream;
    pcen_local_kernel<<<grid, PC_THREADS, 0, st>>>(A, Ls);
    SED_LAUNCH_CHECK();
    pcen_fwd_kernel<<<grid, PC_THREADS, 0, st>>>(A, Ls, y);
    SED_LAUNCH_CHECK();
    return 0;
}

extern "C" int sed_pcen_bwd(const float* x, const float* mean, const float* std, const float* theta, int kind, double eps, double gain,
                            const float* gy, float* dx, float* dtheta, void* ws, int B, int T, int F, void* stream) {
    PcenArgs A;
    if (int rc = pcen_check(__func__, x, mean, std, theta, kind, eps, gain, ws, B, T, F, A)) return rc;
    SED_REQUIRE(gy != nullptr, "null pointer");
    SED_REQUIRE(dx != nullptr || dtheta != nullptr, "dx and dtheta are both NULL: nothing to compute");
    const size_t bytes = (size_t)B * (size_t)T * (size_t)F * sizeof(float);
    SED_REQUIRE(dx == nullptr || (!pcen_overlap(x, dx, bytes) && !pcen_overlap(gy, dx, bytes)), "dx must not overlap x or gy");
    double* Ls = static_cast<double*>(ws);
    double* Rs = Ls + A.n;
    double* part = dtheta != nullptr ? Rs + A.n : nullptr;
    const unsigned grid = (unsigned)cdivz(A.n, PC_THREADS);
    hipStream_t st = (hipStream_t)stream;
    pcen_local_kernel<<<grid, PC_THREADS, 0, st>>>(A, Ls);
    SED_LAUNCH_CHECK();
    pcen_bwd_local_kernel<<<grid, PC_THREADS, 0, st>>>(A, gy, Ls, Rs);
    SED_LAUNCH_CHECK();
    pcen_bwd_apply_kernel<<<grid, PC_THREADS, 0, st>>>(A, gy, Ls, Rs, dx, part);
    SED_LAUNCH_CHECK();
    if (dtheta != nullptr) {
        pcen_reduce_kernel<<<dim3((unsigned)cdiv(F, 64), 4), dim3(64, PC_RED_SLICES), 0, st>>>(part, theta, (size_t)B * (size_t)A.nc, F,
                                                                                               dtheta);
        SED_LAUNCH_CHECK();
    }
    return 0;
}
