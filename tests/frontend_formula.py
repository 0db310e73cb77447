"""The log-mel front-end in float64 numpy, its per-element gate and the mutated references of the sensitivity cases: the reference of
tests/test_frontend_formula_host.py and tests/test_gpu_frontend_exact_oracle.py (kernels: csrc/sed_frontend.hip).

Reference (on the fp32 operands the kernel reads, every step in float64): reflect padding by nfft/2 without repeating the edge
(np.pad(mode="reflect")), frame t = padded[t*hop : t*hop + nfft] times the padded window, np.fft.rfft, power |X|^2, mel power
P @ W.T over [mel_lo, mel_hi), 10*log10(max(1e-10, .)), optional (v - mean) / std.

Gate, per element; u = 2^-24 (one fp32 rounding), derived, not fitted:

  STFT.  |X_got - X_ref| <= E_k = u * (C_FFT * log2(nfft) * ||f||_2 + C_LEAK * max_j |X_j| + C_BIN * |X_k|), f = the windowed frame.
    First term: an fp32 FFT's error scales with the frame's norm (sum_k |X_k|^2 = nfft ||f||^2: ||f||_2 is the root-mean-square bin
    magnitude), not with the bin.  Stage count: log2(nfft/2) butterfly stages of the packed complex transform plus the real-FFT split
    (one more twiddle product and two adds: one more stage) = log2(nfft) stages.  Per stage the norm-wise error of a butterfly pass
    with a table rounded once from double is eta = mu + gamma_4 (sqrt(2) + mu), mu = u, gamma_4 = 4u (Higham, Accuracy and Stability
    of Numerical Algorithms, Thm 24.2): 6.66 u.  The window product adds u once.  Sum: (6.66 log2(nfft) + 1) u <= 6.8 u log2(nfft) of
    the rms bin magnitude; C_FFT = 8.  That bounds the root-mean-square error over the bins in the worst case; an ordinary bin's error
    is a sum of nfft independent roundings per stage with a standard deviation of ~2 u ||f||; its magnitude is Rayleigh distributed,
    so the largest of n elements is sqrt(ln n) standard deviations: 3.5 for the 10^5 bins of a case, 8 .. 12 u ||f|| in the plain fp32
    radix-2 FFT of test_frontend_formula_host.py on noise, against 80 .. 96 u ||f||.
    The other two terms are what a tone adds, which the norm-wise count does not see (a bin that holds a tone is up to sqrt(nfft) / 2
    times the rms bin; with the first term alone the radix-2 FFT comes within 1.3 of the bound at nfft 4096).  j stages from the end
    the tonal bin is the sum of 2^j coherent pieces of |X_k| / 2^j, each rounded ~6 times per stage (two products, their difference,
    two table entries, the sum: 0.42 u each; 1.03 u of the piece's magnitude, complex): 1.03 u |X_k| 2^(-j/2) per stage, <= 1.5 u
    |X_k| over the stages.  The butterfly that ADDS two pieces into bin k SUBTRACTS them into its partner bin (k + nfft/4 for the last
    radix-2 stage, k +- nfft/8, .. before; k + j nfft/16 for a radix-8 pass; nfft/2 - k for the real-FFT split, which takes both
    bins out of the pair Z[k], Z[nfft/2 - k]): the pieces cancel, their rounding errors do not.  A tone therefore leaves up to the
    same ~1.5 u |X_k| in a handful of otherwise small bins, wherever the kernel's radix puts them -- hence max_j |X_j| for every bin
    of the frame.  The largest of the ~100 such elements of a case is ~2 standard deviations, 3 u max|X| on paper and 0.8 .. 1.0 u
    max|X| in the radix-2 FFT (whose largest err / ||f|| sits in exactly those bins): C_LEAK = 4.  The tonal bin itself also takes the
    split's ~8 roundings (1.2 u) and the window's (0.42 u) of its own magnitude: 1.3 u |X_k| more, 2.2 .. 3.6 u |X_k| in all in the
    radix-2 FFT; C_BIN = 8 on top of C_LEAK.
  Log-mel, in the power domain.  The kernel's output is taken back to power (undo the z-score in float64, 10^(v/10)), both sides
    are clamped at 1e-10, and |p_got - p_ref| <= S_m + c_acc * u * p_ref with
      S_m   = sum_k W[m,k] * (2 |X_k| E_k + E_k^2)                the STFT bound propagated through the band (||a+e|^2 - |a|^2| <= 2|a||e| + |e|^2)
      c_acc = C_POW + (hi - lo) + C_TREE                         x^2 + y^2 (a product and an fma: 2 u); an fp32 fma chain over the band's
                                                                 non-negative terms in any order (<= one rounding per term); the cross-lane
                                                                 or cross-wave partial sums (2 quad adds, 6 + 2 wave-sum levels, <= 5 tile partials: <= 8)
              + (ln 10 / 10) * (C_LOG * |v| + C_Z * |v - mean|)  log10f within 2 ulp (ulp(y) <= 2 u |y|: 4 u |v|) and the product 10 * y (u |v|): 5 u |v|
                                                                 dB; the subtraction, the reciprocal of std and the product (or the division): 3 u |v - mean|
                                                                 dB; d p / p = (ln 10 / 10) d v.  The test's own 10^x runs in float64 (2^-53: nothing).
    v = the reference dB value.  A band whose reference power is exactly 0 (silence) must give exactly -100 before normalisation.
  sed_complex_to_logmel.  The spectrum is given: no STFT term.  |p_got - p_ref| <= c * u * p_ref, p_ref = sum_k W |X_k|^2,
    c = C_ABS2 + (hi - lo) / 4 + 2 + the same dB terms: sqrt(x^2 + y^2) squared (2 u under the root halves to u, the root u, the square
    doubles: 5 u), four lanes with a quarter of the band each and two adds.
  sed_logmel_crops.  Bit-equal to bank[start + t] without mean / std; with them (v - mean) / std within C_Z * u * |v - mean| / std.
  sed_complex_augment_logmel (complex_augment_logmel_kernel: gather + mean of nmix crops + real noise + complex z-score + |.|^2 + mel
    + log; reference: mix_logmel_reference, gate: mix_ratio).  |p_got - p_ref| <= S_m + c * u * p_ref with sed_complex_to_logmel's c
    (the kernel squares and sums exactly as that one does) and S_m = sum_k W[m,k] * (2 |v_k| E_k + E_k^2), v_k the complex value the
    kernel squares and E_k = hypot(E_re, E_im) the bound on its error.  Per component (x = re or im of the float64 value at each step,
    E the bound carried so far; every new rounding is taken of |x| + E, the largest the computed value can be):
      sum     the nmix - 1 adds of w_1 .. w_nmix: every partial sum is <= A = sum_j |w_j|, one rounding each     E1 = (nmix - 1) u A
      mean    inv = fl(1 / nmix) and the product, applied only for nmix > 1; both are exact for nmix 2 and 4 (a power of two),
              two roundings for nmix 3                                                                            E2 = E1 / nmix + c_inv u (|x| + E1 / nmix), c_inv = 2 (nmix 3), 0 (else)
      noise   re only, only where nstd > 0: fma(nstd, z, x), one rounding; the product nstd * z of the two fp32
              inputs is exact in the reference.  Generator noise: the device's z is within C_GEN u of the float64
              Box-Muller value of the same 24-bit uniforms (below)                                                E3 = E2 [+ nstd C_GEN u] + u (|x| + ..)
      z-score x - mean: one rounding                                                                              E4 = E3 + u (|x| + E3)
              is = fl(1 / std) (correctly rounded division: u) and the product (u)                                E5 = (E4 + 2 u (|x| + E4)) / std
    C_GEN (absolute: |z| < R = sqrt(-2 ln 2^-24) = sqrt(48 ln 2) = 5.77): u1, u2 are exact in fp32 (24-bit integers times 2^-24).
      The argument fl(fl(2 pi) u2) carries the rounded constant and the product: 2 u * 2 pi = 4 pi u, and |d cos| <= |d arg|.
      cosf: <= 4 ulp, logf: <= 3 ulp (the limits of OpenCL's full profile, which the device library is written to);
      ulp(y) <= 2 u |y|: 8 u on the cosine; 6 u relative under the root, which halves it, plus the root's own u: 4 u on the radius;
      the final product: u.  |dz| <= R (4 pi + 8 + 4 + 1) u = 147.5 u.
    A band whose reference power is exactly 0 (an empty band, an all-zero bank without noise and z-score) must give exactly -100.

Measured on the MI355X (tests/test_gpu_frontend_exact_oracle.py holds the table): the largest err / bound is 0.23 for the STFT
(margin 4.4), 0.26 for the log-mel routes (3.9, through the single-bin bands of a Slaney bank, i.e. the STFT bound again), 0.60 and 0.62
for sed_complex_to_logmel on bands of 1 .. 5 bins and for the crops' z-score, whose bounds are worst-case counts of a few roundings;
0.58 for sed_complex_augment_logmel (margin 1.7, on the same short bands; tests/test_gpu_complex_augment_exact_oracle.py holds its table)
and 0.18 for the generator's draws read out one by one.
"""
import numpy as np

from oracle import dataset_oracle as DO
from oracle import frontend_oracle as FO

U = 2.0 ** -24
C_FFT = 8.0
C_BIN = 8.0
C_LEAK = 4.0
C_POW = 2.0
C_TREE = 8.0
C_LOG = 5.0
C_Z = 3.0
C_ABS2 = 5.0
LN10_10 = np.log(10.0) / 10.0
AMIN = 1e-10

MUTATIONS = ("symmetric_pad", "window_roll", "drop_last_bin", "drop_first_bin", "clip_shift", "meanstd_roll", "edge_half")


# ---- inputs shared by the host and the GPU file -------------------------------------------------------------------------------------
def make_waves(B, samples, seed, amps=None, sr=32000):
    """(B, samples) float32: broadband noise plus a tone and a burst per clip (every bin well above the FFT bound), clip b scaled
    by amps[b] (0: a silent clip)"""
    out = np.empty((B, samples), np.float32)
    t = np.arange(samples) / sr
    for b in range(B):
        rng = np.random.default_rng(1000 * seed + b)
        y = 0.1 * rng.standard_normal(samples)
        y += 0.4 * np.sin(2 * np.pi * (1234.5 + 517.0 * b) * t + b)
        k = samples // 3
        y[k:k + 50] += 0.3 * rng.standard_normal(min(50, samples - k))
        out[b] = (np.clip(y, -1, 1) * (1.0 if amps is None else amps[b])).astype(np.float32)
    return out


def make_window(nfft, win_len=None):
    """np.hanning(win_len) centred in nfft zeros, float32 (the layout sed_logmel_fwd takes)"""
    win_len = nfft if win_len is None else win_len
    w = np.zeros(nfft, np.float64)
    left = (nfft - win_len) // 2
    w[left:left + win_len] = np.hanning(win_len)
    return w.astype(np.float32)


def make_meanstd(n_mels):
    return np.linspace(-40.0, -20.0, n_mels).astype(np.float32) + np.float32(0.37), np.linspace(5.0, 9.0, n_mels).astype(np.float32)


def _fill(W, lo, hi, m, a, b, rng):
    W[m, a:b] = rng.random(b - a).astype(np.float32) + np.float32(0.05)       # edge weights are not near zero
    lo[m], hi[m] = a, b


def make_bank(kind, n_mels, bins, seed=0, width=None, sr=32000):
    """(W (n_mels, bins) float32, lo, hi int32); W is zero outside [lo, hi) for every kind.
      slaney        the oracle's Slaney bank for (sr, nfft = 2 (bins - 1), n_mels)
      random        bands of width/2 .. width bins anywhere; filter 0 starts at bin 0, the last filter ends at bin `bins`
      empty         random, with every filter of the second 16-filter tile (and filters 3 and n_mels - 2) empty (hi == lo)
      dense         every filter spans all bins
      sum:<n>       64-ish filters whose lengths add up to exactly n (the compact weight list of frontend1024_kernel holds 1152)
      lengths       filter i has length i % 6 and lo % 4 == (i // 6) % 4"""
    rng = np.random.default_rng(7919 * seed + n_mels)
    W = np.zeros((n_mels, bins), np.float32)
    lo = np.zeros(n_mels, np.int32)
    hi = np.zeros(n_mels, np.int32)
    if kind == "slaney":
        W[:] = FO.mel_filter_bank_matrix(FO.FrontEndConfig(sr, 2 * (bins - 1), 1, 2 * (bins - 1), mel_bins=n_mels)).T
        nz = W > 0
        lo[:] = np.where(nz.any(1), nz.argmax(1), 0)
        hi[:] = np.where(nz.any(1), bins - nz[:, ::-1].argmax(1), 0)
        return W, lo, hi
    if kind == "dense":
        for m in range(n_mels):
            _fill(W, lo, hi, m, 0, bins, rng)
        return W, lo, hi
    if kind.startswith("sum:"):
        total = int(kind[4:])
        base, extra = divmod(total, n_mels)
        for m in range(n_mels):
            n = base + (1 if m < extra else 0)
            a = int(rng.integers(0, bins - n + 1))
            _fill(W, lo, hi, m, a, a + n, rng)
        assert int((hi - lo).sum()) == total
        return W, lo, hi
    if kind == "lengths":
        for m in range(n_mels):
            n = m % 6
            a = 4 * int(rng.integers(0, (bins - 8) // 4)) + (m // 6) % 4
            _fill(W, lo, hi, m, a, a + n, rng)
        return W, lo, hi
    assert kind in ("random", "empty"), kind
    width = max(2, min(bins - 1, bins // 4 if width is None else width))
    for m in range(n_mels):
        n = int(rng.integers(max(1, width // 2), width + 1))
        a = int(rng.integers(0, bins - n + 1))
        if m == 0:
            a = 0
        if m == n_mels - 1:
            a = bins - n
        if kind == "empty" and (16 <= m < 32 or m in (3, n_mels - 2)):
            lo[m] = hi[m] = a
            continue
        _fill(W, lo, hi, m, a, a + n, rng)
    return W, lo, hi


# ---- reference ----------------------------------------------------------------------------------------------------------------------
def windowed_frames(waves, window, nfft, hop, pad_mode="reflect"):
    """(B, T, nfft) float64: padded[t*hop : t*hop + nfft] * window, T = 1 + samples // hop"""
    waves, window = np.asarray(waves, np.float64), np.asarray(window, np.float64)      # (callers hand in the kernel's fp32 arrays)
    B, n = waves.shape
    T = 1 + n // hop
    idx = (np.arange(T) * hop)[:, None] + np.arange(nfft)[None, :]
    return np.stack([np.pad(w, nfft // 2, mode=pad_mode)[idx] for w in waves]) * window


class Reference:
    """Everything a check needs for one (waves, window, nfft, hop): X (B, T, bins) complex128, E (B, T, bins) the STFT bound."""

    def __init__(self, waves, window, nfft, hop, mutation=None):
        assert mutation in (None,) + MUTATIONS
        self.nfft, self.hop = nfft, hop
        win = np.roll(np.asarray(window), 1) if mutation == "window_roll" else window
        f = windowed_frames(waves, win, nfft, hop, "symmetric" if mutation == "symmetric_pad" else "reflect")
        if mutation == "clip_shift":
            f = np.concatenate([f[:1], f[:-1]])
        self.fnorm = np.sqrt((f * f).sum(-1))
        self.X = np.fft.rfft(f, axis=-1)
        A = np.abs(self.X)
        self.E = U * (C_FFT * np.log2(nfft) * self.fnorm[..., None] + C_LEAK * A.max(-1, keepdims=True) + C_BIN * A)
        self.mutation = mutation

    def mel(self, W, lo, hi, mean=None, std=None):
        return MelReference(self.X, self.E, W, lo, hi, mean, std, self.mutation)


class MelReference:
    """p (.., n_mels) mel power, S its STFT-bound term, v the dB value, z the (optionally z-scored) output -- all float64."""

    def __init__(self, X, E, W, lo, hi, mean=None, std=None, mutation=None):
        W = np.asarray(W, np.float32).astype(np.float64).copy()
        lo, hi = np.asarray(lo).astype(np.int64), np.asarray(hi).astype(np.int64)
        k = np.arange(W.shape[1])[None, :]
        if mutation == "drop_last_bin":
            hi = np.maximum(lo, hi - 1)
        if mutation == "drop_first_bin":
            lo = np.minimum(hi, lo + 1)
        W *= (k >= lo[:, None]) & (k < hi[:, None])                    # the band is [mel_lo, mel_hi)
        A = np.abs(X)
        if mutation == "edge_half":                                    # the old tolerance's worth: ONE band-edge weight halved -- of the
            ok = hi - lo > 1                                           # band whose last bin holds the largest share of its power somewhere
            e = np.maximum(hi - 1, 0)
            share = W[np.arange(len(e)), e] * (A * A)[..., e] / np.maximum((A * A) @ W.T, 1e-300)
            m = int(np.argmax(np.where(ok, share.reshape(-1, len(e)).max(0), -1.0)))
            W[m, e[m]] *= 0.5
        self.n = (hi - lo).astype(np.float64)
        self.p = (A * A) @ W.T
        self.S = None if E is None else (2.0 * A * E + E * E) @ W.T
        self.v = 10.0 * np.log10(np.maximum(AMIN, self.p))
        self.mean = None if mean is None else np.asarray(mean, np.float32).astype(np.float64)
        self.std = None if std is None else np.asarray(std, np.float32).astype(np.float64)
        if mutation == "meanstd_roll" and mean is not None:
            self.mean, self.std = np.roll(self.mean, 1), np.roll(self.std, 1)
        self.z = self.v if mean is None else (self.v - self.mean) / self.std


def logmel_reference(waves, window, nfft, hop, W, lo, hi, mean=None, std=None, mutation=None):
    return Reference(waves, window, nfft, hop, mutation).mel(W, lo, hi, mean, std)


def make_inputs(nfft, hop, samples, B, n_mels=0, bank="random", seed=0, amps=None, win_len=None, meanstd=False, width=None):
    """one case's host arrays: waves, window and (n_mels > 0) W, lo, hi, mean, std (None without meanstd)"""
    d = dict(nfft=nfft, hop=hop, samples=samples, B=B, n_mels=n_mels, waves=make_waves(B, samples, seed + nfft + hop, amps),
             window=make_window(nfft, win_len), W=None, lo=None, hi=None, mean=None, std=None)
    if n_mels:
        d["W"], d["lo"], d["hi"] = make_bank(bank, n_mels, nfft // 2 + 1, seed, width)
        if meanstd:
            d["mean"], d["std"] = make_meanstd(n_mels)
    return d


# one shape per route for the sensitivity cases (random banks: edge weights >= 0.05; B >= 2; first and last frames reflect)
SENSITIVITY = {
    "batched": dict(nfft=1024, hop=128, samples=2432, B=2, n_mels=40, bank="random", width=60, meanstd=True),
    "fallback": dict(nfft=1024, hop=250, samples=2250, B=2, n_mels=40, bank="random", width=60, meanstd=True),
    "generic": dict(nfft=256, hop=100, samples=1000, B=2, n_mels=20, bank="random", width=30, meanstd=True),
    "big": dict(nfft=4096, hop=1500, samples=9001, B=2, n_mels=17, bank="random", width=100, meanstd=True),
}
STFT_MUTATIONS = ("symmetric_pad", "window_roll", "clip_shift")


# ---- gates: every function returns err / bound per element (<= 1 passes; inf: an element that had to be exact and is not) -----------
def _ratio(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = err / bound
    return np.where(err == 0, 0.0, np.where(bound > 0, r, np.inf))


def stft_ratio(got, ref):
    """got (B, T, bins) complex; a silent frame (E = 0) must be exactly 0"""
    got = np.asarray(got).astype(np.complex128)
    assert got.shape == ref.X.shape, (got.shape, ref.X.shape)
    return _ratio(np.abs(got - ref.X), ref.E)


def _db_terms(mr):
    t = C_LOG * np.abs(mr.v)
    if mr.mean is not None:
        t = t + C_Z * np.abs(mr.v - mr.mean)
    return LN10_10 * t


def _power_ratio(got, mr, bound):
    got = np.asarray(got).astype(np.float64)
    assert got.shape == mr.p.shape, (got.shape, mr.p.shape)
    assert np.isfinite(got).all()
    v_got = got if mr.mean is None else got * mr.std + mr.mean
    p_got = np.maximum(AMIN, 10.0 ** (v_got / 10.0))
    r = _ratio(np.abs(p_got - np.maximum(AMIN, mr.p)), bound)
    silent = mr.p == 0
    if silent.any():                      # exactly -100 before normalisation
        if mr.mean is None:
            ok = got == -100.0
        else:
            zr = (np.float64(np.float32(-100.0)) - mr.mean) / mr.std
            ok = np.abs(got - zr) <= C_Z * U * np.abs(zr)
        r = np.where(silent, np.where(ok, 0.0, np.inf), r)
    return r


def logmel_ratio(got, mr):
    """got: the kernel's output (.., n_mels) float32 of a waveform route"""
    return _power_ratio(got, mr, mr.S + (C_POW + mr.n + C_TREE + _db_terms(mr)) * U * mr.p)


def complex_logmel_ratio(got, mr):
    """got: sed_complex_to_logmel's output; mr = MelReference(X, None, ...) on the spectrum the kernel was given"""
    return _power_ratio(got, mr, (C_ABS2 + mr.n / 4.0 + 2.0 + _db_terms(mr)) * U * mr.p)


def crops_ratio(got, bank, starts, crop, mean=None, std=None):
    """sed_logmel_crops against plain indexing: bit-equal without mean / std, else within C_Z u |v - mean| / std"""
    bank = np.asarray(bank, np.float32)
    ref = np.stack([bank[s:s + crop] for s in starts]).astype(np.float64)
    got = np.asarray(got).astype(np.float64)
    assert got.shape == ref.shape
    if mean is None:
        return _ratio(np.abs(got - ref), np.zeros_like(ref))
    mean, std = np.asarray(mean, np.float32).astype(np.float64), np.asarray(std, np.float32).astype(np.float64)
    z = (ref - mean) / std
    return _ratio(np.abs(got - z), C_Z * U * np.abs(z))


# ---- an independent fp32 emulation (what a correct fp32 implementation gives: the gate must accept it) --------------------------------
def log10_f32(x):
    """a correctly rounded fp32 log10 (numpy's own float32 log10 is an ulp off at 1e-10f: -10.000001)"""
    return np.log10(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def emulate_f32(waves, window, nfft, hop, W=None, lo=None, hi=None, mean=None, std=None):
    """Plain float32 numpy: radix-2 DIT FFT of the packed frame with a float32 twiddle table, the real-FFT split, fp32 power and fp32
    band sums, fp32 log and z-score.  Returns the spectrum (complex64) without a bank, else the log-mel output (float32)."""
    f32 = np.float32
    waves, window = np.asarray(waves, f32), np.asarray(window, f32)
    B, n = waves.shape
    T, M = 1 + n // hop, nfft // 2
    idx = (np.arange(T) * hop)[:, None] + np.arange(nfft)[None, :]
    fr = np.stack([np.pad(w, M, mode="reflect")[idx] for w in waves]) * window          # fp32 products
    assert fr.dtype == f32
    logM = M.bit_length() - 1
    rev = np.array([int(format(i, f"0{logM}b")[::-1], 2) for i in range(M)])
    k = np.arange(M, dtype=np.float64)
    twr, twi = np.cos(-2 * np.pi * k / nfft).astype(f32), np.sin(-2 * np.pi * k / nfft).astype(f32)
    zr, zi = fr[..., 0::2][..., rev].copy(), fr[..., 1::2][..., rev].copy()
    for s in range(logM):
        half = 1 << s
        zr = zr.reshape(B, T, -1, 2, half)
        zi = zi.reshape(B, T, -1, 2, half)
        t = 2 * np.arange(half) * (M >> (s + 1))
        wr, wi = twr[t], twi[t]
        br = zr[..., 1, :] * wr - zi[..., 1, :] * wi
        bi = zr[..., 1, :] * wi + zi[..., 1, :] * wr
        ar, ai = zr[..., 0, :], zi[..., 0, :]
        zr = np.stack([ar + br, ar - br], axis=-2).reshape(B, T, M)
        zi = np.stack([ai + bi, ai - bi], axis=-2).reshape(B, T, M)
    kk = np.arange(1, M)
    h = f32(0.5)
    a_r, a_i, c_r, c_i = zr[..., kk], zi[..., kk], zr[..., M - kk], zi[..., M - kk]
    er, ei = h * (a_r + c_r), h * (a_i - c_i)
    orr, oi = h * (a_i + c_i), -h * (a_r - c_r)
    wor, woi = twr[kk] * orr - twi[kk] * oi, twr[kk] * oi + twi[kk] * orr
    Xr = np.concatenate([zr[..., :1] + zi[..., :1], er + wor, zr[..., :1] - zi[..., :1]], axis=-1)
    Xi = np.concatenate([np.zeros_like(zr[..., :1]), ei + woi, np.zeros_like(zr[..., :1])], axis=-1)
    assert Xr.dtype == f32 and Xi.dtype == f32
    if W is None:
        return (Xr + 1j * Xi).astype(np.complex64)
    P = Xr * Xr + Xi * Xi
    W = np.asarray(W, f32)
    out = np.empty((B, T, W.shape[0]), f32)
    for m in range(W.shape[0]):
        acc = np.zeros((B, T), f32)
        for j in range(int(lo[m]), int(hi[m])):
            acc = acc + W[m, j] * P[..., j]
        out[..., m] = f32(10.0) * log10_f32(np.maximum(f32(AMIN), acc))
    if mean is not None:
        out = (out - np.asarray(mean, f32)) / np.asarray(std, f32)
    assert out.dtype == f32
    return out


# ---- sed_complex_augment_logmel: reference, gate, mutated references, inputs, fp32 emulation ------------------------------------------
R_GEN = float(np.sqrt(48.0 * np.log(2.0)))                        # the largest Box-Muller radius of a 24-bit uniform
C_GEN = R_GEN * (4.0 * np.pi + 8.0 + 4.0 + 1.0)                   # |z_device - z_float64| <= C_GEN * u (derivation: the docstring)
INT_MAX = 2 ** 31 - 1

# name -> what a case must have for the mutation to change the result (mix_mutations_for)
MIX_MUTATIONS = {
    "div_nmix_plus_1": "any",            # divide by nmix + 1
    "no_division": "mix",                # the sum, not the mean
    "max_not_mean": "mix",               # component-wise maximum in place of the mean
    "noise_on_imag": "noise",            # the noise also on the imaginary part
    "noise_after_zscore": "noise+z",     # z-score first, then the noise
    "counter_no_frame": "gen",           # generator counter k in place of frame * bins + k
    "counter_n_mels": "gen",             # generator counter frame * n_mels + k
    "conj_mean": "z",                    # the conjugated mean
    "mul_cstd": "z",                     # times std in place of divided by it
    "row_plus_1": "any",                 # bank row start + 1 + t
    "slot0_for_all": "mix",              # every mixed crop read from slot 0
}


def counter_normal64(seed, counters):
    """the generator's draw in float64 from the same two 24-bit uniforms (oracle.dataset_oracle.counter_normal rounds this to fp32)"""
    h = DO.counter_bits(seed, counters)
    u1 = (((h >> np.uint64(40)) & np.uint64(0xFFFFFF)).astype(np.float64) + 1.0) / 16777216.0
    u2 = ((h >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def _counters(B, crop, bins, stride=None, frame_term=True):
    frame = np.arange(B * crop, dtype=np.uint64).reshape(B, crop, 1) * np.uint64(bins if stride is None else stride)
    k = np.arange(bins, dtype=np.uint64)[None, None, :]
    return frame + k if frame_term else np.broadcast_to(k, (B, crop, bins)).copy()


class MixReference:
    """V (B, crop, bins) complex128: the value the kernel squares; E its error bound; p, S, v (B, crop, n_mels) as in MelReference."""

    def __init__(self, bank, starts, nmix, nstd, z, cmean, cstd, W, lo, hi, mutation=None, crop=None, seed=None):
        assert mutation is None or mutation in MIX_MUTATIONS, mutation
        bank = np.asarray(bank, np.complex64).astype(np.complex128)
        frames, bins = bank.shape
        starts, nmix = np.asarray(starts).reshape(-1, 4).astype(np.int64), np.asarray(nmix).astype(np.int64)
        B = len(nmix)
        if z is not None:
            z = np.asarray(z, np.float32).astype(np.float64)
            crop = z.shape[1] if crop is None else crop
            assert z.shape == (B, crop, bins)
        assert crop is not None
        generator = z is None and nstd is not None and seed is not None
        if generator:
            z = counter_normal64(seed, _counters(B, crop, bins, W.shape[0] if mutation == "counter_n_mels" else None,
                                                 mutation != "counter_no_frame"))
        nstd = np.zeros(B) if nstd is None else np.asarray(nstd, np.float32).astype(np.float64)
        assert z is not None or not (nstd > 0).any(), "noise asked for without draws or a seed"
        zscore = cmean is not None
        if zscore:
            mu = np.asarray(cmean, np.complex64).astype(np.complex128)
            sd = np.asarray(cstd, np.float32).astype(np.float64)
            if mutation == "conj_mean":
                mu = mu.conj()
        t = np.arange(crop)
        self.V = np.empty((B, crop, bins), np.complex128)
        self.E = np.empty((B, crop, bins), np.float64)
        for b in range(B):
            nm = int(nmix[b])
            assert 1 <= nm <= 4
            rows = [starts[b, 0 if mutation == "slot0_for_all" else j] + t + (1 if mutation == "row_plus_1" else 0) for j in range(nm)]
            w = np.stack([bank[r % frames] for r in rows])                       # (nm, crop, bins); unused slots are never read
            if mutation == "max_not_mean":
                v = w.real.max(0) + 1j * w.imag.max(0)
            else:
                v = w.sum(0) / {"div_nmix_plus_1": nm + 1.0, "no_division": 1.0}.get(mutation, float(nm))
            c_inv = 2.0 if nm == 3 else 0.0
            ns = nstd[b]
            noise = ns * z[b] if ns > 0 else None
            comp = []
            for part, x in (("re", v.real.copy()), ("im", v.imag.copy())):
                A = np.abs(w.real if part == "re" else w.imag).sum(0)
                e = (nm - 1) * U * A / nm
                e = e + c_inv * U * (np.abs(x) + e)
                if noise is not None and mutation != "noise_after_zscore" and (part == "re" or mutation == "noise_on_imag"):
                    x = x + noise
                    e = e + (ns * C_GEN * U if generator else 0.0)
                    e = e + U * (np.abs(x) + e)
                if zscore:
                    x = x - (mu.real if part == "re" else mu.imag)
                    e = e + U * (np.abs(x) + e)
                    if mutation == "mul_cstd":
                        x, e = x * sd, (e + 2.0 * U * (np.abs(x) + e)) * sd
                    else:
                        x, e = x / sd, (e + 2.0 * U * (np.abs(x) + e)) / sd
                if noise is not None and mutation == "noise_after_zscore" and part == "re":
                    x = x + noise
                comp.append((x, e))
            self.V[b] = comp[0][0] + 1j * comp[1][0]
            self.E[b] = np.hypot(comp[0][1], comp[1][1])
        W = np.asarray(W, np.float32).astype(np.float64).copy()
        lo, hi = np.asarray(lo).astype(np.int64), np.asarray(hi).astype(np.int64)
        k = np.arange(bins)[None, :]
        W *= (k >= lo[:, None]) & (k < hi[:, None])
        A = np.abs(self.V)
        self.n = (hi - lo).astype(np.float64)
        self.p = (A * A) @ W.T
        self.S = (2.0 * A * self.E + self.E * self.E) @ W.T
        self.v = 10.0 * np.log10(np.maximum(AMIN, self.p))
        self.mean = self.std = None
        self.z = self.v


def mix_logmel_reference(bank, starts, nmix, nstd, z, cmean, cstd, W, lo, hi, mutation=None, crop=None, seed=None):
    """float64 reference of sed_complex_augment_logmel on its fp32 inputs.  bank (frames, bins) complex64; starts (B, 4), only the
    first nmix[b] slots of a row are read; nstd (B,) or None (no noise); z (B, crop, bins) explicit draws, or None with `seed` for the
    in-kernel generator (then `crop` is needed too); cmean / cstd (bins,) or None."""
    return MixReference(bank, starts, nmix, nstd, z, cmean, cstd, W, lo, hi, mutation, crop, seed)


def mix_ratio(got, ref):
    """got: the kernel's output (B, crop, n_mels); err / bound per element"""
    return _power_ratio(got, ref, ref.S + (C_ABS2 + ref.n / 4.0 + 2.0 + _db_terms(ref)) * U * ref.p)


def _mc(bins, n_mels, crop, bank, nmix, noise=None, nstd=None, zscore=False, kind="noise", frames=40, width=None):
    return dict(bins=bins, n_mels=n_mels, crop=crop, bank=bank, nmix=tuple(nmix), noise=noise, nstd=nstd, zscore=zscore, kind=kind,
                frames=frames, width=width)


# the cases of tests/test_gpu_complex_augment_exact_oracle.py (the host file runs the fp32 emulation through the same list).
# noise: None (noise_std NULL), "off" (a table of zeros), "explicit", "gen"; kind: "noise" (amplitude 5), "amps" (rows of amplitude 30,
# then rows of 1e-3; the last clip lies in the quiet rows), "zero" (an all-zero bank).  The n_mels loop wraps above 64 (65, 130);
# bins 16385 is four bytes over the 64 KB of LDS a launch gets without asking, 32769 the largest the launch accepts.  Noise of 0.004
# on a band of a hundred bins of amplitude 30 moves its power by less than the band's own rounding bound: the cases whose bands are all
# that wide carry louder noise, so that every noise mutation shows in every case it is listed for.
MIX_CASES = [
    _mc(33, 1, 1, "random", [1]),
    _mc(257, 17, 9, "lengths", [1, 1]),
    _mc(513, 64, 9, "empty", [1, 2], kind="zero"),
    _mc(513, 64, 9, "slaney", [1, 2, 3, 4, 1]),
    _mc(257, 65, 9, "lengths", [4, 3, 2, 1], kind="amps"),
    _mc(513, 130, 1, "lengths", [3, 2], noise="off"),
    _mc(513, 64, 9, "slaney", [1, 2, 3, 4, 1], "explicit", (0.0, 0.004, 0.0, 0.0065, 0.006), zscore=True),
    _mc(257, 130, 9, "lengths", [1, 2, 3, 4], "explicit", (0.7, 0.0, 0.004, 0.05), kind="amps"),
    _mc(33, 17, 1, "dense", [2, 1, 3], "explicit", (0.5, 0.004, 0.0), zscore=True),
    _mc(513, 64, 9, "slaney", [1, 2, 3, 4, 1], "gen", (0.0, 0.004, 0.0, 0.0065, 0.006), zscore=True),
    _mc(257, 65, 9, "lengths", [1, 3], "gen", (0.3, 0.004)),
    _mc(513, 17, 1, "empty", [2, 4, 1], "gen", (0.004, 0.3, 0.0), zscore=True, kind="amps"),
    _mc(257, 64, 9, "dense", [1, 1, 2], zscore=True),
    _mc(513, 130, 9, "lengths", [1, 3], zscore=True, kind="amps"),
    _mc(33, 17, 1, "random", [1], zscore=True, kind="zero"),
    _mc(16385, 17, 1, "lengths", [3, 1], "explicit", (0.004, 0.0), zscore=True, frames=6),
    _mc(16385, 5, 2, "random", [2], "gen", (0.3,), frames=6, width=48),
    _mc(32769, 5, 2, "random", [4], "gen", (0.05,), zscore=True, frames=6, width=48),
    _mc(32769, 1, 1, "random", [1], frames=4),
]


def mix_id(c):
    s = f"b{c['bins']}-m{c['n_mels']}-c{c['crop']}-{c['bank']}-mix{''.join(map(str, c['nmix']))}"
    s += f"-{c['noise']}" if c["noise"] else ""
    s += "-z" if c["zscore"] else ""
    return s + (f"-{c['kind']}" if c["kind"] != "noise" else "")


def mix_group(c):
    """the row of the measured table a case is recorded under"""
    if c["bins"] > 16384:
        return "wide bins"
    if c["noise"] in ("gen", "explicit"):
        return "generator" if c["noise"] == "gen" else "explicit noise"
    return "z-score" if c["zscore"] else "mixed" if max(c["nmix"]) > 1 else "plain"


def mix_mutations_for(c):
    """the mutations that change this case's result (the cases each mutation is listed for)"""
    if c["kind"] == "zero":              # (nothing to mix or shift, and |-mean / std|^2 does not see the conjugate)
        return []
    B, has = len(c["nmix"]), {"any"}
    if max(c["nmix"]) > 1:
        has.add("mix")
    if c["noise"] in ("explicit", "gen"):
        has.add("noise")
        if c["zscore"]:
            has.add("noise+z")
    if c["noise"] == "gen" and B * c["crop"] > 1:
        has.add("gen")
    if c["zscore"]:
        has.add("z")
    return [m for m, need in MIX_MUTATIONS.items() if need in has]


def make_mix_inputs(c, seed=0):
    """one case's host arrays: bank (frames, bins) complex64, starts (B, 4) int32 with -1 / INT_MAX in the unused slots, nmix, nstd and
    z (or None), seed, cmean / cstd (or None), W, lo, hi.  Clip 0 starts at row 0, the last clip's last crop at frames - crop (the last
    legal start); a clip of three or four crops holds one start twice."""
    bins, n_mels, crop, frames = c["bins"], c["n_mels"], c["crop"], c["frames"]
    B = len(c["nmix"])
    rng = np.random.default_rng(1000 * seed + bins + 7 * n_mels + crop)
    amp = np.full(frames, 5.0)
    if c["kind"] == "amps":
        amp[:frames // 2], amp[frames // 2:] = 30.0, 1e-3
    bank = ((rng.standard_normal((frames, bins)) + 1j * rng.standard_normal((frames, bins))) * 10.0 ** rng.uniform(-1.5, 1.5, (frames, bins))
            * amp[:, None]).astype(np.complex64)
    if c["kind"] == "zero":
        bank[:] = 0
    last = frames - crop
    assert last >= 1 and (c["kind"] != "amps" or crop <= frames // 2)
    nmix = np.array(c["nmix"], np.int32)
    starts = rng.integers(0, last + 1, (B, 4)).astype(np.int32)
    if c["kind"] == "amps":
        starts[:-1] = rng.integers(0, frames // 2 - crop + 1, (B - 1, 4))         # loud clips from the loud rows,
        starts[-1] = rng.integers(frames // 2, last + 1, 4)                       # the last clip from the quiet ones
    starts[0, 0] = 0
    for b in range(B):
        if nmix[b] >= 3:
            starts[b, 1] = starts[b, 0]
        if b == B - 1:
            starts[b, nmix[b] - 1] = last
        starts[b, nmix[b]:] = [-1, INT_MAX, -1][:4 - nmix[b]]
    d = dict(c, B=B, bank=bank, starts=starts, nmix=nmix, nstd=None, z=None, seed=0, cmean=None, cstd=None)
    if c["noise"] == "off":
        d["nstd"] = np.zeros(B, np.float32)
    elif c["noise"]:
        d["nstd"] = np.array(c["nstd"], np.float32)
        assert len(d["nstd"]) == B
        if c["noise"] == "explicit":
            d["z"] = rng.standard_normal((B, crop, bins)).astype(np.float32)
        else:
            d["seed"] = 0x9E3779B97F4A7C15 ^ (bins * 1000003 + n_mels)            # all 64 bits in use
    if c["zscore"]:
        d["cmean"] = (0.3 * (rng.standard_normal(bins) + 1j * rng.standard_normal(bins))).astype(np.complex64)
        d["cstd"] = (1.0 + rng.random(bins)).astype(np.float32)
    d["W"], d["lo"], d["hi"] = make_bank(c["bank"], n_mels, bins, seed, c["width"])
    return d


def mix_reference_of(d, mutation=None):
    return mix_logmel_reference(d["bank"], d["starts"], d["nmix"], d["nstd"], d["z"], d["cmean"], d["cstd"], d["W"], d["lo"], d["hi"],
                                mutation, d["crop"], d["seed"] if d["noise"] == "gen" else None)


def emulate_mix_f32(bank, starts, nmix, nstd, z, cmean, cstd, W, lo, hi, crop, seed=None, order="lanes"):
    """Plain float32 numpy of the same operation (no fma: every product and every add rounds).  order "lanes": the band sum as four
    interleaved chains k = lo + q, lo + q + 4, .. added as (0 + 1) + (2 + 3), the kernel's order; "plain": one chain over the band."""
    f32 = np.float32
    bank = np.asarray(bank, np.complex64)
    re, im = np.ascontiguousarray(bank.real), np.ascontiguousarray(bank.imag)
    bins, B = bank.shape[1], len(nmix)
    t = np.arange(crop)
    P = np.empty((B, crop, bins), f32)
    if z is None and nstd is not None and seed is not None:
        h = DO.counter_bits(seed, _counters(B, crop, bins))
        u1 = (((h >> np.uint64(40)) & np.uint64(0xFFFFFF)).astype(f32) + f32(1)) * f32(1 / 16777216)
        u2 = ((h >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(f32) * f32(1 / 16777216)
        z = np.sqrt(f32(-2) * np.log(u1)) * np.cos(f32(2 * np.pi) * u2)
        assert z.dtype == f32
    for b in range(B):
        nm = int(nmix[b])
        x, y = re[starts[b, 0] + t], im[starts[b, 0] + t]
        for j in range(1, nm):
            x, y = x + re[starts[b, j] + t], y + im[starts[b, j] + t]
        if nm > 1:
            inv = f32(1) / f32(nm)
            x, y = x * inv, y * inv
        if nstd is not None and nstd[b] > 0:
            x = x + f32(nstd[b]) * np.asarray(z[b], f32)
        if cmean is not None:
            mu = np.asarray(cmean, np.complex64)
            inv = f32(1) / np.asarray(cstd, f32)
            x, y = (x - mu.real) * inv, (y - mu.imag) * inv
        a = np.sqrt(x * x + y * y)
        P[b] = a * a
        assert P.dtype == f32 and a.dtype == f32
    W = np.asarray(W, f32)
    out = np.empty((B, crop, W.shape[0]), f32)
    for m in range(W.shape[0]):
        chains = [range(int(lo[m]) + q, int(hi[m]), 4) for q in range(4)] if order == "lanes" else [range(int(lo[m]), int(hi[m]))]
        acc = []
        for ch in chains:
            a = np.zeros((B, crop), f32)
            for j in ch:
                a = a + W[m, j] * P[..., j]
            acc.append(a)
        s = (acc[0] + acc[1]) + (acc[2] + acc[3]) if order == "lanes" else acc[0]
        out[..., m] = np.maximum(f32(-100.0), f32(10.0) * log10_f32(np.maximum(f32(AMIN), s)))
    assert out.dtype == f32
    return out
