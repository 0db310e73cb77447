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

Measured on the MI355X (tests/test_gpu_frontend_exact_oracle.py holds the table): the largest err / bound is 0.23 for the STFT
(margin 4.4), 0.26 for the log-mel routes (3.9, through the single-bin bands of a Slaney bank, i.e. the STFT bound again), 0.60 and 0.62
for sed_complex_to_logmel on bands of 1 .. 5 bins and for the crops' z-score, whose bounds are worst-case counts of a few roundings.
"""
import numpy as np

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
