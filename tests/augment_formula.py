"""The definition of sed_logmel_augment (include/sed_hip.h) restated for the tests: plain loops in float64 over the fp32 inputs
(augment_formula) and a vectorised numpy version of the same definition (augment_vectorised) that also returns the fp32 stage
values the exactness rules of tests/test_gpu_augment.py need.  tests/test_augment_host.py checks one against the other.

Row b of the int32 table: start, shift, partner, lam (float bits), n_tmask x (t0, w), n_fmask x (f0, w).  With T = crop:
    z_b[t, f]   = bank[start_b + t, f]                     ((bank - mean[f]) / std[f] when mean / std are given)
    u_b[t, f]   = z_b[(t - shift_b) mod T, f] + gain[b, f]
    v_b         = u_b if partner_b == b else lam_b * u_b + (1 - lam_b) * u_partner_b
    out_b[t, f] = mask_value if t is in a time interval [t0, t0 + w) or f in a frequency interval of row b, else v_b[t, f]
    r_b[t, k]   = events[start_b + (t - shift_b) mod T, k]
    ev_b        = r_b if partner_b == b else max(r_b, r_p) (label_mix 0) or lam * r_b + (1 - lam) * r_p (label_mix 1)"""
from types import SimpleNamespace

import numpy as np


def table_lam(tab):
    """the lam column of a table as float32"""
    return np.ascontiguousarray(np.asarray(tab, dtype=np.int32)[:, 3]).view(np.float32)


def make_row(start, shift=0, partner=0, lam=1.0, tmasks=(), fmasks=()):
    row = [int(start), int(shift), int(partner), int(np.array([lam], dtype=np.float32).view(np.int32)[0])]
    for t0, w in list(tmasks) + list(fmasks):
        row += [int(t0), int(w)]
    return row


def augment_formula(bank, tab, T, F, n_tmask, n_fmask, mean=None, std=None, gain=None, mask_value=0.0, events=None,
                    label_mix=0):
    """Plain loops, every operation in float64 (Python floats).  Returns (out (B, T, F), ev (B, T, K) or None) as float64."""
    tab = np.asarray(tab, dtype=np.int32)
    B = tab.shape[0]
    lam32 = table_lam(tab)

    def u(b, t, f):
        start, shift = int(tab[b, 0]), int(tab[b, 1])
        x = float(bank[start + (t - shift) % T, f])
        if mean is not None:
            x = (x - float(mean[f])) / float(std[f])
        if gain is not None:
            x = x + float(gain[b, f])
        return x

    def r(b, t, k):
        start, shift = int(tab[b, 0]), int(tab[b, 1])
        return float(events[start + (t - shift) % T, k])

    out = np.zeros((B, T, F), dtype=np.float64)
    K = None if events is None else events.shape[1]
    ev = None if events is None else np.zeros((B, T, K), dtype=np.float64)
    for b in range(B):
        p, lam = int(tab[b, 2]), float(lam32[b])
        tm = [(int(tab[b, 4 + 2 * j]), int(tab[b, 5 + 2 * j])) for j in range(n_tmask)]
        fm = [(int(tab[b, 4 + 2 * n_tmask + 2 * j]), int(tab[b, 5 + 2 * n_tmask + 2 * j])) for j in range(n_fmask)]
        for t in range(T):
            t_in = any(t0 <= t < t0 + w for t0, w in tm)
            for f in range(F):
                if t_in or any(f0 <= f < f0 + w for f0, w in fm):
                    out[b, t, f] = float(mask_value)
                elif p == b:
                    out[b, t, f] = u(b, t, f)
                else:
                    out[b, t, f] = lam * u(b, t, f) + (1.0 - lam) * u(p, t, f)
            if ev is not None:
                for k in range(K):
                    if p == b:
                        ev[b, t, k] = r(b, t, k)
                    elif label_mix == 0:
                        ev[b, t, k] = max(r(b, t, k), r(p, t, k))
                    else:
                        ev[b, t, k] = lam * r(b, t, k) + (1.0 - lam) * r(p, t, k)
    return out, ev


def augment_vectorised(bank, tab, T, F, n_tmask, n_fmask, mean=None, std=None, gain=None, mask_value=0.0, events=None,
                       label_mix=0):
    """The same definition with numpy indexing.  Returns a namespace:
      out, ev        float64, the formula (equal to augment_formula's)
      masked         (B, T, F) bool: the cells that hold mask_value
      mixed          (B,) bool: partner != b
      z32, z64       (B, T, F): the UNSHIFTED z-scored crop in fp32 arithmetic (one IEEE subtraction, one IEEE division; the raw
                     crop without mean / std) and in float64
      u32            (B, T, F) float32: shifted z32 plus the fp32 gain, ONE IEEE add (the shifted z32 itself without a gain)
      mix64, bound   (B, T, F) float64: lam * u32_b + (1 - lam) * u32_p in float64 over the fp32 u, and the derived bound
                     3 * 2^-24 * (|lam * u_b| + |(1 - lam) * u_p|): one rounding per product and one for the sum"""
    tab = np.asarray(tab, dtype=np.int32)
    bank = np.asarray(bank, dtype=np.float32)
    B = tab.shape[0]
    lam32 = table_lam(tab)
    lam = lam32.astype(np.float64)[:, None, None]
    start, shift, partner = tab[:, 0].astype(np.int64), tab[:, 1].astype(np.int64), tab[:, 2].astype(np.int64)
    ar = np.arange(T, dtype=np.int64)
    rows = start[:, None] + ar[None, :]                                    # (B, T) unshifted
    srows = start[:, None] + (ar[None, :] - shift[:, None]) % T            # (B, T) shifted
    raw = bank[rows]
    if mean is not None:
        m32, s32 = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
        z32 = (raw - m32[None, None, :]) / s32[None, None, :]
        z64 = (raw.astype(np.float64) - m32.astype(np.float64)) / s32.astype(np.float64)
    else:
        z32, z64 = raw, raw.astype(np.float64)
    assert z32.dtype == np.float32
    tsel = (ar[None, :] - shift[:, None]) % T
    zs32 = np.take_along_axis(z32, tsel[:, :, None], axis=1)
    zs64 = np.take_along_axis(z64, tsel[:, :, None], axis=1)
    if gain is not None:
        g32 = np.asarray(gain, dtype=np.float32)
        u32 = zs32 + g32[:, None, :]
        u64 = zs64 + g32.astype(np.float64)[:, None, :]
    else:
        u32, u64 = zs32, zs64
    assert u32.dtype == np.float32
    mixed = partner != np.arange(B)
    v64 = np.where(mixed[:, None, None], lam * u64 + (1.0 - lam) * u64[partner], u64)
    a, c = lam * u32.astype(np.float64), (1.0 - lam) * u32[partner].astype(np.float64)
    mix64 = a + c
    bound = 3.0 * 2.0 ** -24 * (np.abs(a) + np.abs(c))
    tmask = np.zeros((B, T), dtype=bool)
    for j in range(n_tmask):
        t0, w = tab[:, 4 + 2 * j], tab[:, 5 + 2 * j]
        tmask |= (ar[None, :] >= t0[:, None]) & (ar[None, :] < (t0 + w)[:, None])
    fmask = np.zeros((B, F), dtype=bool)
    fr = np.arange(F)
    for j in range(n_fmask):
        f0, w = tab[:, 4 + 2 * n_tmask + 2 * j], tab[:, 5 + 2 * n_tmask + 2 * j]
        fmask |= (fr[None, :] >= f0[:, None]) & (fr[None, :] < (f0 + w)[:, None])
    masked = tmask[:, :, None] | fmask[:, None, :]
    out = np.where(masked, np.float64(mask_value), v64)
    ev = None
    if events is not None:
        r = np.asarray(events, dtype=np.float64)[srows]                     # (B, T, K)
        if label_mix == 0:
            mixed_r = np.maximum(r, r[partner])
        else:
            mixed_r = lam * r + (1.0 - lam) * r[partner]
        ev = np.where(mixed[:, None, None], mixed_r, r)
    return SimpleNamespace(out=out, ev=ev, masked=masked, mixed=mixed, z32=z32, z64=z64, u32=u32, mix64=mix64, bound=bound)
