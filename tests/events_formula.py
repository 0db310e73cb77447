"""The event decoding of csrc/sed_events.hip restated in plain numpy / Python loops, as the tests' reference (no kernel of the library
serves as one): the median filter with its reflection index, the hysteresis decoder as a per-row loop over frames, the segment
counts, and a brute-force maximum matching for the event-based counts."""
import math

import numpy as np


def reflect_index(i, T):
    """half-sample-symmetric reflection (scipy's mode='reflect'): i mod 2T, then i if < T else 2T - 1 - i"""
    m = i % (2 * T)             # Python's % is non-negative for a positive modulus
    return m if m < T else 2 * T - 1 - m


def median_formula(x, win):
    """x (B, T, K): out[b, t, k] = the middle one of the sorted win values x[b, r(t + j), k], j = -h .. h"""
    x = np.asarray(x)
    B, T, K = x.shape
    h = win // 2
    out = np.empty_like(x)
    for t in range(T):
        idx = [reflect_index(t + j, T) for j in range(-h, h + 1)]
        out[:, t, :] = np.sort(x[:, idx, :], axis=1)[:, h, :]
    return out


def decode_row(p, th_hi, th_lo, max_gap, min_len):
    """One row p (T,) fp32 -> list of (onset, offset) with the offset exclusive.  Comparisons are strict, in fp32."""
    p = np.asarray(p, dtype=np.float32)
    above_lo, above_hi = (p > np.float32(th_lo)).tolist(), (p > np.float32(th_hi)).tolist()
    T = len(p)
    # 1. candidate runs of p > lo, kept when a frame exceeds hi
    kept, t = [], 0
    while t < T:
        if above_lo[t]:
            s, seen = t, False
            while t < T and above_lo[t]:
                seen = seen or above_hi[t]
                t += 1
            if seen:
                kept.append([s, t])
        else:
            t += 1
    # 2. merge kept runs with at most max_gap inactive frames between them (chains)
    merged = []
    for s, e in kept:
        if merged and s - merged[-1][1] <= max_gap:
            merged[-1][1] = e
        else:
            merged.append([s, e])
    # 3. drop what is shorter than min_len
    return [(s, e) for s, e in merged if e - s >= min_len]


def decode_formula(prob, th_hi, th_lo, max_gap, min_len):
    """prob (B, T, K) -> events (n, 4) int32 rows (b, k, onset, offset) in ascending (b, k, onset) order, row_counts (B*K,) int32,
    total, decisions (B, T, K) uint8"""
    prob = np.asarray(prob, dtype=np.float32)
    B, T, K = prob.shape
    events, counts = [], []
    dec = np.zeros((B, T, K), dtype=np.uint8)
    for b in range(B):
        for k in range(K):
            ev = decode_row(prob[b, :, k], th_hi, th_lo, max_gap, min_len)
            counts.append(len(ev))
            for s, e in ev:
                events.append((b, k, s, e))
                dec[b, s:e, k] = 1
    return (np.asarray(events, dtype=np.int32).reshape(-1, 4), np.asarray(counts, dtype=np.int32), len(events), dec)


def segment_counts_formula(dec, target, seg_frames):
    """dec (B, T, K) 0/1, target (B, Tt, K): (K, 3) int64 (TP, FP, FN) over segments of seg_frames frames of the first min(T, Tt)"""
    dec, target = np.asarray(dec), np.asarray(target)
    B, T, K = dec.shape
    n = min(T, target.shape[1])
    out = np.zeros((K, 3), dtype=np.int64)
    for b in range(B):
        for s0 in range(0, n, seg_frames):
            s1 = min(s0 + seg_frames, n)
            for k in range(K):
                pa = bool((dec[b, s0:s1, k] != 0).any())
                ra = bool((target[b, s0:s1, k] > 0.5).any())
                out[k] += (pa and ra, pa and not ra, ra and not pa)
    return out


def compatible(p, r, collar, offset_pct=0.5):
    """p, r: (onset, offset)"""
    tol = max(collar, math.ceil(offset_pct * (r[1] - r[0])))
    return abs(p[0] - r[0]) <= collar and abs(p[1] - r[1]) <= tol


def brute_force_matching(pred, ref, collar, offset_pct=0.5):
    """Size of a maximum matching between two lists of (onset, offset), at most 6 per side: EVERY assignment is tried -- each
    predicted event in turn stays unmatched or takes any still-free reference event (at most 13327 assignments for 6 x 6)."""
    assert len(pred) <= 6 and len(ref) <= 6
    ok = [[compatible(p, r, collar, offset_pct) for r in ref] for p in pred]

    def best_from(i, used):
        if i == len(pred):
            return 0
        best = best_from(i + 1, used)                       # pred[i] unmatched
        for j in range(len(ref)):
            if ok[i][j] and j not in used:
                best = max(best, 1 + best_from(i + 1, used | {j}))
        return best

    return best_from(0, frozenset())


def greedy_matching(pred, ref, collar, offset_pct=0.5):
    """First fit in time order: each predicted event, by onset, takes the earliest still-free compatible reference event."""
    used, n = set(), 0
    for p in sorted(pred):
        for j, r in sorted(enumerate(ref), key=lambda jr: jr[1]):
            if j not in used and compatible(p, r, collar, offset_pct):
                used.add(j)
                n += 1
                break
    return n
