"""The PSDS definition of include/sed_hip.h as plain loops over explicit event lists (numpy / float64, host only): the reference of
tests/test_psds_host.py and tests/test_gpu_psds.py.  Intersections are computed by counting frames of boolean arrays -- no bit
words, no popcounts -- so nothing here is shared with csrc/sed_psds.hip.

  runs(mask)                                  the maximal runs of True as (onset, offset) pairs, offset exclusive
  psds_counts(prob, target, th, dtc, gtc, cttc)   counts int64 (nth, K, K + 3) and gt int64 (K, 2) of one call
  curve_value(points, e), psds_exact(class_points, alpha_st, e_max)   the score's step functions integrated in exact Fractions
"""
from fractions import Fraction

import numpy as np


def runs(mask):
    """[(onset, offset)] of the maximal runs of True in a 1-D boolean array, offset exclusive, ascending"""
    mask = np.asarray(mask, dtype=bool)
    if mask.size == 0:
        return []
    edge = np.diff(np.concatenate(([0], mask.astype(np.int8), [0])))
    return list(zip(np.flatnonzero(edge == 1).tolist(), np.flatnonzero(edge == -1).tolist()))


def psds_counts(prob, target, th, dtc, gtc, cttc):
    """prob (B, T, K) fp32, target (B, Tt, K) fp32, th nth fp32 thresholds, criteria (num, den) ->
    counts (nth, K, K + 3) = (tp, fp, ndet, ct[0..K-1]) and gt (K, 2) = (events, frames), int64."""
    prob = np.asarray(prob, dtype=np.float32)
    target = np.asarray(target, dtype=np.float32)
    th = np.asarray(th, dtype=np.float32).reshape(-1)
    B, T, K = prob.shape
    n = min(T, target.shape[1])
    counts = np.zeros((len(th), K, K + 3), dtype=np.int64)
    gt = np.zeros((K, 2), dtype=np.int64)
    for b in range(B):
        tgt = target[b, :n] > np.float32(0.5)                   # (n, K)
        gt_events = [runs(tgt[:, c]) for c in range(K)]
        for c in range(K):
            gt[c, 0] += len(gt_events[c])
            gt[c, 1] += sum(e - a for a, e in gt_events[c])
        for i in range(len(th)):
            with np.errstate(invalid="ignore"):
                det = prob[b, :n] > th[i]                       # fp32, strict; a NaN compares False
            for k in range(K):
                covered = np.zeros(n, dtype=bool)               # frames under RELEVANT detections of class k
                for a, e in runs(det[:, k]):
                    length = e - a
                    counts[i, k, 2] += 1
                    per_class = np.count_nonzero(tgt[a:e], axis=0)        # d's frames with each class's target on
                    if int(per_class[k]) * dtc[1] >= dtc[0] * length:
                        covered[a:e] = True
                    else:
                        counts[i, k, 1] += 1
                        for c in range(K):
                            if c != k and int(per_class[c]) * cttc[1] >= cttc[0] * length:
                                counts[i, k, 3 + c] += 1
                for a, e in gt_events[k]:
                    if int(np.count_nonzero(covered[a:e])) * gtc[1] >= gtc[0] * (e - a):
                        counts[i, k, 0] += 1
    return counts, gt


def curve_value(points, e):
    """The class curve through `points` = [(efpr, tpr)] at e, exactly: sorted by (efpr, tpr), tpr replaced by its running maximum,
    the largest such tpr among the points with efpr <= e, 0 if there is none."""
    best = Fraction(0)
    for x, t in sorted((Fraction(x), Fraction(t)) for x, t in points):
        if x <= e:
            best = max(best, t)
    return best


def fraction_sqrt(v):
    """The exact square root of a Fraction that has one (the test cases are chosen so)"""
    from math import isqrt
    num, den = isqrt(v.numerator), isqrt(v.denominator)
    assert num * num == v.numerator and den * den == v.denominator, f"{v} has no rational square root"
    return Fraction(num, den)


def psds_exact(class_points, alpha_st, e_max):
    """Exact PSDS of the scored classes' point lists [[(efpr, tpr)]] (Fractions): the common axis is every efpr in [0, e_max], sorted
    and unique, then e_max; on [e_j, e_j+1) the value is max(mean_k - alpha_st * std_k, 0) of the class curves at e_j (population
    standard deviation); the integral over [0, e_max] divided by e_max.  Also returns the per-class areas / e_max."""
    alpha_st, e_max = Fraction(alpha_st), Fraction(e_max)
    axis = sorted({Fraction(x) for pts in class_points for x, _ in pts if 0 <= Fraction(x) <= e_max}) + [e_max]
    total, areas = Fraction(0), [Fraction(0)] * len(class_points)
    for j in range(len(axis) - 1):
        vals = [curve_value(pts, axis[j]) for pts in class_points]
        mean = sum(vals) / len(vals)
        std = fraction_sqrt(sum((v - mean) ** 2 for v in vals) / len(vals))
        width = axis[j + 1] - axis[j]
        total += max(mean - alpha_st * std, Fraction(0)) * width
        areas = [a + v * width for a, v in zip(areas, vals)]
    return total / e_max, [a / e_max for a in areas]
