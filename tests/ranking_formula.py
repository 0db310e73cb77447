"""The rank metrics of csrc/sed_rank.hip as plain float64 / integer loops (the definitions of include/sed_hip.h, nothing else).

pack_formula    scores / targets (rows, K) -> keys (K, n) uint32 and invalid (K,): n = min(rows), positive = target > 0.5, valid =
                0 <= p <= 1 in fp32, key = (bits(p + 0.0f) << 1) | positive, invalid scores packed as key 0 and counted.
curve_formula   one row of keys (any order) -> P, n, auc2, best_tp, best_npred, groups, best_score, AP: sort, walk from the highest
                score down, one step per tie group (equal key >> 1).  AP terms are (tp_g / P) * (TP_g / n_g) in float64, summed with
                math.fsum (the correctly rounded sum); everything else is Python integers.
No library call and no vectorised shortcut: tests/test_ranking_host.py checks these loops against the pairwise definition of AUC,
against exact fractions and against sklearn."""
import math

import numpy as np


def pack_formula(score, target):
    score = np.asarray(score, dtype=np.float32)
    target = np.asarray(target, dtype=np.float32)
    K = score.shape[1]
    n = min(score.shape[0], target.shape[0])
    keys = np.zeros((K, n), dtype=np.uint32)
    invalid = np.zeros(K, dtype=np.int64)
    zero = np.float32(0.0)
    for k in range(K):
        for i in range(n):
            p = np.float32(score[i, k])
            if not (p >= zero and p <= np.float32(1.0)):        # NaN fails both comparisons
                invalid[k] += 1
                continue
            bits = int(np.array(p + zero, dtype=np.float32).view(np.uint32))     # -0 + 0 = +0
            keys[k, i] = (bits << 1) | (1 if target[i, k] > np.float32(0.5) else 0)
    return keys, invalid


def key_score(key):
    """the fp32 score of a key"""
    return np.array(int(key) >> 1, dtype=np.uint32).view(np.float32)[()]


def curve_formula(keys):
    ks = sorted(int(v) for v in np.asarray(keys).reshape(-1))
    n = len(ks)
    P = sum(k & 1 for k in ks)
    out = {"P": P, "n": n, "auc2": 0, "best_tp": 0, "best_npred": 0, "groups": 0, "best_score": np.float32(1.0),
           "AP": float("nan"), "terms": []}
    TP, seen, i = 0, 0, n - 1
    best = None                                  # (TP_g, n_g, score bits)
    while i >= 0:
        bits = ks[i] >> 1
        tp = fp = 0
        while i >= 0 and (ks[i] >> 1) == bits:
            if ks[i] & 1:
                tp += 1
            else:
                fp += 1
            i -= 1
        out["auc2"] += fp * (2 * TP + tp)
        TP += tp
        seen += tp + fp
        out["groups"] += 1
        if P > 0:
            if tp > 0:
                out["terms"].append((float(tp) / float(P)) * (float(TP) / float(seen)))
            # F1_g = 2 TP / (seen + P): exact comparison; a tie keeps the earlier (higher-score) group
            if best is None or TP * (best[1] + P) > best[0] * (seen + P):
                best = (TP, seen, bits)
    if P > 0:
        out["AP"] = math.fsum(out["terms"])
        out["best_tp"], out["best_npred"] = best[0], best[1]
        out["best_score"] = np.array(best[2], dtype=np.uint32).view(np.float32)[()]
    return out


COUNT_NAMES = ("P", "n", "auc2", "best_tp", "best_npred", "groups")


def counts_row(res):
    return [int(res[name]) for name in COUNT_NAMES]


def rank_formula(score, target):
    """per-class list of curve_formula results for (rows, K) scores and targets; raises on an invalid score like the wrapper"""
    keys, invalid = pack_formula(score, target)
    if invalid.any():
        raise ValueError(f"invalid scores per class: {invalid.tolist()}")
    return [curve_formula(row) for row in keys]


def auc_pairwise(score, label):
    """P(positive outscores negative) + P(tie) / 2 over all positive-negative pairs, as an exact Fraction (None if undefined)"""
    from fractions import Fraction
    pos = [float(s) for s, l in zip(score, label) if l]
    neg = [float(s) for s, l in zip(score, label) if not l]
    if not pos or not neg:
        return None
    twice = 0
    for a in pos:
        for b in neg:
            twice += 2 if a > b else (1 if a == b else 0)
    return Fraction(twice, 2 * len(pos) * len(neg))
