"""The semi-supervised losses of csrc/sed_semi.hip and sed_weak_bce_fwd_bwd_ex (csrc/sed_weak.hip) as plain float64 formulas: the
definitions the kernels are tested against (tests/test_gpu_semi.py), themselves checked against torch autograd on the host
(tests/test_semi_host.py).  The pooling of the clip-level loss is tests/weak_formula.py's.

pre (B, t, K) are the pre-interpolation logits.  With N = min(t*ratio, Tt) virtual frames, row i stands for the frames
[i*ratio, i*ratio + c_i), c_i = clamp(N - i*ratio, 0, ratio).  sel is None (all clips) or (B,) of anything truthy; S = how many
clips are selected.  p = 1/(1+exp(-x)), q = 1/(1+exp(x)).
    bce_sel    l_f = -(w y_f ln sigma(x) + (1 - y_f) ln sigma(-x)), ln sigma(x) = min(x, 0) - log1p(exp(-|x|)), no clamp
               loss = weight * sum_{b in sel} sum_{f<N} sum_k l_f / (S N K)
               dpre[b,i,k] = weight * grad_scale / (S N K) * sum_{f of row i, f<N} ((1 - y_f) p - w y_f q)
    weak_ex    P, Q, dP/dp_i, Y of weak_formula; BCE: l and dl/dP of weak_formula; MSE: l = (P - Y)^2, dl/dP = 2 (P - Y)
               loss = weight * sum_{b in sel} sum_k l / (S K),  dpre_i = weight * grad_scale / (S K) * dl/dP * dP/dp_i * p_i q_i
    frame_mse  loss = weight * sum_{b in sel} sum_i c_i sum_k (p - p_T)^2 / (S N K)
               dpre[b,i,k] = weight * grad_scale / (S N K) * c_i * 2 (p - p_T) p q
    ema        teacher <- alpha * teacher + (1 - alpha) * student
Unselected clips and rows with c_i = 0 get gradient 0; S = 0 gives loss 0 and gradient 0.  Every loss returns (loss, dpre (B, t, K))."""
import math

import numpy as np

from weak_formula import clip_labels, frame_counts, weak_vectorised


def selection(sel, B):
    """(mask (B,) bool, S)"""
    m = np.ones(B, dtype=bool) if sel is None else np.asarray(sel).astype(bool)
    assert m.shape == (B,)
    return m, int(m.sum())


def _pq(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x)), 1.0 / (1.0 + np.exp(x))


def bce_sel(pre, target, sel, ratio, Tt, recall_factor, weight=1.0, grad_scale=1.0, with_abs=False):
    """with_abs: also the per-element sum of the magnitudes of the terms sed_bce_fwd_bwd, the fp32 kernel, forms the gradient from
    (what its error is relative to: tests/test_gpu_ops_exact_oracle.py, _bce_ref)"""
    pre, target = np.asarray(pre, dtype=np.float64), np.asarray(target, dtype=np.float64)
    B, t, K = pre.shape
    assert target.shape == (B, Tt, K)
    N, c = frame_counts(t, ratio, Tt)
    m, S = selection(sel, B)
    dpre, gabs = np.zeros((B, t, K)), np.zeros((B, t, K))
    if S == 0:
        return (0.0, dpre, gabs) if with_abs else (0.0, dpre)
    w = recall_factor
    p, q = _pq(pre)
    tail = np.log1p(np.exp(-np.abs(pre)))
    lsp, lsn = np.minimum(pre, 0.0) - tail, np.minimum(-pre, 0.0) - tail
    y = np.zeros((B, t * ratio, K))
    live = np.zeros((1, t * ratio, 1))
    y[:, :N], live[:, :N] = target[:, :N], 1.0
    y, live = y.reshape(B, t, ratio, K), live.reshape(1, t, ratio, 1)
    l = -(w * y * lsp[:, :, None] + (1.0 - y) * lsn[:, :, None]) * live
    g = ((1.0 - y) * p[:, :, None] - w * y * q[:, :, None]) * live
    ga = (p[:, :, None] * (1.0 + (w - 1.0) * y) + w * y) * live      # the fp32 kernel forms sigma (1 + (w - 1) y) - w y
    mm = m[:, None, None]
    den = float(S) * N * K
    loss = weight * float(l.sum(axis=2)[m].sum()) / den
    dpre = np.where(mm, weight * grad_scale / den * g.sum(axis=2), 0.0)
    if with_abs:
        return loss, dpre, np.where(mm, abs(weight * grad_scale) / den * ga.sum(axis=2), 0.0)
    return loss, dpre


def weak_ex(pre, target, sel, criterion, ratio, Tt, mode, recall_factor, weight=1.0, grad_scale=1.0):
    """criterion: 'bce' or 'mse'.  Returns (P (B, K) of every clip, loss, dpre).  The mean over the S selected clips is
    weak_formula's loss of the batch made of those clips alone."""
    assert criterion in ("bce", "mse")
    pre = np.asarray(pre, dtype=np.float64)
    target = np.asarray(target, dtype=np.float64)
    B, t, K = pre.shape
    m, S = selection(sel, B)
    P = weak_vectorised(pre, np.zeros((B, K)), ratio, Tt, mode, 1.0)[0]
    dpre = np.zeros((B, t, K))
    if S == 0:
        return P, 0.0, dpre
    if criterion == "bce":
        _, _, loss, dpre[m] = weak_vectorised(pre[m], target[m], ratio, Tt, mode, recall_factor, weight, grad_scale)
        return P, loss, dpre
    # Y = 1, w = 1: dl/dP = -1 / max(P, 1e-12), so weak_formula's gradient times -S K max(P, 1e-12) is dP/dp_i * p_i q_i
    N, _ = frame_counts(t, ratio, Tt)
    Ps, _, _, d1 = weak_vectorised(pre[m], np.ones((S, K)), ratio, Tt, mode, 1.0)
    chain = -d1 * (S * K) * np.maximum(Ps, 1e-12)[:, None, :]
    Y = clip_labels(target[m], N)
    loss = weight * float(((Ps - Y) ** 2).sum()) / (S * K)
    dpre[m] = weight * grad_scale / (S * K) * (2.0 * (Ps - Y))[:, None, :] * chain
    return P, loss, dpre


def frame_mse(pre, pre_teacher, sel, ratio, Tt, weight=1.0, grad_scale=1.0):
    pre, pt = np.asarray(pre, dtype=np.float64), np.asarray(pre_teacher, dtype=np.float64)
    B, t, K = pre.shape
    assert pt.shape == pre.shape
    N, c = frame_counts(t, ratio, Tt)
    m, S = selection(sel, B)
    if S == 0:
        return 0.0, np.zeros((B, t, K))
    p, q = _pq(pre)
    pT = _pq(pt)[0]
    cc = c.astype(np.float64)[None, :, None]
    den = float(S) * N * K
    d = p - pT
    loss = weight * float((cc * d * d)[m].sum()) / den
    dpre = np.where(m[:, None, None], weight * grad_scale / den * cc * 2.0 * d * p * q, 0.0)
    return loss, dpre


def ema(teacher, student, alpha):
    return alpha * np.asarray(teacher, dtype=np.float64) + (1.0 - alpha) * np.asarray(student, dtype=np.float64)


def ema_factor(n, ema_decay):
    """alpha_n after the n-th step, n = 1, 2, ...: min(1 - 1/n, ema_decay)"""
    return min(1.0 - 1.0 / n, ema_decay)


def rampup(n, weight, R):
    """the consistency weight at step n: weight * exp(-5 (1 - min(n, R)/R)^2) for R > 0, constant for R = 0"""
    if R <= 0:
        return float(weight)
    return float(weight) * math.exp(-5.0 * (1.0 - min(n, R) / R) ** 2)
