"""The weak-label (clip-level) loss of csrc/sed_weak.hip as a plain float64 formula: the definition the kernels are tested against
(tests/test_gpu_weak.py) and that is itself checked against torch autograd on the host (tests/test_weak_host.py).

pre (B, t, K) are the pre-interpolation logits.  With N = min(t*ratio, Tt) virtual frames, row i stands for
c_i = clamp(N - i*ratio, 0, ratio) frames; rows with c_i = 0 take no part, not in the max either, and get gradient 0.
For one (b, k), x_i the logit:
    p_i = 1/(1+exp(-x_i)),  q_i = 1/(1+exp(x_i))
    max     P = p_j, Q = q_j, j the smallest index of the largest x_i among c_i > 0          dP/dp_i = [i == j]
    mean    P = sum c_i p_i / N,  Q = sum c_i q_i / N                                         dP/dp_i = c_i / N
    linear  P = S2/S1, S1 = sum c_i p_i, S2 = sum c_i p_i^2, Q = sum c_i p_i q_i / S1         dP/dp_i = c_i (2 p_i - P) / S1
            (S1 == 0: P = 0, Q = 1, gradient 0)
    exp     P = sum c_i p_i e^{p_i} / E, E = sum c_i e^{p_i}, Q = sum c_i q_i e^{p_i} / E     dP/dp_i = c_i e^{p_i} (1 + p_i - P) / E
    l = -(w Y max(ln P, -100) + (1 - Y) max(ln Q, -100)),  loss = weight * mean over B*K of l
    dl/dP = -w Y / max(P, 1e-12) + (1 - Y) / max(Q, 1e-12)
    dpre_i = weight * grad_scale / (B*K) * dl/dP * dP/dp_i * p_i q_i
target is (B, K) clip labels, or the strong (B, Tt, K) tensor, of which Y is the maximum over the first N frames.
Both functions return (P (B, K), Y (B, K), loss, dpre (B, t, K)) in float64."""
import math

import numpy as np

MODES = ("max", "mean", "linear", "exp")


def frame_counts(t, ratio, Tt):
    """(N, c (t,) int): the virtual frames and how many each row of pre stands for"""
    N = min(t * ratio, Tt)
    return N, np.clip(N - np.arange(t) * ratio, 0, ratio)


def clip_labels(target, N):
    target = np.asarray(target, dtype=np.float64)
    return target if target.ndim == 2 else target[:, :N].max(axis=1)


def _exp(v):
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


def _log(v):
    return math.log(v) if v > 0.0 else -math.inf


def weak_loop(pre, target, ratio, Tt, mode, recall_factor, weight=1.0, grad_scale=1.0):
    assert mode in MODES
    pre = np.asarray(pre, dtype=np.float64)
    B, t, K = pre.shape
    N, c = frame_counts(t, ratio, Tt)
    Y = clip_labels(target, N)
    P = np.zeros((B, K))
    dpre = np.zeros((B, t, K))
    total = 0.0
    for b in range(B):
        for k in range(K):
            rows = [i for i in range(t) if c[i] > 0]
            x = [float(pre[b, i, k]) for i in rows]
            cc = [float(c[i]) for i in rows]
            p = [1.0 / (1.0 + _exp(-v)) for v in x]
            q = [1.0 / (1.0 + _exp(v)) for v in x]
            n = len(rows)
            dP = [0.0] * n
            if mode == "max":
                j = 0
                for i in range(1, n):
                    if x[i] > x[j]:
                        j = i
                Pv, Qv = p[j], q[j]
                dP[j] = 1.0
            elif mode == "mean":
                Pv = sum(cc[i] * p[i] for i in range(n)) / N
                Qv = sum(cc[i] * q[i] for i in range(n)) / N
                dP = [cc[i] / N for i in range(n)]
            elif mode == "linear":
                S1 = sum(cc[i] * p[i] for i in range(n))
                if S1 == 0.0:
                    Pv, Qv = 0.0, 1.0
                else:
                    Pv = sum(cc[i] * p[i] * p[i] for i in range(n)) / S1
                    Qv = sum(cc[i] * p[i] * q[i] for i in range(n)) / S1
                    dP = [cc[i] * (2.0 * p[i] - Pv) / S1 for i in range(n)]
            else:
                e = [math.exp(v) for v in p]
                E = sum(cc[i] * e[i] for i in range(n))
                Pv = sum(cc[i] * p[i] * e[i] for i in range(n)) / E
                Qv = sum(cc[i] * q[i] * e[i] for i in range(n)) / E
                dP = [cc[i] * e[i] * (1.0 + p[i] - Pv) / E for i in range(n)]
            y = float(Y[b, k])
            total += -(recall_factor * y * max(_log(Pv), -100.0) + (1.0 - y) * max(_log(Qv), -100.0))
            dl = -recall_factor * y / max(Pv, 1e-12) + (1.0 - y) / max(Qv, 1e-12)
            P[b, k] = Pv
            for i in range(n):
                dpre[b, rows[i], k] = weight * grad_scale / (B * K) * dl * dP[i] * (p[i] * q[i])
    return P, Y, weight * total / (B * K), dpre


def weak_vectorised(pre, target, ratio, Tt, mode, recall_factor, weight=1.0, grad_scale=1.0):
    assert mode in MODES
    pre = np.asarray(pre, dtype=np.float64)
    B, t, K = pre.shape
    N, c = frame_counts(t, ratio, Tt)
    Y = clip_labels(target, N)
    n = int((c > 0).sum())
    x = pre[:, :n]
    cc = c[:n].astype(np.float64)[None, :, None]
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-x))
        q = 1.0 / (1.0 + np.exp(x))
    if mode == "max":
        j = x.argmax(axis=1)                                   # the first of equals
        P = np.take_along_axis(p, j[:, None, :], axis=1)[:, 0]
        Q = np.take_along_axis(q, j[:, None, :], axis=1)[:, 0]
        dP = (np.arange(n)[None, :, None] == j[:, None, :]).astype(np.float64)
    elif mode == "mean":
        P = (cc * p).sum(axis=1) / N
        Q = (cc * q).sum(axis=1) / N
        dP = np.broadcast_to(cc / N, x.shape)
    elif mode == "linear":
        S1 = (cc * p).sum(axis=1)
        dead = S1 == 0.0
        S1s = np.where(dead, 1.0, S1)
        P = np.where(dead, 0.0, (cc * p * p).sum(axis=1) / S1s)
        Q = np.where(dead, 1.0, (cc * p * q).sum(axis=1) / S1s)
        dP = np.where(dead[:, None, :], 0.0, cc * (2.0 * p - P[:, None, :]) / S1s[:, None, :])
    else:
        e = np.exp(p)
        E = (cc * e).sum(axis=1)
        P = (cc * p * e).sum(axis=1) / E
        Q = (cc * q * e).sum(axis=1) / E
        dP = cc * e * (1.0 + p - P[:, None, :]) / E[:, None, :]
    with np.errstate(divide="ignore"):
        l = -(recall_factor * Y * np.maximum(np.log(P), -100.0) + (1.0 - Y) * np.maximum(np.log(Q), -100.0))
    dl = -recall_factor * Y / np.maximum(P, 1e-12) + (1.0 - Y) / np.maximum(Q, 1e-12)
    dpre = np.zeros((B, t, K))
    dpre[:, :n] = weight * grad_scale / (B * K) * dl[:, None, :] * dP * (p * q)
    return P, Y, weight * float(l.sum()) / (B * K), dpre
