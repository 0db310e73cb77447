"""The attention pooling head of csrc/sed_attn.hip as plain float64 formulas: the definition the kernels are tested against
(tests/test_gpu_att.py) and that is itself checked against torch autograd on the host (tests/test_att_host.py).

pre, att (B, t, K) are the frame and attention logits before interpolate().  With N = min(t*ratio, Tt) virtual frames, row i
stands for c_i = clamp(N - i*ratio, 0, ratio) frames; rows with c_i = 0 take no part, not in the maximum either.
For one (b, k), x_i = pre, a_i = att:
    p_i = 1/(1+exp(-x_i)),  q_i = 1/(1+exp(x_i))
    e_i = exp(a_i - a_max), a_max over the rows with c_i > 0               (a softmax over time, per class)
    Z = sum c_i e_i,  P = sum c_i e_i p_i / Z,  Q = sum c_i e_i q_i / Z    (Q from its own sum)
    "bce"  l = -(w Y max(ln P, -100) + (1 - Y) max(ln Q, -100)),  dl/dP = -w Y / max(P, 1e-12) + (1 - Y) / max(Q, 1e-12)
    "mse"  l = (P - Y)^2,  dl/dP = 2 (P - Y)
    loss = weight * mean of l over B*K, or over S*K for the S clips of a selection (S = 0: loss 0, gradient 0)
    coef = weight * grad_scale / (B*K), or / (S*K)
    dpre_i = coef * dl/dP * (c_i e_i / Z) * p_i q_i
    datt_i = coef * dl/dP * c_i e_i (p_i - P) / Z
target is (B, K) clip labels, or the strong (B, Tt, K) tensor, of which Y is the maximum over the first N frames.
att_loop and att_vectorised return a dict: P, Y (B, K), loss, dpre, datt (B, t, K) in float64, and A_P, A_loss, A_dpre, A_datt: the
same expressions over absolute values (p_i + P in place of p_i - P, |ln| and (P + Y) in the criteria), the scale of the gate

    |got - ref| <= 2^-23 |ref| + 2^-40 A + 2^-150

(double arithmetic whose rounding errors are relative to the terms that are added and subtracted, then ONE rounding to fp32:
relative 2^-24, and half a step of the subnormal grid, 2^-150, where the result lies below fp32's normal range)."""
import math

import numpy as np

from weak_formula import clip_labels, frame_counts

CRITERIA = ("bce", "mse")


def _exp(v):
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


def _log(v):
    return math.log(v) if v > 0.0 else -math.inf


def _divisor(B, K, sel):
    """(the clips that take part (B,) bool, S*K or 0)"""
    on = np.ones(B, dtype=bool) if sel is None else np.asarray(sel) != 0
    return on, int(on.sum()) * K


def att_loop(pre, att, target, ratio, Tt, recall_factor, weight=1.0, grad_scale=1.0, criterion="bce", sel=None):
    assert criterion in CRITERIA
    pre, att = np.asarray(pre, dtype=np.float64), np.asarray(att, dtype=np.float64)
    B, t, K = pre.shape
    N, c = frame_counts(t, ratio, Tt)
    Y = clip_labels(target, N)
    on, div = _divisor(B, K, sel)
    out = {n: np.zeros((B, K)) for n in ("P", "A_P")}
    out.update({n: np.zeros((B, t, K)) for n in ("dpre", "datt", "A_dpre", "A_datt")})
    total = atotal = 0.0
    w = recall_factor
    for b in range(B):
        for k in range(K):
            rows = [i for i in range(t) if c[i] > 0]
            p = [1.0 / (1.0 + _exp(-float(pre[b, i, k]))) for i in rows]
            q = [1.0 / (1.0 + _exp(float(pre[b, i, k]))) for i in rows]
            amax = max(float(att[b, i, k]) for i in rows)
            ce = [float(c[i]) * math.exp(float(att[b, i, k]) - amax) for i in rows]
            Z = sum(ce)
            Pv = sum(ce[j] * p[j] for j in range(len(rows))) / Z
            Qv = sum(ce[j] * q[j] for j in range(len(rows))) / Z
            out["P"][b, k] = out["A_P"][b, k] = Pv
            if not on[b] or div == 0:
                continue
            y = float(Y[b, k])
            if criterion == "bce":
                lp, lq = max(_log(Pv), -100.0), max(_log(Qv), -100.0)
                total += -(w * y * lp + (1.0 - y) * lq)
                atotal += w * abs(y) * abs(lp) + abs(1.0 - y) * abs(lq)
                dl = -w * y / max(Pv, 1e-12) + (1.0 - y) / max(Qv, 1e-12)
                adl = w * abs(y) / max(Pv, 1e-12) + abs(1.0 - y) / max(Qv, 1e-12)
            else:
                total += (Pv - y) ** 2
                atotal += (Pv + abs(y)) ** 2
                dl, adl = 2.0 * (Pv - y), 2.0 * (Pv + abs(y))
            coef = weight * grad_scale / div
            for j, i in enumerate(rows):
                out["dpre"][b, i, k] = coef * dl * (ce[j] / Z) * (p[j] * q[j])
                out["A_dpre"][b, i, k] = abs(coef) * adl * (ce[j] / Z) * (p[j] * q[j])
                out["datt"][b, i, k] = coef * dl * ce[j] * (p[j] - Pv) / Z
                out["A_datt"][b, i, k] = abs(coef) * adl * ce[j] * (p[j] + Pv) / Z
    out["Y"] = Y
    out["loss"] = weight * total / div if div else 0.0
    out["A_loss"] = abs(weight) * atotal / div if div else 0.0
    return out


def att_vectorised(pre, att, target, ratio, Tt, recall_factor, weight=1.0, grad_scale=1.0, criterion="bce", sel=None):
    assert criterion in CRITERIA
    pre, att = np.asarray(pre, dtype=np.float64), np.asarray(att, dtype=np.float64)
    B, t, K = pre.shape
    N, c = frame_counts(t, ratio, Tt)
    Y = clip_labels(target, N)
    on, div = _divisor(B, K, sel)
    n = int((c > 0).sum())
    x, a = pre[:, :n], att[:, :n]
    cc = c[:n].astype(np.float64)[None, :, None]
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-x))
        q = 1.0 / (1.0 + np.exp(x))
    ce = cc * np.exp(a - a.max(axis=1, keepdims=True))
    Z = ce.sum(axis=1)
    P = (ce * p).sum(axis=1) / Z
    Q = (ce * q).sum(axis=1) / Z
    w = recall_factor
    if criterion == "bce":
        with np.errstate(divide="ignore"):
            lp, lq = np.maximum(np.log(P), -100.0), np.maximum(np.log(Q), -100.0)
        l = -(w * Y * lp + (1.0 - Y) * lq)
        al = w * np.abs(Y) * np.abs(lp) + np.abs(1.0 - Y) * np.abs(lq)
        dl = -w * Y / np.maximum(P, 1e-12) + (1.0 - Y) / np.maximum(Q, 1e-12)
        adl = w * np.abs(Y) / np.maximum(P, 1e-12) + np.abs(1.0 - Y) / np.maximum(Q, 1e-12)
    else:
        l, al = (P - Y) ** 2, (P + np.abs(Y)) ** 2
        dl, adl = 2.0 * (P - Y), 2.0 * (P + np.abs(Y))
    out = {"P": P, "A_P": P.copy(), "Y": Y}
    for name in ("dpre", "datt", "A_dpre", "A_datt"):
        out[name] = np.zeros((B, t, K))
    if div:
        coef = weight * grad_scale / div
        m = on[:, None, None].astype(np.float64)
        wgt = ce / Z[:, None, :]
        out["dpre"][:, :n] = m * (coef * dl[:, None, :] * wgt * (p * q))
        out["A_dpre"][:, :n] = m * (abs(coef) * adl[:, None, :] * wgt * (p * q))
        out["datt"][:, :n] = m * (coef * dl[:, None, :] * ce * (p - P[:, None, :]) / Z[:, None, :])
        out["A_datt"][:, :n] = m * (abs(coef) * adl[:, None, :] * ce * (p + P[:, None, :]) / Z[:, None, :])
    out["loss"] = weight * float(l[on].sum()) / div if div else 0.0
    out["A_loss"] = abs(weight) * float(al[on].sum()) / div if div else 0.0
    return out


def gate(got, ref, A):
    """(passes, worst error / bound) of the module docstring's gate, per element"""
    got, ref, A = (np.asarray(v, dtype=np.float64) for v in (got, ref, A))
    if not (np.isfinite(got).all() and np.isfinite(ref).all()):
        return False, math.inf
    bound = 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * A + 2.0 ** -150
    err = np.abs(got - ref)
    return bool((err <= bound).all()), float((err / bound).max()) if err.size else 0.0


# ---- the linear layer and the backward of both heads ---------------------------------------------------------------------------------
def linear_fwd(m, w, b):
    """att (rows, K) = b + m[:, :C] @ w.T and the scale of its dot-product bound, |m| @ |w|.T + |b|  (m (rows, Cp), w (K, C))"""
    m, w, b = (np.asarray(v, dtype=np.float64) for v in (m, w, b))
    C = w.shape[1]
    return b[None, :] + m[:, :C] @ w.T, np.abs(m[:, :C]) @ np.abs(w).T + np.abs(b)[None, :]


def linear_bwd(d, m, C):
    """(dw (K, C), db (K,), scale of dw: |d|.T @ |m|, scale of db: sum |d|) for the gradient d (rows, K) of a layer fed by m"""
    d, m = np.asarray(d, dtype=np.float64), np.asarray(m, dtype=np.float64)[:, :C]
    return d.T @ m, d.sum(axis=0), np.abs(d).T @ np.abs(m), np.abs(d).sum(axis=0)


def feature_grad(dpre, datt, fc_w, att_w, Wf):
    """((dpre @ fc_w + datt @ att_w) / Wf (rows, C), the same over absolute values)"""
    dpre, datt, fc_w, att_w = (np.asarray(v, dtype=np.float64) for v in (dpre, datt, fc_w, att_w))
    return (dpre @ fc_w + datt @ att_w) / Wf, (np.abs(dpre) @ np.abs(fc_w) + np.abs(datt) @ np.abs(att_w)) / Wf
