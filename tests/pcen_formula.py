"""PCEN forward and backward in float64 numpy, as plain loops over t: the formulas of include/sed_hip.h (csrc/sed_pcen.hip), the
reference of tests/test_pcen_host.py and tests/test_gpu_pcen.py.

Every output comes with its companion A: the same expression with every term replaced by its absolute value, the scale of the
rounding error of an evaluation in double.  A kernel result is accepted within 2^-23 |ref| + 2^-40 A (the one fp32 rounding plus
the slack of the project's double-arithmetic kernels)."""
import numpy as np

LN10_10 = np.log(10.0) / 10.0


def params(theta):
    """theta (4, F) = (a, d, rho, sigma) -> alpha, delta, r, s as float64 (F,)"""
    th = np.asarray(theta, dtype=np.float64)
    return np.exp(th[0]), np.exp(th[1]), np.exp(th[2]), 1.0 / (1.0 + np.exp(-th[3]))


def energy(x, kind, gain, mean=None, std=None):
    x = np.asarray(x, dtype=np.float64)
    if kind == 0:
        sc = 1.0 if std is None else np.asarray(std, dtype=np.float64)
        sh = 0.0 if mean is None else np.asarray(mean, dtype=np.float64)
        return gain * 10.0 ** ((x * sc + sh) / 10.0)
    return gain * np.maximum(x, 0.0)


def smoother(E, s):
    """M (B, T, F): M_0 = E_0, M_t = (1 - s) M_{t-1} + s E_t"""
    M = np.empty_like(E)
    M[:, 0] = E[:, 0]
    for t in range(1, E.shape[1]):
        M[:, t] = (1.0 - s) * M[:, t - 1] + s * E[:, t]
    return M


def forward(x, theta, kind, eps, gain, mean=None, std=None):
    """x (B, T, F) -> (y, A_y) float64"""
    alpha, delta, r, s = params(theta)
    E = energy(x, kind, gain, mean, std)
    M = smoother(E, s)
    G = E * (eps + M) ** (-alpha)
    y = (G + delta) ** r - delta ** r
    return y, (G + delta) ** r + delta ** r


def backward(x, theta, kind, eps, gain, g, mean=None, std=None):
    """g = dL/dy (B, T, F) -> dict: dx (B, T, F), dtheta (4, F) and their companions A_dx, A_dtheta"""
    alpha, delta, r, s = params(theta)
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    B, T, F = x.shape
    E = energy(x, kind, gain, mean, std)
    M = smoother(E, s)
    u = eps + M
    upa = u ** (-alpha)
    G = E * upa
    Gd = G + delta
    q = g * r * Gd ** (r - 1.0)
    direct = q * upa
    m = -q * alpha * G / u
    lam = np.zeros_like(E)
    Lam = np.zeros_like(E)                     # the same recurrence over |m|
    nxt = np.zeros((B, F))
    nxt_abs = np.zeros((B, F))
    for t in range(T - 1, -1, -1):
        nxt = m[:, t] + (1.0 - s) * nxt
        nxt_abs = np.abs(m[:, t]) + (1.0 - s) * nxt_abs
        lam[:, t], Lam[:, t] = nxt, nxt_abs
    w = np.broadcast_to(s, (B, T, F)).copy()   # dM_t/dE_t: s for t >= 1, 1 at t = 0
    w[:, 0] = 1.0
    dE = direct + w * lam
    dE_abs = np.abs(direct) + w * Lam
    if kind == 0:
        sc = 1.0 if std is None else np.asarray(std, dtype=np.float64)
        dEdx = E * LN10_10 * sc
    else:
        dEdx = gain * (x > 0)
    dx = dE * dEdx
    A_dx = dE_abs * np.abs(dEdx)
    Mprev = np.concatenate([np.zeros((B, 1, F)), M[:, :-1]], axis=1)
    tmask = np.ones((1, T, 1))
    tmask[:, 0] = 0.0
    terms = [(-q * G * np.log(u), alpha),
             (g * r * (Gd ** (r - 1.0) - delta ** (r - 1.0)), delta),
             (g * (Gd ** r * np.log(Gd) - delta ** r * np.log(delta)), r),
             (tmask * lam * (E - Mprev), s * (1.0 - s))]
    dtheta = np.stack([fac * term.sum(axis=(0, 1)) for term, fac in terms])
    # the companions: as for y, whose A is (G + delta)^r + delta^r, every term of a summand is taken absolute, also the two of a
    # difference inside it and the terms of lambda: a summand whose difference cancels (G = 0: exactly, in this file) is still
    # evaluated to the rounding error of its two terms
    ag = np.abs(g)
    abs_terms = [np.abs(q) * G * np.abs(np.log(u)),
                 ag * r * (Gd ** (r - 1.0) + delta ** (r - 1.0)),
                 ag * (Gd ** r * np.abs(np.log(Gd)) + delta ** r * np.abs(np.log(delta))),
                 tmask * Lam * (E + Mprev)]
    A_dtheta = np.stack([fac * term.sum(axis=(0, 1)) for term, (_, fac) in zip(abs_terms, terms)])
    return {"dx": dx, "dtheta": dtheta, "A_dx": A_dx, "A_dtheta": A_dtheta}


def bound(ref, A):
    """the acceptance bound of a kernel result per element"""
    return 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * A


def worst_ratio(got, ref, A):
    """max |got - ref| / bound over the elements (0 where both the difference and the bound are 0)"""
    got = np.asarray(got, dtype=np.float64)
    err, bnd = np.abs(got - ref), bound(ref, A)
    ratio = np.where(err == 0.0, 0.0, err / np.where(bnd > 0.0, bnd, np.finfo(np.float64).tiny))
    return float(ratio.max()) if ratio.size else 0.0
