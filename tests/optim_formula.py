"""The grouped optimizer step in float64 numpy: the learning-rate schedule, one Adam / AdamW step over parameter groups (scale,
weight decay, frozen; amsgrad on or off; the clip factor) and the clipping norm over the non-frozen groups.  Written from the issue's
definitions and torch.optim's documented single-tensor algorithm, not from the package's code; tests/test_optim_groups_host.py checks it
against torch.optim.Adam / AdamW with real param_groups and torch.optim.lr_scheduler.LambdaLR."""
import math

import numpy as np

KINDS = ("const", "step", "cosine", "linear", "invsqrt")


def lr_at(base_lr, s, kind, warmup=0, total=0, every=200, gamma=0.997, floor=0.0):
    """lr(s) = base_lr * w(s) * d(s) for the 1-based step s; w(s) = min(1, s / warmup) with a warm-up, else 1"""
    assert s >= 1 and kind in KINDS
    W = warmup
    w = min(1.0, s / W) if W > 0 else 1.0
    if kind == "const":
        d = 1.0
    elif kind == "step":
        d = gamma ** ((s - 1) // every)
    elif kind == "invsqrt":
        d = math.sqrt(max(W, 1) / max(s, W, 1))
    else:
        u = min(1.0, max(0.0, (s - W) / (total - W)))
        d = floor + (1.0 - floor) * (0.5 * (1.0 + math.cos(math.pi * u)) if kind == "cosine" else 1.0 - u)
    return base_lr * w * d


def grouped_norm(g, group_of, specs, grad_scale=1.0):
    """||g * grad_scale||_2 over the elements of the non-frozen groups.  group_of: the group index per element; specs[k] =
    (lr_scale, weight_decay, frozen)"""
    g = np.asarray(g, dtype=np.float64) * grad_scale
    live = ~np.asarray([specs[k][2] for k in group_of], dtype=bool)
    return float(np.sqrt(np.sum(g[live] ** 2)))


def clip_coef(norm, max_norm):
    """clip_grad_norm_'s factor"""
    return min(1.0, max_norm / (norm + 1e-6))


def grouped_adam_step(p, g, m, v, vmax, group_of, specs, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, decoupled=False, coef=1.0,
                      grad_scale=1.0):
    """One step of torch.optim.Adam (decoupled False: weight decay added to the gradient) or AdamW (True: p *= 1 - lr wd first) with
    per-group lr = lr * lr_scale and weight decay; vmax None: amsgrad off.  A frozen group's elements keep p, m, v, vmax whatever g
    holds.  Returns new (p, m, v, vmax) as float64 arrays."""
    p, g, m, v = (np.array(a, dtype=np.float64) for a in (p, g, m, v))
    x = None if vmax is None else np.array(vmax, dtype=np.float64)
    group_of = np.asarray(group_of)
    scale = np.asarray([specs[k][0] for k in group_of], dtype=np.float64)
    wd = np.asarray([specs[k][1] for k in group_of], dtype=np.float64)
    live = ~np.asarray([specs[k][2] for k in group_of], dtype=bool)
    with np.errstate(all="ignore"):
        gr = g * grad_scale * coef
        lrg = lr * scale
        p1 = p.copy()
        if decoupled:
            p1 = np.where(wd != 0.0, p * (1.0 - lrg * wd), p)
        else:
            gr = np.where(wd != 0.0, gr + wd * p, gr)
        m1 = m + (1.0 - beta1) * (gr - m)
        v1 = beta2 * v + (1.0 - beta2) * gr * gr
        d = v1
        if x is not None:
            x1 = np.maximum(x, v1)
            d = x1
        denom = np.sqrt(d) / math.sqrt(1.0 - beta2 ** step) + eps
        p1 = p1 - (lrg / (1.0 - beta1 ** step)) * m1 / denom
    out_p, out_m, out_v = np.where(live, p1, p), np.where(live, m1, m), np.where(live, v1, v)
    out_x = None if x is None else np.where(live, x1, x)
    return out_p, out_m, out_v, out_x
