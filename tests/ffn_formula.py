"""The feed-forward sub-layer of csrc/sed_ffn.hip and the post-LN encoder stack around it as plain numpy formulas: the definition the
kernels are tested against (tests/test_gpu_ffn.py, tests/test_gpu_sa_encoder.py) and that is itself checked against
torch.nn.TransformerEncoderLayer / TransformerEncoder in float64 on the host (tests/test_ffn_host.py).

FFN.  x (R, C), w1 (D, C), b1 (D), w2 (C, D), b2 (C):
    u = x w1^T + b1,   a = act(u),   y = a w2^T + b2
    act: "relu" max(u, 0);  "gelu" the erf form 0.5 u (1 + erf(u / sqrt 2)) = u Phi(u)
    backward from dy:  da = dy w2,  du = da act'(u)  (relu: 1 for u > 0 else 0;  gelu: Phi(u) + u phi(u)),
                       dw2 = dy^T a,  db2 = sum_rows dy,  dw1 = du^T x,  db1 = sum_rows du,  dx = du w1
Layer l (post-LN, torch.nn.TransformerEncoderLayer(C, H, D, dropout=0, batch_first=True, norm_first=False)):
    h1 = LayerNorm(x + attention(x))  (tests/mhsa_formula.py: head),   h2 = LayerNorm(h1 + ffn(h1))  (only with an FFN)
the positional table is added once, before layer 0.

Gates (derived here, not tuned on kernel output), per element |got - ref| <= gate, with u_ = 2^-24 (fp32's unit roundoff; U below)
and absolute values inside every sum so that no cancellation in the reference can shrink a gate:
  hidden      u is a C-term fma chain plus the bias add:   delta_u = (C + 2) U (sum_c |x||w1| + |b1|)
  activation  |err a| <= L delta_u + C_ACT U |a|:  act is L-Lipschitz (L = 1 for ReLU, L = sup |gelu'| = GELU_L for GELU, computed below
              on a grid, about 1.13) and the device evaluation of act itself is good to C_ACT U relative to |a|
  output      |err y| <= sum_d |w2| (L delta_u + C_ACT U |a|) + (D + 2) U (sum_d |a||w2| + |b2|)
  bf16        the operand roundings of x, w1 (2 x 2^-9 relative per product) add 2^-8 sum_c |x||w1| to delta_u, those of a and w2 add
              2^-8 sum_d |a||w2| to the output
  backward    the same construction; the inputs of every backward launch are fed as the reference rounded to fp32, so each product
              carries its own term only: da: (D + 2) U sum_d |dy||w2|;  du: 2^-23 |du| + C_DACT U |da| (Phi + |u| phi) (the
              absolute-value form of gelu': its two terms cancel for u < 0);  dw2 / dw1: (R + 2) U sum_rows |dy||a| / |du||x|;
              db2 / db1: (R + 2) U sum_rows |dy| / |du|;  dx: (D + 2) U sum_d |du||w1|;  bf16 adds 2^-8 of the same sums (not to the
              column sums, which are taken over the fp32 values)
  sed_ffn_act_bwd alone:  a within 2^-23 |a| + C_ACT U |a|,  du within 2^-23 |du| + C_DACT U |da| (Phi + |u| phi)
C_ACT, C_DACT cover the device erfcf / expf and the rounding of their arguments (u / sqrt 2 is rounded once, and erfc's relative
condition number grows like u^2 for u << 0).  No device-math accuracy table ships with the ROCm installation used, so they were
measured once on the MI355X against float64 over the dense grid u in [-10, 10] (step 2^-12, tools/ffn_time.py --cact) and doubled:
the measured worst relative errors were 126.22 U (a, at u = -9.78) and 75.49 U (gelu', relative to Phi + |u| phi, at u = -9.72);
over |u| <= 5 they are 32.9 U and 19.1 U.  ReLU is exact; the constants below are used for both activations.
"""
import numpy as np
from scipy.special import erfc

import mhsa_formula as M

U = 2.0 ** -24
C_ACT = 253.0          # 2 x 126.22, rounded up
C_DACT = 151.0         # 2 x 75.49, rounded up
RELU, GELU = 0, 1
ACT_CODE = {"relu": RELU, "gelu": GELU}


def phi(u):
    return np.exp(-0.5 * u * u) / np.sqrt(2.0 * np.pi)


def Phi(u):
    return 0.5 * erfc(-u / np.sqrt(2.0))          # = 0.5 (1 + erf(u / sqrt 2)) without the cancellation for u << 0


def act_fwd(u, act, dtype=np.float64):
    u = np.asarray(u, dtype=dtype)
    if act == "relu":
        return np.maximum(u, dtype(0))
    if act == "gelu":
        return (dtype(0.5) * u * erfc(-u * dtype(np.sqrt(0.5))).astype(dtype)).astype(dtype)
    if act == "gelu_tanh":      # (a mutant: the tanh approximation)
        return (0.5 * u * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (u + 0.044715 * u ** 3)))).astype(dtype)
    raise ValueError(act)


def act_grad(u, act, dtype=np.float64):
    u = np.asarray(u, dtype=dtype)
    if act == "relu":
        return (u > 0).astype(dtype)
    return (Phi(u) + u * phi(u)).astype(dtype)


_grid = np.linspace(-10.0, 10.0, 200001)
GELU_L = float(np.abs(act_grad(_grid, "gelu")).max())          # sup |gelu'|, attained near u = sqrt 2


def lipschitz(act):
    return 1.0 if act == "relu" else GELU_L


def ffn(x, w1, b1, w2, b2, act, dy=None, dtype=np.float64, mutant=None, bf16_operands=False):
    """The definition (float64) or a plain implementation in `dtype` arithmetic.  bf16_operands: x, w1, a, w2 (backward: dy, du too)
    rounded to bf16 where they are operands of a product.  mutant: a deliberately wrong definition (tests/test_ffn_host.py)."""
    rb = (lambda v: M.round_bf16(v).astype(dtype)) if bf16_operands else (lambda v: v)
    x, w1, b1, w2, b2 = (np.asarray(v, dtype=dtype) for v in (x, w1, b1, w2, b2))
    u = (rb(x) @ rb(w1).T).astype(dtype)
    if mutant != "no_b1":
        u = u + b1
    a = act_fwd(u, "gelu_tanh" if mutant == "gelu_tanh" and act == "gelu" else act, dtype)
    w2f = w2
    if mutant == "swap_w2_chunks":          # hidden chunks [0, 32) and [32, 64) of w2 change places
        w2f = w2.copy()
        w2f[:, 0:32], w2f[:, 32:64] = w2[:, 32:64], w2[:, 0:32]
    y = ((rb(a) @ rb(w2f).T).astype(dtype) + b2).astype(dtype)
    out = dict(u=u, a=a, y=y)
    if dy is None:
        return out
    dy = np.asarray(dy, dtype=dtype)
    da = (rb(dy) @ rb(w2)).astype(dtype)
    du = (da * act_grad(a if mutant == "grad_at_a" else u, act, dtype)).astype(dtype)
    out.update(da=da, du=du, dw2=(rb(dy).T @ rb(a)).astype(dtype), db2=dy.sum(axis=0, dtype=dtype),
               dw1=(rb(du).T @ rb(x)).astype(dtype), db1=du.sum(axis=0, dtype=dtype), dx=(rb(du) @ rb(w1)).astype(dtype))
    return out


def act_bwd_gates(u, da, act):
    u, da = np.asarray(u, dtype=np.float64), np.asarray(da, dtype=np.float64)
    a = act_fwd(u, act)
    gabs = (u > 0).astype(np.float64) if act == "relu" else Phi(u) + np.abs(u) * phi(u)
    return dict(a=(2.0 ** -23 + C_ACT * U) * np.abs(a), du=2.0 ** -23 * np.abs(da * act_grad(u, act)) + C_DACT * U * np.abs(da) * gabs)


def ffn_gates(x, w1, b1, w2, b2, act, dy=None, mode="f32"):
    """-> dict of per-element gates (module docstring) for u, a, y and, with dy, da, du, dw2, db2, dw1, db1, dx"""
    assert mode in ("f32", "bf16")
    x, w1, b1, w2, b2 = (np.asarray(v, dtype=np.float64) for v in (x, w1, b1, w2, b2))
    R, C = x.shape
    D = w1.shape[0]
    pb = 2.0 ** -8 if mode == "bf16" else 0.0
    r = ffn(x, w1, b1, w2, b2, act, dy)
    L = lipschitz(act)
    xw = np.abs(x) @ np.abs(w1).T
    du_ = (C + 2) * U * (xw + np.abs(b1)) + pb * xw
    ea = L * du_ + C_ACT * U * np.abs(r["a"])
    aw = np.abs(r["a"]) @ np.abs(w2).T
    g = dict(u=du_, a=ea, y=ea @ np.abs(w2).T + (D + 2) * U * (aw + np.abs(b2)) + pb * aw)
    if dy is None:
        return g
    dy = np.abs(np.asarray(dy, dtype=np.float64))
    g["da"] = ((D + 2) * U + pb) * (dy @ np.abs(w2))
    g["du"] = act_bwd_gates(r["u"], r["da"], act)["du"]
    adu = np.abs(r["du"])
    g["dw2"] = ((R + 2) * U + pb) * (dy.T @ np.abs(r["a"]))
    g["db2"] = (R + 2) * U * dy.sum(axis=0)
    g["dw1"] = ((R + 2) * U + pb) * (adu.T @ np.abs(x))
    g["db1"] = (R + 2) * U * adu.sum(axis=0)
    g["dx"] = ((D + 2) * U + pb) * (adu @ np.abs(w1))
    return g


def layer_names(l):
    """the module names of layer l in Csa_AvgPooling's state_dict: attn, attn_norm, ffn, ffn_norm (+ _l{l} from layer 1 on)"""
    s = "" if l == 0 else f"_l{l}"
    return "attn" + s, "attn_norm" + s, "ffn" + s, "ffn_norm" + s


def encoder(x, W, B, t, H, layers=1, ffn_width=0, act="relu", pos_encoding=True, dh_out=None, dtype=np.float64, mutant=None):
    """The stack in float64 (or plain `dtype` arithmetic for the FFN and LayerNorm parts).  x (B*t, C) mel-mean rows; W: dict by
    state_dict name (attn.in_proj_weight ... ffn_norm_l1.bias).  dh_out: the gradient of the last layer's output -> also "dx" and
    "d_" + name for every parameter.  mutant: no_ffn_residual, ln_before_add, pe_every_layer."""
    W = {n: np.asarray(v, dtype=np.float64) for n, v in W.items()}
    cur = np.asarray(x, dtype=np.float64)
    saved = []
    for l in range(layers):
        an, nn_, fn, fnn = layer_names(l)
        Wa = {"in_proj_weight": W[an + ".in_proj_weight"], "in_proj_bias": W[an + ".in_proj_bias"], "out_proj.weight": W[an + ".out_proj.weight"],
              "out_proj.bias": W[an + ".out_proj.bias"], "norm.weight": W[nn_ + ".weight"], "norm.bias": W[nn_ + ".bias"]}
        pe = pos_encoding and (l == 0 or mutant == "pe_every_layer")
        hd = M.head(cur, Wa, B, t, H, pos_encoding=pe)
        h1 = hd["h"]
        rec = dict(x=cur, Wa=Wa, pe=pe, h1=h1)
        if ffn_width > 0:
            f = ffn(h1, W[fn + ".linear1.weight"], W[fn + ".linear1.bias"], W[fn + ".linear2.weight"], W[fn + ".linear2.bias"], act, dtype=dtype)
            if mutant == "ln_before_add":
                zero = np.zeros_like(h1)
                cur = M.add_layernorm(h1, zero, W[fnn + ".weight"], W[fnn + ".bias"])["y"] + f["y"]
            else:
                res = np.zeros_like(h1) if mutant == "no_ffn_residual" else h1
                cur = M.add_layernorm(res.astype(dtype), f["y"], W[fnn + ".weight"], W[fnn + ".bias"], dtype=dtype)["y"].astype(np.float64)
            rec["f"] = f["y"]
        else:
            cur = h1
        saved.append(rec)
    out = dict(h=cur)
    if dh_out is None:
        return out
    assert mutant is None and dtype == np.float64
    g = np.asarray(dh_out, dtype=np.float64)
    for l in reversed(range(layers)):
        an, nn_, fn, fnn = layer_names(l)
        rec = saved[l]
        if ffn_width > 0:
            lb = M.add_layernorm(rec["h1"], rec["f"], W[fnn + ".weight"], W[fnn + ".bias"], g)
            out["d_" + fnn + ".weight"], out["d_" + fnn + ".bias"] = lb["dgamma"], lb["dbeta"]
            fb = ffn(rec["h1"], W[fn + ".linear1.weight"], W[fn + ".linear1.bias"], W[fn + ".linear2.weight"], W[fn + ".linear2.bias"], act, lb["dres"])
            for k, v in (("linear1.weight", "dw1"), ("linear1.bias", "db1"), ("linear2.weight", "dw2"), ("linear2.bias", "db2")):
                out[f"d_{fn}.{k}"] = fb[v]
            g = fb["dx"] + lb["dres"]
        hb = M.head(rec["x"], rec["Wa"], B, t, H, pos_encoding=rec["pe"], dh_out=g)
        for k in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"):
            out[f"d_{an}.{k}"] = hb["d_" + k]
        out["d_" + nn_ + ".weight"], out["d_" + nn_ + ".bias"] = hb["d_norm.weight"], hb["d_norm.bias"]
        g = hb["dx"]
    out["dx"] = g
    return out


def stack_gate(h, layers, C, D, t):
    """The gate of a whole stack's output in fp32 arithmetic.  A LayerNorm output is O(1) per element (unit variance times gamma), each
    of a layer's sums has at most max(C, D, t) terms, and a layer is a chain of eight such stages (three products and the softmax of the
    attention, two products of the FFN, two LayerNorms), each of whose errors the following LayerNorm passes on with a factor of
    order one: 8 layers (max(C, D, t) + 8) U (1 + |h|)."""
    return 8.0 * layers * (max(C, D, t) + 8) * U * (1.0 + np.abs(np.asarray(h, dtype=np.float64)))


def exact_case(rng, R, C, D):
    """The exact-integer family: x in {-1, 0, 1}, w1 in {-1, 0, 1} with at most 8 non-zeros per hidden unit, b1 in {-2 .. 2}, w2 in
    {-1, 0, 1}, b2 in {-3 .. 3}: every hidden value is an integer of magnitude <= 8 + 2 (bf16 holds integers up to 256 exactly), every
    sum stays far below 2^24, so float64, fp32 and bf16-operand arithmetic give the same values in any order."""
    x = rng.integers(-1, 2, (R, C)).astype(np.float32)
    w1 = np.zeros((D, C), dtype=np.float32)
    for d in range(D):
        idx = rng.choice(C, size=8, replace=False)
        w1[d, idx] = rng.integers(-1, 2, 8)
    b1 = rng.integers(-2, 3, D).astype(np.float32)
    w2 = rng.integers(-1, 2, (C, D)).astype(np.float32)
    b2 = rng.integers(-3, 4, C).astype(np.float32)
    return x, w1, b1, w2, b2


check = M.check
round_bf16 = M.round_bf16
