"""The dropout of the self-attention head (csrc/philox.h and the _drop kernels of csrc/sed_mhsa.hip / sed_layernorm.hip / sed_ffn.hip) as plain numpy: the
counter-based generator, the two mask layouts, and the float64 definitions of the three masked operations with their gates.  The
kernels are tested against this (tests/test_gpu_dropout.py, tests/test_gpu_sa_dropout.py); this file is itself checked against
torch autograd and the undropped formula modules on the host (tests/test_dropout_host.py).

Masks.  Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds).
    state  (seed_lo, seed_hi, step, 0), four uint32;   key (seed_lo, seed_hi ^ stream),  stream = 8 layer + site
    sites  0 attention probabilities, 1 attention output before its residual add, 2 convolution module output before its residual
           add, 3 FFN hidden activation, 4 FFN output before its residual add
    rows [R][N], element (r, c):           counter (c >> 2, r mod 2^32, r >> 32, step), output word c & 3
    attention, clip b, head g, (i, j):     counter (j >> 2, i, b H + g, step),          output word j & 3
    keep iff word >= thr,  thr = min(2^32 - 1, floor(p 2^32 + 1/2)) in double from the FLOAT p;  kept values are multiplied in fp32
    by s = (float)(1 / (1 - (double)p)).  Below m is the 0 / 1 keep mask and ms = m s.

Definitions (float64).
    attention   s_ij, lse_i, p_ij as tests/mhsa_formula.py (all keys, no renormalisation);  p~_ij = ms_ij p_ij,  ctx_ic = sum_j p~_ij v_jc
                D_i = sum_c dctx_ic ctx_ic (the dropped ctx),  dv_jc = sum_i p~_ij dctx_ic,  dp_ij = ms_ij sum_c dctx_ic v_jc,
                ds_ij = p_ij (dp_ij - D_i),  dq, dk from ds as undropped
    residual    y = LayerNorm(x + ms a);  dres (the gradient of x) as undropped with xhat of the dropped sum,  da = ms dres
    FFN         u = x w1^T + b1 (undropped),  a = ms act(u),  y = a w2^T + b2;  da = dy w2,  du = da ms act'(u),  dw2 = dy^T a

Gates (derived here, not tuned on kernel output; U = 2^-24).  They are the gates of mhsa_formula / ffn_formula with the dropped
quantity in place of the undropped one and ONE extra rounding U for each multiply by ms:
  attention  The weights' relative error rho_i is unchanged (the mask touches neither the scores nor the normalising sum).
             ctx: (rho_i + (t + 3) U + pb) sum_j p~_ij |v_jc| -- p~ in place of p, (t + 2) -> (t + 3) for the scale multiply, and the
             bf16 operand term pb = 2^-8 over the scaled operands p~.  lse: unchanged.
             backward: Abar_ij = ms_ij sum_c |dctx||v| + sum_c |dctx||ctx| (dp carries ms), ES_ij = p_ij Abar_ij (rho'_i + (dh + 6) U + pb)
             (one more rounding: dp times ms);  dv: sum_i p~_ij |dctx_ic| (rho'_i + (t + 3) U + pb);  dq, dk as undropped from ES.
  residual   mhsa_formula's LayerNorm gates evaluated at a' = ms a with (C + 9) U in place of (C + 8) U (the scale multiply is one
             more rounding in z; the kernel's fma makes it none);  da: ms gate(dres) + U |da|;  dgamma, dbeta unchanged in form.
  FFN        delta_u unchanged;  |err a| <= ms (L delta_u + C_ACT U |act(u)|) + U |a|;  y: that through |w2| plus
             (D + 2) U (sum_d |a||w2| + |b2|) plus pb sum_d |a||w2| with the dropped a.
             sed_ffn_act_bwd_drop alone: a within ms (2^-23 + C_ACT U) |act(u)| + U |a|,  du within ms gate_du(undropped) + U |du|.
"""
import numpy as np

import ffn_formula as F
import mhsa_formula as M

U = 2.0 ** -24
SITE_ATTN, SITE_ATTN_OUT, SITE_CONV_OUT, SITE_FFN_HIDDEN, SITE_FFN_OUT = 0, 1, 2, 3, 4
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def stream_id(layer, site):
    return 8 * layer + site


def philox4x32_10(counter, key):
    """counter: four broadcastable arrays (or ints), key: two; -> four uint32 arrays of the broadcast shape"""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & MASK32 for v in key]
    c = list(np.broadcast_arrays(*c))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK32]
        k = [(k[0] + np.uint64(W0)) & MASK32, (k[1] + np.uint64(W1)) & MASK32]
    return [v.astype(np.uint32) for v in c]


def thr_scale(p):
    """-> (thr, s): the threshold as a Python int and the fp32 scale, both from the float32 value of p"""
    pf = float(np.float32(p))
    assert 0.0 <= pf < 1.0
    thr = min(2 ** 32 - 1, int(np.floor(pf * 4294967296.0 + 0.5)))
    return thr, np.float32(1.0 / (1.0 - pf))


def _state(state):
    s = [int(v) & 0xFFFFFFFF for v in np.asarray(state).reshape(-1)[:4]]
    return s[0], s[1], s[2]


def words_rows(state, stream, R, N, row0=0):
    """the uint32 word of every element of a row tensor: (R, N)"""
    lo, hi, step = _state(state)
    r = (np.arange(R, dtype=np.uint64) + np.uint64(row0))[:, None]
    q = np.arange((N + 3) // 4, dtype=np.uint64)[None, :]
    w = philox4x32_10((q, r & MASK32, r >> np.uint64(32), step), (lo, hi ^ stream))
    return np.stack(w, axis=-1).reshape(R, -1)[:, :N]


def words_attn(state, stream, B, H, t):
    """(B, H, t, t): [b][g][i][j]"""
    lo, hi, step = _state(state)
    bh = np.arange(B * H, dtype=np.uint64)[:, None, None]
    i = np.arange(t, dtype=np.uint64)[None, :, None]
    q = np.arange((t + 3) // 4, dtype=np.uint64)[None, None, :]
    w = philox4x32_10((q, i, bh, step), (lo, hi ^ stream))
    return np.stack(w, axis=-1).reshape(B * H, t, -1)[:, :, :t].reshape(B, H, t, t)


def keep_rows(state, stream, R, N, p):
    """the 0 / 1 keep mask of a row tensor, uint8 (R, N)"""
    return (words_rows(state, stream, R, N).astype(np.uint64) >= thr_scale(p)[0]).astype(np.uint8)


def keep_attn(state, stream, B, H, t, p):
    """uint8 (B, H, t, t): [b][g][query][key]"""
    return (words_attn(state, stream, B, H, t).astype(np.uint64) >= thr_scale(p)[0]).astype(np.uint8)


# ---- attention ------------------------------------------------------------------------------------------------------------------
def core(q, k, v, keep, s, dctx=None, dtype=np.float64, mutant=None, bf16_operands=False, lse=None, ctx=None, keep_bwd=None):
    """The masked core: the definition (float64) or a plain implementation in `dtype` arithmetic.  keep (B, H, t, t) 0 / 1, s the scale.
    lse, ctx: teacher-forced backward, as mhsa_formula.core.  keep_bwd: the mask the backward uses (a mutant's; default keep).
    mutant: no_rescale, renormalise, transposed_mask, D_undropped."""
    q, k, v = (np.asarray(a, dtype=dtype) for a in (q, k, v))
    B, t, H, dh = q.shape
    keep = np.asarray(keep)
    if mutant == "transposed_mask":
        keep = keep.transpose(0, 1, 3, 2)
    ms = (keep.astype(dtype) * (dtype(1) if mutant == "no_rescale" else dtype(s))).astype(dtype)
    scale = dtype(1.0 / np.sqrt(dh))
    sc = (np.einsum("bihc,bjhc->bhij", q, k).astype(dtype) * scale).astype(dtype)
    m = sc.max(axis=3, keepdims=True)
    e = np.exp(sc - m).astype(dtype)
    l = e.sum(axis=3, keepdims=True, dtype=dtype)
    p = (e / l).astype(dtype)
    lse_own = (m + np.log(l)).astype(dtype)[..., 0]
    pt = (p * ms).astype(dtype)
    if mutant == "renormalise":
        pt = (pt / np.maximum(pt.sum(axis=3, keepdims=True), dtype(1e-30))).astype(dtype)
    rb = (lambda a: M.round_bf16(a).astype(dtype)) if bf16_operands else (lambda a: a)
    out = dict(ctx=np.einsum("bhij,bjhc->bihc", rb(pt), v).astype(dtype), lse=lse_own, p=p, pt=pt, s=sc)
    if dctx is None:
        return out
    dctx = np.asarray(dctx, dtype=dtype)
    if lse is not None:
        p = (p * np.exp(lse_own - np.asarray(lse, dtype=dtype))[..., None].astype(dtype)).astype(dtype)
    msb = ms if keep_bwd is None else (np.asarray(keep_bwd).astype(dtype) * dtype(s)).astype(dtype)
    ptb = (p * msb).astype(dtype)
    out["p_bwd"], out["pt_bwd"], out["ms_bwd"] = p, ptb, msb
    if mutant == "D_undropped":
        cD = np.einsum("bhij,bjhc->bihc", p, v).astype(dtype)
    else:
        cD = out["ctx"] if ctx is None else np.asarray(ctx, dtype=dtype)
    D = np.einsum("bihc,bihc->bhi", dctx, cD).astype(dtype)[..., None]
    dp = (np.einsum("bihc,bjhc->bhij", dctx, v).astype(dtype) * msb).astype(dtype)
    ds = (p * (dp - D)).astype(dtype)
    out["dv"] = np.einsum("bhij,bihc->bjhc", rb(ptb), dctx).astype(dtype)
    out["dq"] = (scale * np.einsum("bhij,bjhc->bihc", rb(ds), k)).astype(dtype)
    out["dk"] = (scale * np.einsum("bhij,bihc->bjhc", rb(ds), q)).astype(dtype)
    return out


def core_gates(q, k, v, keep, s, dctx, mode="f32", lse=None, ctx=None):
    """per-element gates for ctx, lse, dq, dk, dv (module docstring)"""
    assert mode in ("f32", "bf16")
    q, k, v, dctx = (np.asarray(a, dtype=np.float64) for a in (q, k, v, dctx))
    B, t, H, dh = q.shape
    scale = 1.0 / np.sqrt(dh)
    r = core(q, k, v, keep, s, dctx, lse=lse, ctx=ctx)
    aq, ak, av, ad = np.abs(q), np.abs(k), np.abs(v), np.abs(dctx)
    delta = (dh + 2) * U * scale * np.einsum("bihc,bjhc->bhij", aq, ak).max(axis=3)
    S = np.abs(r["s"]).max(axis=3)
    rho = 2.0 * delta + M.c1(t) * U + 4.0 * U * S
    pb = 2.0 ** -8 if mode == "bf16" else 0.0
    g = {}
    g["ctx"] = (rho + (t + 3) * U + pb).transpose(0, 2, 1)[..., None] * np.einsum("bhij,bjhc->bihc", r["pt"], av)
    g["lse"] = rho + 2.0 ** -23 * np.abs(r["lse"])
    lse = r["lse"] if lse is None else np.asarray(lse, dtype=np.float64)
    ctx = r["ctx"] if ctx is None else np.asarray(ctx, dtype=np.float64)
    p, ptb, msb = r["p_bwd"], r["pt_bwd"], r["ms_bwd"]
    rho_b = delta + U * np.abs(lse) + 4.0 * U * S + 8.0 * U
    Abar = msb * np.einsum("bihc,bjhc->bhij", ad, av) + np.einsum("bihc,bihc->bhi", ad, np.abs(ctx))[..., None]
    pA = p * Abar
    ES = pA * (rho_b[..., None] + (dh + 6) * U + pb)
    g["dv"] = np.einsum("bhij,bihc->bjhc", ptb * (rho_b[..., None] + (t + 3) * U + pb), ad)
    tot = ES + (t + 3) * U * pA
    g["dq"] = scale * np.einsum("bhij,bjhc->bihc", tot, ak)
    g["dk"] = scale * np.einsum("bhij,bihc->bjhc", tot, aq)
    return g


# ---- residual add + LayerNorm -----------------------------------------------------------------------------------------------------
def add_layernorm(x, a, keep, s, gamma, beta, dy=None, eps=M.EPS, dtype=np.float64, mutant=None, stats=None, keep_bwd=None):
    """y = LayerNorm(x + ms a) -> mhsa_formula.add_layernorm's dict plus, with dy, da = ms dres.  mutant: no_rescale, da_unmasked."""
    sc = dtype(1) if mutant == "no_rescale" else dtype(s)
    ms = (np.asarray(keep).astype(dtype) * sc).astype(dtype)
    a = np.asarray(a, dtype=dtype)
    out = M.add_layernorm(x, (a * ms).astype(dtype), gamma, beta, eps=eps, dtype=dtype)
    if dy is None:
        return out
    msb = ms if keep_bwd is None else (np.asarray(keep_bwd).astype(dtype) * sc).astype(dtype)
    out = M.add_layernorm(x, (a * msb).astype(dtype), gamma, beta, dy, eps=eps, dtype=dtype, stats=stats)
    out["da"] = out["dres"] if mutant == "da_unmasked" else (out["dres"] * msb).astype(dtype)
    return out


def add_layernorm_gates(x, a, keep, s, gamma, beta, dy, eps=M.EPS, stats=None):
    ms = np.asarray(keep).astype(np.float64) * float(s)
    C = np.shape(x)[1]
    g = M.add_layernorm_gates(x, np.asarray(a, dtype=np.float64) * ms, gamma, beta, dy, eps, stats=stats)
    f = (C + 9.0) / (C + 8.0)                      # one more rounding in z
    g = dict(y=g["y"] * f, dres=g["dres"] * f, dgamma=g["dgamma"], dbeta=g["dbeta"])
    r = add_layernorm(x, a, keep, s, gamma, beta, dy, eps, stats=stats)
    g["da"] = ms * g["dres"] + U * np.abs(r["da"])
    return g


# ---- FFN ------------------------------------------------------------------------------------------------------------------------------
def ffn(x, w1, b1, w2, b2, act, keep, s, dy=None, dtype=np.float64, mutant=None, bf16_operands=False, keep_bwd=None):
    """a = ms act(u).  keep (R, D).  mutant: no_rescale, mask_on_u (the mask applied to u instead of act(u))."""
    rb = (lambda v: M.round_bf16(v).astype(dtype)) if bf16_operands else (lambda v: v)
    x, w1, b1, w2, b2 = (np.asarray(v, dtype=dtype) for v in (x, w1, b1, w2, b2))
    ms = (np.asarray(keep).astype(dtype) * (dtype(1) if mutant == "no_rescale" else dtype(s))).astype(dtype)
    u = ((rb(x) @ rb(w1).T).astype(dtype) + b1).astype(dtype)
    if mutant == "mask_on_u":
        a = F.act_fwd((u * ms).astype(dtype), act, dtype)
    else:
        a = (F.act_fwd(u, act, dtype) * ms).astype(dtype)
    y = ((rb(a) @ rb(w2).T).astype(dtype) + b2).astype(dtype)
    out = dict(u=u, a=a, y=y)
    if dy is None:
        return out
    dy = np.asarray(dy, dtype=dtype)
    msb = ms if keep_bwd is None else (np.asarray(keep_bwd).astype(dtype) * dtype(s)).astype(dtype)
    ab = a if keep_bwd is None else (F.act_fwd(u, act, dtype) * msb).astype(dtype)
    da = (rb(dy) @ rb(w2)).astype(dtype)
    if mutant == "mask_on_u":
        du = (da * msb * F.act_grad((u * msb).astype(dtype), act, dtype)).astype(dtype)
    else:
        du = (da * msb * F.act_grad(u, act, dtype)).astype(dtype)
    out.update(da=da, du=du, a_bwd=ab, dw2=(rb(dy).T @ rb(ab)).astype(dtype), db2=dy.sum(axis=0, dtype=dtype),
               dw1=(rb(du).T @ rb(x)).astype(dtype), db1=du.sum(axis=0, dtype=dtype), dx=(rb(du) @ rb(w1)).astype(dtype))
    return out


def act_bwd_gates(u, da, act, keep, s):
    ms = np.asarray(keep).astype(np.float64) * float(s)
    g = F.act_bwd_gates(u, da, act)
    a = F.act_fwd(np.asarray(u, dtype=np.float64), act) * ms
    du = np.asarray(da, dtype=np.float64) * ms * F.act_grad(np.asarray(u, dtype=np.float64), act)
    return dict(a=ms * g["a"] + U * np.abs(a), du=ms * g["du"] + U * np.abs(du))


def ffn_gates(x, w1, b1, w2, b2, act, keep, s, mode="f32"):
    """gates of the fused forward: u, a, y"""
    assert mode in ("f32", "bf16")
    x, w1, b1, w2, b2 = (np.asarray(v, dtype=np.float64) for v in (x, w1, b1, w2, b2))
    R, C = x.shape
    D = w1.shape[0]
    ms = np.asarray(keep).astype(np.float64) * float(s)
    pb = 2.0 ** -8 if mode == "bf16" else 0.0
    r = ffn(x, w1, b1, w2, b2, act, keep, s)
    xw = np.abs(x) @ np.abs(w1).T
    du_ = (C + 2) * U * (xw + np.abs(b1)) + pb * xw
    aa = np.abs(r["a"])
    ea = ms * (F.lipschitz(act) * du_ + F.C_ACT * U * np.abs(F.act_fwd(r["u"], act))) + U * aa
    aw = aa @ np.abs(w2).T
    return dict(u=du_, a=ea, y=ea @ np.abs(w2).T + (D + 2) * U * (aw + np.abs(b2)) + pb * aw)


# ---- the masked encoder stack ---------------------------------------------------------------------------------------------------------
def head(x, Wa, B, t, H, state, p, layer, pos_encoding=True, dh_out=None):
    """mhsa_formula.head with the attention probabilities (site 0) and the attention output before its residual add (site 1) dropped"""
    x = np.asarray(x, dtype=np.float64)
    R, C = x.shape
    dh = C // H
    s = float(thr_scale(p)[1])
    ka = keep_attn(state, stream_id(layer, SITE_ATTN), B, H, t, p)
    ko = keep_rows(state, stream_id(layer, SITE_ATTN_OUT), R, C, p)
    xp = x + np.tile(M.positional_table(t, C), (B, 1)) if pos_encoding else x
    qkv = xp @ Wa["in_proj_weight"].T + Wa["in_proj_bias"]
    q, k, v = M.split_qkv(qkv, B, t, H, dh)
    c = core(q, k, v, ka, s)
    ctx = c["ctx"].reshape(R, C)
    a = ctx @ Wa["out_proj.weight"].T + Wa["out_proj.bias"]
    out = dict(h=add_layernorm(xp, a, ko, s, Wa["norm.weight"], Wa["norm.bias"])["y"])
    if dh_out is None:
        return out
    lb = add_layernorm(xp, a, ko, s, Wa["norm.weight"], Wa["norm.bias"], dh_out)
    dres, da = lb["dres"], lb["da"]
    out["d_norm.weight"], out["d_norm.bias"] = lb["dgamma"], lb["dbeta"]
    out["d_out_proj.weight"], out["d_out_proj.bias"] = da.T @ ctx, da.sum(axis=0)
    cb = core(q, k, v, ka, s, (da @ Wa["out_proj.weight"]).reshape(B, t, H, dh))
    dqkv = M.join_qkv(cb["dq"], cb["dk"], cb["dv"])
    out["d_in_proj_weight"], out["d_in_proj_bias"] = dqkv.T @ xp, dqkv.sum(axis=0)
    out["dx"] = dqkv @ Wa["in_proj_weight"] + dres
    return out


def encoder(x, W, B, t, H, state, p, layers=1, ffn_width=0, act="relu", pos_encoding=True, conv=False, dh_out=None):
    """The post-LN stack in float64 with torch.nn.TransformerEncoderLayer(dropout=p)'s placement (and the convolution module's output
    dropped before its residual add), in training mode, the masks of `state` = (seed_lo, seed_hi, step, 0).  x (B*t, C) mel-mean rows;
    W by state_dict name.  -> h, with conv the running statistics, and with dh_out: dx and "d_" + name per parameter."""
    import convmod_formula as V
    W = {n: np.asarray(a, dtype=np.float64) for n, a in W.items()}
    cur = np.asarray(x, dtype=np.float64)
    R, C = cur.shape
    s = float(thr_scale(p)[1])
    saved, out = [], {}
    for l in range(layers):
        an, nn_, fn, fnn = F.layer_names(l)
        Wa = {"in_proj_weight": W[an + ".in_proj_weight"], "in_proj_bias": W[an + ".in_proj_bias"], "out_proj.weight": W[an + ".out_proj.weight"],
              "out_proj.bias": W[an + ".out_proj.bias"], "norm.weight": W[nn_ + ".weight"], "norm.bias": W[nn_ + ".bias"]}
        pe = pos_encoding and l == 0
        rec = dict(x=cur, Wa=Wa, pe=pe)
        cur = head(cur, Wa, B, t, H, state, p, l, pos_encoding=pe)["h"]
        rec["h1"] = cur
        if conv:
            cm, cn = V.conv_names(l)
            Wc = V.conv_state(W, l)
            m = V.module(cur, Wc, B, t, True)
            out[cm + ".bn.running_mean"], out[cm + ".bn.running_var"] = m["running_mean"], m["running_var"]
            kc = keep_rows(state, stream_id(l, SITE_CONV_OUT), R, C, p)
            rec.update(Wc=Wc, o=m["o"], kc=kc)
            cur = add_layernorm(cur, m["o"], kc, s, Wc["conv_norm.weight"], Wc["conv_norm.bias"])["y"]
        rec["hc"] = cur
        if ffn_width > 0:
            kh = keep_rows(state, stream_id(l, SITE_FFN_HIDDEN), R, ffn_width, p)
            kf = keep_rows(state, stream_id(l, SITE_FFN_OUT), R, C, p)
            f = ffn(cur, W[fn + ".linear1.weight"], W[fn + ".linear1.bias"], W[fn + ".linear2.weight"], W[fn + ".linear2.bias"], act, kh, s)
            rec.update(f=f["y"], kh=kh, kf=kf)
            cur = add_layernorm(cur, f["y"], kf, s, W[fnn + ".weight"], W[fnn + ".bias"])["y"]
        saved.append(rec)
    out["h"] = cur
    if dh_out is None:
        return out
    g = np.asarray(dh_out, dtype=np.float64)
    for l in reversed(range(layers)):
        an, nn_, fn, fnn = F.layer_names(l)
        rec = saved[l]
        if ffn_width > 0:
            lb = add_layernorm(rec["hc"], rec["f"], rec["kf"], s, W[fnn + ".weight"], W[fnn + ".bias"], g)
            out["d_" + fnn + ".weight"], out["d_" + fnn + ".bias"] = lb["dgamma"], lb["dbeta"]
            fb = ffn(rec["hc"], W[fn + ".linear1.weight"], W[fn + ".linear1.bias"], W[fn + ".linear2.weight"], W[fn + ".linear2.bias"], act,
                     rec["kh"], s, lb["da"])
            for k, v in (("linear1.weight", "dw1"), ("linear1.bias", "db1"), ("linear2.weight", "dw2"), ("linear2.bias", "db2")):
                out[f"d_{fn}.{k}"] = fb[v]
            g = fb["dx"] + lb["dres"]
        if conv:
            cm, cn = V.conv_names(l)
            Wc = rec["Wc"]
            lb = add_layernorm(rec["h1"], rec["o"], rec["kc"], s, Wc["conv_norm.weight"], Wc["conv_norm.bias"], g)
            out["d_" + cn + ".weight"], out["d_" + cn + ".bias"] = lb["dgamma"], lb["dbeta"]
            mb = V.module(rec["h1"], Wc, B, t, True, do=lb["da"])
            for n, a in mb.items():
                if n.startswith("d_"):
                    out["d_" + cm + "." + n[2:]] = a
            g = mb["dh"] + lb["dres"]
        hb = head(rec["x"], rec["Wa"], B, t, H, state, p, l, pos_encoding=rec["pe"], dh_out=g)
        for k in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"):
            out[f"d_{an}.{k}"] = hb["d_" + k]
        out["d_" + nn_ + ".weight"], out["d_" + nn_ + ".bias"] = hb["d_norm.weight"], hb["d_norm.bias"]
        g = hb["dx"]
    out["dx"] = g
    return out


check = M.check
round_bf16 = M.round_bf16
