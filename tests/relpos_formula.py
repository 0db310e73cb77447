"""The learned relative-position bias of the self-attention head (the REL instantiations of csrc/sed_mhsa.hip behind sed_mhsa_fwd_rel /
sed_mhsa_bwd_rel, with sed_relpos_expand / sed_relpos_fold) as plain numpy: the two bucket maps, the float64 definition of the biased
windowed core over explicit t x t matrices, forward and backward, with an optional dropout keep mask and teacher-forced lse / ctx, the
per-distance gradient drel, the folded dw, the encoder stack and the gates.  The kernels are tested against this
(tests/test_gpu_relpos.py); this file is itself checked against torch.nn.MultiheadAttention(attn_mask=float mask) and
torch.nn.TransformerEncoderLayer(src_mask=) in float64 on the host (tests/test_relpos_host.py).

Buckets.  d = j - i (key minus query).  The function here is the definition:
    clipped, L >= 1:        bucket(d) = clamp(d, -L, L) + L                                           2L + 1 buckets
    log, (nb, maxd):        n = nb / 2, a = |d|, m = n // 2 (T5's max_exact; nb even >= 4, maxd > nb / 4)
                            bucket(d) = (n if d > 0 else 0) + (a                                              if a < m
                                                              min(n - 1, m + floor(ln(a/m) / ln(maxd/m) (n - m)))  otherwise)
                            in float64 as written (T5's _relative_position_bucket, bidirectional)
bucket_map(cfg, t)[d + t - 1] is the int table over d in [-(t-1), t-1] that the host builds.

Definitions (float64), in window_formula's symbols, rel[g][d + t - 1] = w[g][bucket(d)]:
    s_ij = scale q_i . k_j + rel[g][(j - i) + t - 1]                  (the bias is added AFTER the scaling)
    lse, p, p~, ctx, D, dv, dp, ds, dq, dk as in window_formula with this s   (ds is the gradient of the biased score)
    drel[g][d + t - 1] = sum_b sum_{(i, j) in the window, j - i = d} ds_ij      (no scale)
    dw[g][n]           = sum_{d: bucket(d) = n} drel[g][d + t - 1]              (0 for a bucket no distance of the clip maps to)
A zero table is window_formula.core bit for bit (x + 0.0 = x).

Gates (derived from window_formula's, not tuned on kernel output; U = 2^-24):
  score     the biased score gains one rounding of the add on top of the product's error: delta_i of window_formula becomes
            delta_i = max_{j in W_i} ((dh + 2) U scale sum_c |q_ic||k_jc| + U (|scale q_i . k_j| + |bias_ij|)), and S_i is the largest
            |biased score| of the row.  With these two every line of window_formula's gates (ctx, lse, dv, dq, dk, ES) goes through
            unchanged, evaluated on the biased p.
  drel      a distance's sum has n_d contributing cells over all clips (in-window, inside the clip): the kernel adds them in fp32 inside
            a wave, the per-wave partials in fp64, and rounds once -- at most (n_d + 2) U sum |ds| -- and each ds carries
            window_formula's ES_ij:  gate = (n_d + 2) U sum |ds_ij| + sum ES_ij over the distance's cells.
  dw        the same over the bucket's cells: (n_b + 2) U sum |ds_ij| + sum ES_ij, n_b the bucket's cell count.
  raw dctx  (bf16, raw_dctx=True)  window_formula's terms for a dctx the kernel rounds as an operand, on the biased p; through ES they
            reach drel and dw as every other error of ds does.
"""
import numpy as np

import convmod_formula as V
import dropout_formula as D
import ffn_formula as F
import mhsa_formula as M
import window_formula as W

U = 2.0 ** -24
MAX_BUCKETS = 4096


def check_config(cfg):
    """an int L >= 1 -> ("clip", L); a pair (nb, maxd) -> ("log", nb, maxd); ValueError otherwise"""
    integer = lambda x: isinstance(x, (int, np.integer)) and not isinstance(x, bool)
    if isinstance(cfg, (tuple, list)):
        if len(cfg) != 2 or not integer(cfg[0]) or not integer(cfg[1]):
            raise ValueError(f"a pair of integers (num_buckets, max_distance) is expected, got {cfg!r}")
        nb, maxd = int(cfg[0]), int(cfg[1])
        if nb < 4 or nb % 2 or 4 * maxd <= nb or nb > MAX_BUCKETS:
            raise ValueError(f"num_buckets even in [4, {MAX_BUCKETS}] and max_distance > num_buckets / 4 are expected, got {cfg!r}")
        return "log", nb, maxd
    if not integer(cfg) or cfg < 1 or 2 * cfg + 1 > MAX_BUCKETS:
        raise ValueError(f"an integer L in [1, {(MAX_BUCKETS - 1) // 2}] is expected, got {cfg!r}")
    return "clip", int(cfg)


def num_buckets(cfg):
    c = check_config(cfg)
    return 2 * c[1] + 1 if c[0] == "clip" else c[1]


def bucket(cfg, d):
    """the bucket of ONE distance d = j - i (python ints and math: the definition)"""
    import math
    c = check_config(cfg)
    d = int(d)
    if c[0] == "clip":
        return max(-c[1], min(c[1], d)) + c[1]
    nb, maxd = c[1], c[2]
    n = nb // 2
    m = n // 2
    a = abs(d)
    off = n if d > 0 else 0
    if a < m:
        return off + a
    return off + min(n - 1, m + int(math.floor(math.log(a / m) / math.log(maxd / m) * (n - m))))


def bucket_map(cfg, t):
    """int32 (2t - 1,): bucket(d) at index d + t - 1"""
    return np.array([bucket(cfg, d) for d in range(-(t - 1), t)], dtype=np.int32)


def expand(w, cfg, t):
    """rel (H, 2t - 1) = w[:, bucket_map]"""
    return np.asarray(w)[:, bucket_map(cfg, t)]


def dist_index(t):
    """(t, t) [query][key]: (j - i) + t - 1"""
    i = np.arange(t)
    return (i[None, :] - i[:, None]) + t - 1


def bias_matrix(rel, t):
    """(H, t, t): rel[g][(j - i) + t - 1]"""
    return np.asarray(rel)[:, dist_index(t)]


def _bias_for(rel, t, mutant):
    rel = np.asarray(rel)
    idx = dist_index(t)
    if mutant == "i_minus_j":
        idx = idx.T
    elif mutant == "diag_off_by_one":
        idx = np.minimum(idx + 1, 2 * t - 2)
    elif mutant == "next_head":
        rel = np.roll(rel, -1, axis=0)
    return rel[:, idx]


def core(q, k, v, rel, left, right, dctx=None, keep=None, s=1.0, dtype=np.float64, mutant=None, bf16_operands=False, lse=None, ctx=None,
         cfg=None):
    """The biased windowed core: the definition (float64) or a plain implementation in `dtype` arithmetic.  rel (H, 2t - 1).  keep, s, lse,
    ctx as window_formula.core.  cfg: also fold drel into dw (H, num_buckets).  mutant (tests/test_relpos_host.py): i_minus_j,
    diag_off_by_one, bias_before_scale, dw_scaled, next_head, dw_unclamped_only, dw_out_of_window."""
    q, k, v = (np.asarray(a, dtype=dtype) for a in (q, k, v))
    B, t, H, dh = q.shape
    w = W.in_window(t, left, right)[None, None]
    bias = _bias_for(np.asarray(rel, dtype=dtype), t, mutant)[None].astype(dtype)
    ms = np.ones((1, 1, t, t), dtype=dtype) if keep is None else (np.asarray(keep).astype(dtype) * dtype(s)).astype(dtype)
    scale = dtype(1.0 / np.sqrt(dh))
    raw = np.einsum("bihc,bjhc->bhij", q, k).astype(dtype)
    if mutant == "bias_before_scale":
        sc = ((raw + bias).astype(dtype) * scale).astype(dtype)
    else:
        sc = ((raw * scale).astype(dtype) + bias).astype(dtype)
    sw = np.where(w, sc, dtype(-np.inf))
    m = sw.max(axis=3, keepdims=True)
    e = np.exp(sw - m).astype(dtype)
    l = e.sum(axis=3, keepdims=True, dtype=dtype)
    p = np.where(w, e / l, dtype(0)).astype(dtype)
    lse_own = (m + np.log(l)).astype(dtype)[..., 0]
    pt = (p * ms).astype(dtype)
    rb = (lambda a: M.round_bf16(a).astype(dtype)) if bf16_operands else (lambda a: a)
    out = dict(ctx=np.einsum("bhij,bjhc->bihc", rb(pt), v).astype(dtype), lse=lse_own, p=p, pt=pt, s=sc, w=w[0, 0],
               s_raw=(raw * scale).astype(dtype), bias=bias[0])
    if dctx is None:
        return out
    dctx = np.asarray(dctx, dtype=dtype)
    if lse is not None:
        p = (p * np.exp(lse_own - np.asarray(lse, dtype=dtype))[..., None].astype(dtype)).astype(dtype)
    ptb = (p * ms).astype(dtype)
    out["p_bwd"], out["pt_bwd"] = p, ptb
    cD = out["ctx"] if ctx is None else np.asarray(ctx, dtype=dtype)
    Dr = np.einsum("bihc,bihc->bhi", dctx, cD).astype(dtype)[..., None]
    dp = (np.einsum("bihc,bjhc->bhij", dctx, v).astype(dtype) * ms).astype(dtype)
    ds = (p * (dp - Dr)).astype(dtype)
    out["ds"] = ds
    out["dv"] = np.einsum("bhij,bihc->bjhc", rb(ptb), dctx).astype(dtype)
    out["dq"] = (scale * np.einsum("bhij,bjhc->bihc", rb(ds), k)).astype(dtype)
    out["dk"] = (scale * np.einsum("bhij,bihc->bjhc", rb(ds), q)).astype(dtype)
    dsd = ds
    if mutant == "dw_out_of_window":                 # ds of every cell of the clip, the softmax over the window's lse
        dsd = (np.exp(sc - lse_own[..., None]).astype(dtype) * (dp - Dr)).astype(dtype)
    out["drel"] = diag_sums(dsd.sum(axis=0, dtype=dtype), dtype)
    if mutant == "dw_scaled":
        out["drel"] = (out["drel"] * scale).astype(dtype)
    if cfg is not None:
        drel = out["drel"]
        if mutant == "dw_unclamped_only":            # the clipped tails |d| > L dropped
            c = check_config(cfg)
            d = np.arange(-(t - 1), t)
            drel = np.where((np.abs(d) <= c[1])[None, :], drel, dtype(0)) if c[0] == "clip" else drel
        out["dw"] = fold(drel, cfg, t, dtype)
    return out


def diag_sums(x, dtype=np.float64):
    """(H, t, t) [query][key] -> (H, 2t - 1): the sum over the cells with j - i = d at index d + t - 1"""
    H, t, _ = x.shape
    out = np.zeros((H, 2 * t - 1), dtype=dtype)
    for d in range(-(t - 1), t):
        out[:, d + t - 1] = np.diagonal(x, offset=d, axis1=1, axis2=2).sum(axis=1, dtype=dtype)
    return out


def fold(drel, cfg, t, dtype=np.float64):
    """(H, 2t - 1) -> (H, num_buckets): dw[g][n] = sum over the distances of bucket n, ascending d; 0 for an empty bucket"""
    mp = bucket_map(cfg, t)
    drel = np.asarray(drel, dtype=dtype)
    out = np.zeros((drel.shape[0], num_buckets(cfg)), dtype=dtype)
    for x in range(2 * t - 1):
        out[:, mp[x]] += drel[:, x]
    return out


def core_gates(q, k, v, rel, left, right, dctx, keep=None, s=1.0, mode="f32", lse=None, ctx=None, cfg=None, raw_dctx=False):
    """per-element gates for ctx, lse, dq, dk, dv, drel and (with cfg) dw (module docstring): window_formula.core_gates line by line on
    the biased p, with the score's extra rounding in delta and S.  raw_dctx (bf16): dctx is not bf16-representable and the kernel rounds
    it where it is an MFMA operand -- window_formula's raw dctx terms on the biased p (they enter drel and dw through ES)."""
    assert mode in ("f32", "bf16")
    q, k, v, dctx = (np.asarray(a, dtype=np.float64) for a in (q, k, v, dctx))
    B, t, H, dh = q.shape
    scale = 1.0 / np.sqrt(dh)
    r = core(q, k, v, rel, left, right, dctx, keep=keep, s=s, lse=lse, ctx=ctx)
    w = r["w"]
    ms = np.ones((1, 1, t, t)) if keep is None else np.asarray(keep).astype(np.float64) * float(s)
    e = 0.0 if keep is None else 1.0
    n_q = w.sum(axis=1).astype(np.float64)[None, None, :]
    n_k = w.sum(axis=0).astype(np.float64)
    aq, ak, av, ad = np.abs(q), np.abs(k), np.abs(v), np.abs(dctx)
    add = U * (np.abs(r["s_raw"]) + np.abs(r["bias"])[None])
    delta = np.where(w, (dh + 2) * U * scale * np.einsum("bihc,bjhc->bhij", aq, ak) + add, 0.0).max(axis=3)
    S = np.where(w, np.abs(r["s"]), 0.0).max(axis=3)
    rho = 2.0 * delta + M.c1(n_q) * U + 4.0 * U * S
    pb = 2.0 ** -8 if mode == "bf16" else 0.0
    g = {}
    g["ctx"] = (rho + (n_q + 2 + e) * U + pb).transpose(0, 2, 1)[..., None] * np.einsum("bhij,bjhc->bihc", r["pt"], av)
    g["lse"] = rho + 2.0 ** -23 * np.abs(r["lse"])
    lse = r["lse"] if lse is None else np.asarray(lse, dtype=np.float64)
    ctx = r["ctx"] if ctx is None else np.asarray(ctx, dtype=np.float64)
    p, ptb = r["p_bwd"], r["pt_bwd"]
    rho_b = delta + U * np.abs(lse) + 4.0 * U * S + 8.0 * U
    Abar = ms * np.einsum("bihc,bjhc->bhij", ad, av) + np.einsum("bihc,bihc->bhi", ad, np.abs(ctx))[..., None]
    pA = p * Abar
    ES = pA * (rho_b[..., None] + (dh + 5 + e) * U + pb)
    g["dv"] = np.einsum("bhij,bihc->bjhc", ptb * (rho_b[..., None] + (n_k[None, None, None, :] + 2 + e) * U + pb), ad)
    if raw_dctx and mode == "bf16":
        eps = M.round_bf16(dctx).astype(np.float64) - dctx
        ES = ES + p * ms * np.minimum(np.abs(np.einsum("bihc,bjhc->bhij", eps, v)), 2.0 ** -8 * np.einsum("bihc,bjhc->bhij", ad, av))
        g["dv"] = g["dv"] + np.minimum(np.abs(np.einsum("bhij,bihc->bjhc", ptb, eps)), 2.0 ** -8 * np.einsum("bhij,bihc->bjhc", ptb, ad))
    g["dq"] = scale * np.einsum("bhij,bjhc->bihc", ES + (n_q[..., None] + 3) * U * pA, ak)
    g["dk"] = scale * np.einsum("bhij,bihc->bjhc", ES + (n_k[None, None, None, :] + 3) * U * pA, aq)
    n_d = B * diag_sums(np.broadcast_to(w.astype(np.float64), (H, t, t)))
    abs_ds, es = diag_sums(np.abs(r["ds"]).sum(axis=0)), diag_sums(ES.sum(axis=0))
    g["drel"] = (n_d + 2) * U * abs_ds + es
    if cfg is not None:
        g["dw"] = (fold(n_d, cfg, t) + 2) * U * fold(abs_ds, cfg, t) + fold(es, cfg, t)
    return g


# ---- the encoder stack with the bias ------------------------------------------------------------------------------------------------
def rel_name(l):
    return "rel_pos" if l == 0 else f"rel_pos_l{l}"


def head(x, Wa, rel, B, t, H, left, right, state=None, p=0.0, layer=0, pos_encoding=True, dh_out=None):
    """window_formula.head with the biased core; with dh_out also drel (H, 2t - 1)"""
    x = np.asarray(x, dtype=np.float64)
    R, C = x.shape
    dh = C // H
    if p:
        s = float(D.thr_scale(p)[1])
        ka = D.keep_attn(state, D.stream_id(layer, D.SITE_ATTN), B, H, t, p)
        ko = D.keep_rows(state, D.stream_id(layer, D.SITE_ATTN_OUT), R, C, p)
    else:
        s, ka, ko = 1.0, None, np.ones((R, C), dtype=np.uint8)
    xp = x + np.tile(M.positional_table(t, C), (B, 1)) if pos_encoding else x
    qkv = xp @ Wa["in_proj_weight"].T + Wa["in_proj_bias"]
    q, k, v = M.split_qkv(qkv, B, t, H, dh)
    c = core(q, k, v, rel, left, right, keep=ka, s=s)
    ctx = c["ctx"].reshape(R, C)
    a = ctx @ Wa["out_proj.weight"].T + Wa["out_proj.bias"]
    out = dict(h=D.add_layernorm(xp, a, ko, s, Wa["norm.weight"], Wa["norm.bias"])["y"], qkv=qkv, ctx=ctx, lse=c["lse"])
    if dh_out is None:
        return out
    lb = D.add_layernorm(xp, a, ko, s, Wa["norm.weight"], Wa["norm.bias"], dh_out)
    dres, da = lb["dres"], lb["da"]
    out["d_norm.weight"], out["d_norm.bias"] = lb["dgamma"], lb["dbeta"]
    out["d_out_proj.weight"], out["d_out_proj.bias"] = da.T @ ctx, da.sum(axis=0)
    out["dctx"] = da @ Wa["out_proj.weight"]
    cb = core(q, k, v, rel, left, right, out["dctx"].reshape(B, t, H, dh), keep=ka, s=s)
    dqkv = M.join_qkv(cb["dq"], cb["dk"], cb["dv"])
    out["dqkv"], out["drel"] = dqkv, cb["drel"]
    out["d_in_proj_weight"], out["d_in_proj_bias"] = dqkv.T @ xp, dqkv.sum(axis=0)
    out["dx"] = dqkv @ Wa["in_proj_weight"] + dres
    return out


def encoder(x, Wt, cfg, B, t, H, left, right, state=None, p=0.0, layers=1, ffn_width=0, act="relu", pos_encoding=True, conv=False,
            dh_out=None):
    """window_formula.encoder (post-LN stack, training mode) with every layer's scores biased by its own table Wt[rel_name(l) + ".weight"]
    (H, num_buckets); -> h, and with dh_out: dx and "d_" + name per parameter, the tables' included."""
    Wt = {n: np.asarray(a, dtype=np.float64) for n, a in Wt.items()}
    cur = np.asarray(x, dtype=np.float64)
    R, C = cur.shape
    s = float(D.thr_scale(p)[1]) if p else 1.0

    def rows(l, site, N):
        return D.keep_rows(state, D.stream_id(l, site), R, N, p) if p else np.ones((R, N), dtype=np.uint8)

    saved, out = [], {}
    for l in range(layers):
        an, nn_, fn, fnn = F.layer_names(l)
        Wa = {"in_proj_weight": Wt[an + ".in_proj_weight"], "in_proj_bias": Wt[an + ".in_proj_bias"], "out_proj.weight": Wt[an + ".out_proj.weight"],
              "out_proj.bias": Wt[an + ".out_proj.bias"], "norm.weight": Wt[nn_ + ".weight"], "norm.bias": Wt[nn_ + ".bias"]}
        pe = pos_encoding and l == 0
        rec = dict(x=cur, Wa=Wa, pe=pe, rel=expand(Wt[rel_name(l) + ".weight"], cfg, t))
        cur = head(cur, Wa, rec["rel"], B, t, H, left, right, state, p, l, pos_encoding=pe)["h"]
        rec["h1"] = cur
        if conv:
            cm, cn = V.conv_names(l)
            Wc = V.conv_state(Wt, l)
            m = V.module(cur, Wc, B, t, True)
            out[cm + ".bn.running_mean"], out[cm + ".bn.running_var"] = m["running_mean"], m["running_var"]
            kc = rows(l, D.SITE_CONV_OUT, C)
            rec.update(Wc=Wc, o=m["o"], kc=kc)
            cur = D.add_layernorm(cur, m["o"], kc, s, Wc["conv_norm.weight"], Wc["conv_norm.bias"])["y"]
        rec["hc"] = cur
        if ffn_width > 0:
            kh, kf = rows(l, D.SITE_FFN_HIDDEN, ffn_width), rows(l, D.SITE_FFN_OUT, C)
            f = D.ffn(cur, Wt[fn + ".linear1.weight"], Wt[fn + ".linear1.bias"], Wt[fn + ".linear2.weight"], Wt[fn + ".linear2.bias"], act, kh, s)
            rec.update(f=f["y"], kh=kh, kf=kf)
            cur = D.add_layernorm(cur, f["y"], kf, s, Wt[fnn + ".weight"], Wt[fnn + ".bias"])["y"]
        saved.append(rec)
    out["h"] = cur
    if dh_out is None:
        return out
    g = np.asarray(dh_out, dtype=np.float64)
    for l in reversed(range(layers)):
        an, nn_, fn, fnn = F.layer_names(l)
        rec = saved[l]
        if ffn_width > 0:
            lb = D.add_layernorm(rec["hc"], rec["f"], rec["kf"], s, Wt[fnn + ".weight"], Wt[fnn + ".bias"], g)
            out["d_" + fnn + ".weight"], out["d_" + fnn + ".bias"] = lb["dgamma"], lb["dbeta"]
            fb = D.ffn(rec["hc"], Wt[fn + ".linear1.weight"], Wt[fn + ".linear1.bias"], Wt[fn + ".linear2.weight"], Wt[fn + ".linear2.bias"], act,
                       rec["kh"], s, lb["da"])
            for kk, vv in (("linear1.weight", "dw1"), ("linear1.bias", "db1"), ("linear2.weight", "dw2"), ("linear2.bias", "db2")):
                out[f"d_{fn}.{kk}"] = fb[vv]
            g = fb["dx"] + lb["dres"]
        if conv:
            cm, cn = V.conv_names(l)
            Wc = rec["Wc"]
            lb = D.add_layernorm(rec["h1"], rec["o"], rec["kc"], s, Wc["conv_norm.weight"], Wc["conv_norm.bias"], g)
            out["d_" + cn + ".weight"], out["d_" + cn + ".bias"] = lb["dgamma"], lb["dbeta"]
            mb = V.module(rec["h1"], Wc, B, t, True, do=lb["da"])
            for n, a in mb.items():
                if n.startswith("d_"):
                    out["d_" + cm + "." + n[2:]] = a
            g = mb["dh"] + lb["dres"]
        hb = head(rec["x"], rec["Wa"], rec["rel"], B, t, H, left, right, state, p, l, pos_encoding=rec["pe"], dh_out=g)
        for kk in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"):
            out[f"d_{an}.{kk}"] = hb["d_" + kk]
        out["d_" + nn_ + ".weight"], out["d_" + nn_ + ".bias"] = hb["d_norm.weight"], hb["d_norm.bias"]
        out["d_" + rel_name(l) + ".weight"] = fold(hb["drel"], cfg, t)
        g = hb["dx"]
    out["dx"] = g
    return out


check = M.check
round_bf16 = M.round_bf16
