"""The local attention window of the self-attention head (the WIN instantiations of csrc/sed_mhsa.hip behind sed_mhsa_fwd_win /
sed_mhsa_bwd_win) as plain numpy: the float64 definition over explicit t x t matrices, forward and backward, with an optional dropout
keep mask (dropout_formula.keep_attn), the windowed encoder stack, the brute-force tile count and the gates.  The kernels are tested
against this (tests/test_gpu_window.py, tests/test_gpu_sa_window.py); this file is itself checked against torch.nn.MultiheadAttention
(attn_mask=) and torch.nn.TransformerEncoderLayer(src_mask=) in float64 on the host (tests/test_window_host.py).

Window.  left >= 0, right >= 0 (None: unbounded).  Key j of the same clip takes part for query i iff i - left <= j <= i + right:
w_ij = 1 there, 0 elsewhere (torch's attn_mask is its negation).  The diagonal is always inside, so no row is empty.

Definitions (float64), in mhsa_formula's / dropout_formula's symbols, ms_ij = m_ij s (1 without dropout):
    s_ij as unwindowed;  lse_i = max_{j in W_i} s_ij + ln sum_{j in W_i} exp(s_ij - max),   p_ij = w_ij exp(s_ij - lse_i)
    p~_ij = ms_ij p_ij,   ctx_ic = sum_j p~_ij v_jc,   D_i = sum_c dctx_ic ctx_ic
    dv_jc = sum_i p~_ij dctx_ic,   dp_ij = ms_ij sum_c dctx_ic v_jc,   ds_ij = p_ij (dp_ij - D_i)   (0 outside the window, as p is)
    dq_ic = scale sum_j ds_ij k_jc,   dk_jc = scale sum_i ds_ij q_ic
An unbounded window is mhsa_formula.core (dropout_formula.core with a mask) term for term.

Tiles.  A pass walks 32 x 32 tiles (query tile, key tile); tiles_brute counts those that hold at least one in-window cell of a real
row and a real key.  (Passes 0 and 2 group them by query tile, pass 1 by key tile: the same set of tiles.)

Gates (derived here from mhsa_formula's and dropout_formula's, not tuned on kernel output; U = 2^-24).  The derivations of those two
docstrings go through line by line with p_ij = 0 outside the window; what changes is which keys a row's sums and maxima run over:
  delta_i   (dh + 2) U scale max_{j in W_i} sum_c |q_ic| |k_jc|: only in-window scores enter the row's maximum and sum.
  S_i       max_{j in W_i} |s_ij|.
  c1        The sum of a row has n_i = |W_i| positive terms ((n_i - 1) U) and the running maximum is rescaled once per VISITED tile, at
            most n_i / 32 + 2 of them (6 U each; a visited tile with no key of the row multiplies l = 0 by a factor and adds 0:
            exact): c1(n_i) = 2 n_i + 32 covers both, as c1(t) does for t keys.  rho_i = 2 delta_i + c1(n_i) U + 4 U S_i.
  ctx       (rho_i + (n_i + 2 + e) U + pb) sum_j p~_ij |v_jc|: an n_i-term product sum; e = 1 with dropout (the multiply by s), pb = 2^-8
            in bf16 (the operand rounding of p~).
  lse       rho_i + 2^-23 |lse_i|.
  backward  rho'_i = delta_i + U |lse_i| + 4 U S_i + 8 U;  Abar_ij = ms_ij sum_c |dctx||v| + sum_c |dctx||ctx|;
            ES_ij = p_ij Abar_ij (rho'_i + (dh + 5 + e) U + pb)  (0 outside the window: the kernel selects 0 there, it does not multiply)
            dv_jc: sum_i p~_ij |dctx_ic| (rho'_i + (n'_j + 2 + e) U + pb) with n'_j the number of in-window QUERIES of key j (the length
                   of dv's sum)
            dq_ic: scale sum_j (ES_ij + (n_i + 3) U p_ij Abar_ij) |k_jc|;   dk_jc: scale sum_i (ES_ij + (n'_j + 3) U p_ij Abar_ij) |q_ic|
  raw dctx  (bf16, raw_dctx=True)  mhsa_formula's terms for a dctx the kernel rounds as an operand, with p (p~) over the window: the
            deterministic shift |sum_i p~_ij eps_ic| on dv and p_ij ms_ij |sum_c eps_ic v_jc| on ES, eps = round(dctx) - dctx, each
            capped by its absolute-value form at 2^-8, the half ulp of 8 significant bits at the bottom of a binade: |eps| <= 2^-8 |dctx|.
            mhsa_formula caps at 2^-9, the top-of-binade figure, which sums over all t keys stay far below; under a window it is no
            bound -- window (3, 0) leaves the last key of a clip ONE query, whose dv moves by its actual p~ eps, up to 2^-8 p~ |dctx|.
            A float64 emulation of the documented rounding with exact accumulation missed the 2^-9 cap at 1.24 gates there (and
            the kernel at 1.19, tests/test_gpu_sa_block_at_size.py's configuration AR); at 2^-8 it stands at 0.99.  Where the shift is
            below the 2^-9 form, as in every sum of more than a few terms, the gate is the one it was.
  teacher-forced  lse=, ctx= as in mhsa_formula: the backward half takes the lse and ctx it is given.
"""
import numpy as np

import convmod_formula as V
import dropout_formula as D
import ffn_formula as F
import mhsa_formula as M

U = 2.0 ** -24
TILE = 32


def sides(t, left, right):
    """None / >= t - 1 -> t - 1 (unbounded)"""
    cap = max(t - 1, 0)
    return (cap if left is None else min(int(left), cap)), (cap if right is None else min(int(right), cap))


def in_window(t, left, right):
    """bool (t, t): [query][key]"""
    left, right = sides(t, left, right)
    i = np.arange(t)[:, None]
    j = np.arange(t)[None, :]
    return (j >= i - left) & (j <= i + right)


def torch_mask(t, left, right):
    """torch's attn_mask / src_mask: True where the key must NOT be attended to"""
    return ~in_window(t, left, right)


def tiles_brute(t, left, right, which=0):
    """tiles of pass `which` (0 forward, 1 dK / dV, 2 dQ) with at least one in-window cell of a real row"""
    assert which in (0, 1, 2)
    w = in_window(t, left, right)
    n = 0
    for a0 in range(0, t, TILE):
        for b0 in range(0, t, TILE):
            blk = w[b0:b0 + TILE, a0:a0 + TILE] if which == 1 else w[a0:a0 + TILE, b0:b0 + TILE]
            n += int(blk.any())
    return n


def _window_for(t, left, right, mutant):
    if mutant == "swapped":
        return in_window(t, right, left)
    if mutant == "left_off_by_one":
        return in_window(t, None if left is None else left + 1, right)
    if mutant == "right_off_by_one":
        return in_window(t, left, None if right is None else right + 1)
    if mutant == "tile_start":                       # the window measured from the query tile's first query
        l, r = sides(t, left, right)
        i = (np.arange(t)[:, None] // TILE) * TILE
        j = np.arange(t)[None, :]
        return ((j >= i - l) & (j <= i + r)) | np.eye(t, dtype=bool)
    return in_window(t, left, right)


def core(q, k, v, left, right, dctx=None, keep=None, s=1.0, dtype=np.float64, mutant=None, bf16_operands=False, lse=None, ctx=None):
    """The windowed core: the definition (float64) or a plain implementation in `dtype` arithmetic.  keep (B, H, t, t) 0 / 1 and s: the
    dropout mask and scale (None: no dropout).  lse (B, H, t), ctx (B, t, H, dh): teacher-forced backward, as mhsa_formula.core.
    mutant: swapped, left_off_by_one, right_off_by_one, tile_start, no_renorm, bwd_unmasked, lse_all (tests/test_window_host.py)."""
    q, k, v = (np.asarray(a, dtype=dtype) for a in (q, k, v))
    B, t, H, dh = q.shape
    w = _window_for(t, left, right, mutant)[None, None]
    ms = np.ones((1, 1, t, t), dtype=dtype) if keep is None else (np.asarray(keep).astype(dtype) * dtype(s)).astype(dtype)
    scale = dtype(1.0 / np.sqrt(dh))
    sc = (np.einsum("bihc,bjhc->bhij", q, k).astype(dtype) * scale).astype(dtype)
    sw = sc if mutant == "no_renorm" else np.where(w, sc, dtype(-np.inf))
    m = sw.max(axis=3, keepdims=True)
    e = np.exp(sw - m).astype(dtype)
    l = e.sum(axis=3, keepdims=True, dtype=dtype)
    p = np.where(w, e / l, dtype(0)).astype(dtype)
    lse_own = (m + np.log(l)).astype(dtype)[..., 0]
    if mutant == "lse_all":
        ma = sc.max(axis=3, keepdims=True)
        lse_own = (ma + np.log(np.exp(sc - ma).sum(axis=3, keepdims=True, dtype=dtype))).astype(dtype)[..., 0]
    pt = (p * ms).astype(dtype)
    rb = (lambda a: M.round_bf16(a).astype(dtype)) if bf16_operands else (lambda a: a)
    out = dict(ctx=np.einsum("bhij,bjhc->bihc", rb(pt), v).astype(dtype), lse=lse_own, p=p, pt=pt, s=sc, w=w[0, 0])
    if dctx is None:
        return out
    dctx = np.asarray(dctx, dtype=dtype)
    if mutant == "bwd_unmasked":                     # P rebuilt from the (windowed) lse over every key of the clip
        p = np.exp(sc - lse_own[..., None]).astype(dtype)
    elif mutant == "lse_all":
        p = np.where(w, np.exp(sc - lse_own[..., None]), dtype(0)).astype(dtype)
    elif lse is not None:
        p = (p * np.exp(lse_own - np.asarray(lse, dtype=dtype))[..., None].astype(dtype)).astype(dtype)
    ptb = (p * ms).astype(dtype)
    out["p_bwd"], out["pt_bwd"] = p, ptb
    cD = out["ctx"] if ctx is None else np.asarray(ctx, dtype=dtype)
    Dr = np.einsum("bihc,bihc->bhi", dctx, cD).astype(dtype)[..., None]
    dp = (np.einsum("bihc,bjhc->bhij", dctx, v).astype(dtype) * ms).astype(dtype)
    ds = (p * (dp - Dr)).astype(dtype)
    out["dv"] = np.einsum("bhij,bihc->bjhc", rb(ptb), dctx).astype(dtype)
    out["dq"] = (scale * np.einsum("bhij,bjhc->bihc", rb(ds), k)).astype(dtype)
    out["dk"] = (scale * np.einsum("bhij,bihc->bjhc", rb(ds), q)).astype(dtype)
    return out


def core_gates(q, k, v, left, right, dctx, keep=None, s=1.0, mode="f32", lse=None, ctx=None, raw_dctx=False):
    """per-element gates for ctx, lse, dq, dk, dv (module docstring).  raw_dctx (bf16): dctx is not bf16-representable and the kernel
    rounds it where it is an MFMA operand -- mhsa_formula's raw dctx terms, over the window."""
    assert mode in ("f32", "bf16")
    q, k, v, dctx = (np.asarray(a, dtype=np.float64) for a in (q, k, v, dctx))
    B, t, H, dh = q.shape
    scale = 1.0 / np.sqrt(dh)
    r = core(q, k, v, left, right, dctx, keep=keep, s=s, lse=lse, ctx=ctx)
    w = r["w"]
    ms = np.ones((1, 1, t, t)) if keep is None else np.asarray(keep).astype(np.float64) * float(s)
    e = 0.0 if keep is None else 1.0
    n_q = w.sum(axis=1).astype(np.float64)[None, None, :]                 # in-window keys per query
    n_k = w.sum(axis=0).astype(np.float64)                                # in-window queries per key
    aq, ak, av, ad = np.abs(q), np.abs(k), np.abs(v), np.abs(dctx)
    delta = (dh + 2) * U * scale * np.where(w, np.einsum("bihc,bjhc->bhij", aq, ak), 0.0).max(axis=3)
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
    return g


# ---- the windowed encoder stack -----------------------------------------------------------------------------------------------------
def head(x, Wa, B, t, H, left, right, state=None, p=0.0, layer=0, pos_encoding=True, dh_out=None):
    """dropout_formula.head with the windowed core (p = 0: every mask is all ones and s = 1, which is mhsa_formula.head windowed)"""
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
    c = core(q, k, v, left, right, keep=ka, s=s)
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
    cb = core(q, k, v, left, right, out["dctx"].reshape(B, t, H, dh), keep=ka, s=s)
    dqkv = M.join_qkv(cb["dq"], cb["dk"], cb["dv"])
    out["dqkv"] = dqkv
    out["d_in_proj_weight"], out["d_in_proj_bias"] = dqkv.T @ xp, dqkv.sum(axis=0)
    out["dx"] = dqkv @ Wa["in_proj_weight"] + dres
    return out


def encoder(x, W, B, t, H, left, right, state=None, p=0.0, layers=1, ffn_width=0, act="relu", pos_encoding=True, conv=False,
            dh_out=None):
    """dropout_formula.encoder (post-LN stack, training mode) with every layer's attention windowed; p = 0: no dropout.
    -> h, with conv the running statistics, and with dh_out: dx and "d_" + name per parameter."""
    W = {n: np.asarray(a, dtype=np.float64) for n, a in W.items()}
    cur = np.asarray(x, dtype=np.float64)
    R, C = cur.shape
    s = float(D.thr_scale(p)[1]) if p else 1.0

    def rows(l, site, N):
        return D.keep_rows(state, D.stream_id(l, site), R, N, p) if p else np.ones((R, N), dtype=np.uint8)

    saved, out = [], {}
    for l in range(layers):
        an, nn_, fn, fnn = F.layer_names(l)
        Wa = {"in_proj_weight": W[an + ".in_proj_weight"], "in_proj_bias": W[an + ".in_proj_bias"], "out_proj.weight": W[an + ".out_proj.weight"],
              "out_proj.bias": W[an + ".out_proj.bias"], "norm.weight": W[nn_ + ".weight"], "norm.bias": W[nn_ + ".bias"]}
        pe = pos_encoding and l == 0
        rec = dict(x=cur, Wa=Wa, pe=pe)
        cur = head(cur, Wa, B, t, H, left, right, state, p, l, pos_encoding=pe)["h"]
        rec["h1"] = cur
        if conv:
            cm, cn = V.conv_names(l)
            Wc = V.conv_state(W, l)
            m = V.module(cur, Wc, B, t, True)
            out[cm + ".bn.running_mean"], out[cm + ".bn.running_var"] = m["running_mean"], m["running_var"]
            kc = rows(l, D.SITE_CONV_OUT, C)
            rec.update(Wc=Wc, o=m["o"], kc=kc)
            cur = D.add_layernorm(cur, m["o"], kc, s, Wc["conv_norm.weight"], Wc["conv_norm.bias"])["y"]
        rec["hc"] = cur
        if ffn_width > 0:
            kh, kf = rows(l, D.SITE_FFN_HIDDEN, ffn_width), rows(l, D.SITE_FFN_OUT, C)
            f = D.ffn(cur, W[fn + ".linear1.weight"], W[fn + ".linear1.bias"], W[fn + ".linear2.weight"], W[fn + ".linear2.bias"], act, kh, s)
            rec.update(f=f["y"], kh=kh, kf=kf)
            cur = D.add_layernorm(cur, f["y"], kf, s, W[fnn + ".weight"], W[fnn + ".bias"])["y"]
        saved.append(rec)
    out["h"] = cur
    if dh_out is None:
        return out
    g = np.asarray(dh_out, dtype=np.float64)
    for l in reversed(range(layers)):
        an, nn_, fn, fnn = F.layer_names(l)
        rec = saved[l]
        if ffn_width > 0:
            lb = D.add_layernorm(rec["hc"], rec["f"], rec["kf"], s, W[fnn + ".weight"], W[fnn + ".bias"], g)
            out["d_" + fnn + ".weight"], out["d_" + fnn + ".bias"] = lb["dgamma"], lb["dbeta"]
            fb = D.ffn(rec["hc"], W[fn + ".linear1.weight"], W[fn + ".linear1.bias"], W[fn + ".linear2.weight"], W[fn + ".linear2.bias"], act,
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
        hb = head(rec["x"], rec["Wa"], B, t, H, left, right, state, p, l, pos_encoding=rec["pe"], dh_out=g)
        for kk in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"):
            out[f"d_{an}.{kk}"] = hb["d_" + kk]
        out["d_" + nn_ + ".weight"], out["d_" + nn_ + ".bias"] = hb["d_norm.weight"], hb["d_norm.bias"]
        g = hb["dx"]
    out["dx"] = g
    return out


check = M.check
round_bf16 = M.round_bf16
