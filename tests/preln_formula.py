"""The pre-LN residual LayerNorm of the self-attention head (sed_resid_layernorm_fwd / sed_resid_layernorm_bwd, csrc/sed_layernorm.hip) and the
pre-LN / macaron (Conformer) encoder stack of Csa_AvgPooling(sa_norm_first=True) as plain numpy: the float64 definition of the two
kernels, forward and backward, of a layer and of a stack, and the gates.  The kernels are tested against this
(tests/test_gpu_preln.py, tests/test_gpu_sa_preln.py); this file is itself checked against torch.nn.TransformerEncoder(
TransformerEncoderLayer(norm_first=True), N, norm=LayerNorm) and a torch-module composition of the macaron + convolution block in float64
on the host (tests/test_preln_host.py).  It builds on mhsa_formula (LayerNorm), ffn_formula, convmod_formula, window_formula,
relpos_formula and dropout_formula as they are.

Kernels.  With f = fp32(s * msd) per element -- msd the row-dropout keep factor m * sd of dropout_formula (sd = fp32(1 / (1 - p)), m the
0 / 1 keep bit of stream 8 layer + site; msd = 1 for p = 0); the product with s is DEFINED as the fp32 product, so the reference takes
that rounding too:
    forward    xsum = x + f a,   y = LayerNorm(xsum) gamma + beta,   stats = (mean, rstd) of xsum          a absent: y = LayerNorm(x)
    backward   g = dy gamma, xhat = (xsum - mean) rstd from the GIVEN xsum and stats (what the kernel is fed):
               dxsum = dres_in + rstd (g - mean_c(g) - xhat mean_c(g xhat))      da = f dxsum
               dgamma = sum_rows dy xhat,  dbeta = sum_rows dy

Layer l on the residual stream x (R = B t rows, C columns; the positional table added once before layer 0):
    [macaron]      x <- x + 1/2 FFNm(LN(x))     ffn_mac_norm*, ffn_mac*
                   x <- x + MHSA(LN(x))         attn_norm*, attn*, [rel_pos*]
    [conv]         x <- x + ConvModule(LN(x))   conv_norm*, convm*
    [ffn]          x <- x + s FFN(LN(x))        ffn_norm*, ffn*;   s = 1/2 with macaron, else 1
    [closing]      x <- LN(x)                   out_norm*          every layer with macaron, else the last layer only
Dropout sites: 0 attention probabilities, 1 attention output, 2 convolution module output, 3 FFN hidden, 4 FFN output (dropout_formula),
5 the macaron FFN's hidden activation, 6 the macaron FFN's output before its add.

Gates, u = 2^-24, derived from mhsa_formula's LayerNorm gate ((C + 8) u of the absolute-value expression):
    xsum    one fma: the only rounding is the result's, u |xsum| <= u (|x| + |f a|); held to 2 u (|x| + |f a|).
    y       mhsa_formula's y gate evaluated on z = xsum, plus the error e = gate(xsum) carried through the LayerNorm to first order:
            |gamma_c| rstd (e_c + mean_c(e) + |xhat_c| mean_c(e |xhat|)).  stats: the mean within (C + 8) u mean_c|z| + mean_c(e); rstd
            has no gate of its own (on a row of variance ~ eps its relative error is not first order) -- it is held through y, and bit
            for bit against sed_add_layernorm_fwd where s = 1.
    dxsum   mhsa_formula's dres gate (xsum and stats are inputs of the backward, exact fp32 numbers, so nothing is carried) plus the
            rounding of the add, u |dres_in| (the other half of that rounding, u |d|, is inside the (C + 8) u).
    da      |f| gate(dxsum) + u |da|: one more rounding.
    dgamma, dbeta   mhsa_formula's ((rows + 8) u of the absolute-value sums).
"""
import numpy as np

import convmod_formula as V
import dropout_formula as D
import ffn_formula as F
import mhsa_formula as M
import relpos_formula as RP

U = M.U
EPS = M.EPS
SITE_MAC_HIDDEN, SITE_MAC_OUT = 5, 6
check = M.check


def factor(s, keep=None, sd=1.0, shape=None):
    """f = fp32(s * m sd) per element as float64 (the defined fp32 product); keep None: no dropout"""
    if keep is None:
        return np.full(shape, float(np.float32(s) * np.float32(sd)), dtype=np.float64) if shape is not None else float(np.float32(s) * np.float32(sd))
    return (np.float32(s) * (np.asarray(keep).astype(np.float32) * np.float32(sd))).astype(np.float64)


def resid_layernorm(x, a, s, gamma, beta, keep=None, sd=1.0, dy=None, dres_in=None, xsum=None, stats=None, eps=EPS, dtype=np.float64,
                    mutant=None):
    """The two kernels.  a None: y = LayerNorm(x).  -> dict xsum, y, mean, rstd and, with dy: dxsum, da (None without a), dgamma, dbeta.
    The backward takes xsum and stats (rows, 2) as GIVEN where they are (what sed_resid_layernorm_bwd is fed), else its own forward's.
    dtype float32: a plain implementation in that arithmetic.  mutant: drop_dres_in, da_without_s, xhat_from_x."""
    x, gamma, beta = (np.asarray(v, dtype=dtype) for v in (x, gamma, beta))
    if a is None:
        f, z = None, x
    else:
        f = factor(s, keep, sd, x.shape).astype(dtype)
        z = (np.asarray(a, dtype=dtype) * f + x).astype(dtype)
    zero = np.zeros_like(z)
    out = M.add_layernorm(z, zero, gamma, beta, eps=eps, dtype=dtype)
    out = dict(xsum=z, y=out["y"], mean=out["mean"], rstd=out["rstd"])
    if dy is None:
        return out
    zb = z if xsum is None else np.asarray(xsum, dtype=dtype)
    if mutant == "xhat_from_x":
        zb = x
    st = np.stack([out["mean"], out["rstd"]], axis=1) if stats is None else stats
    lb = M.add_layernorm(zb, np.zeros_like(zb), gamma, beta, dy, eps=eps, dtype=dtype, stats=st)
    d = lb["dres"]
    if dres_in is not None and mutant != "drop_dres_in":
        d = (np.asarray(dres_in, dtype=dtype) + d).astype(dtype)
    out.update(dxsum=d, dgamma=lb["dgamma"], dbeta=lb["dbeta"], da=None)
    if a is not None:
        fb = f if mutant != "da_without_s" else (f / dtype(s)).astype(dtype)
        out["da"] = (d * fb).astype(dtype)
    return out


def resid_layernorm_gates(x, a, s, gamma, beta, keep=None, sd=1.0, dy=None, dres_in=None, xsum=None, stats=None, eps=EPS):
    """The gates of resid_layernorm's outputs (module docstring): xsum, y, mean and, with dy, dxsum, da, dgamma, dbeta."""
    x, gamma, beta = (np.asarray(v, dtype=np.float64) for v in (x, gamma, beta))
    rows, C = x.shape
    r = resid_layernorm(x, a, s, gamma, beta, keep, sd, eps=eps)
    z = r["xsum"]
    zero = np.zeros_like(z)
    if a is None:
        e = zero
    else:
        e = 2.0 * U * (np.abs(x) + np.abs(factor(s, keep, sd, x.shape) * np.asarray(a, dtype=np.float64)))
    ones = np.ones_like(z)
    g0 = M.add_layernorm_gates(z, zero, gamma, beta, ones, eps)
    rstd = r["rstd"][:, None]
    xh = (z - r["mean"][:, None]) * rstd
    az = np.abs(z)
    Mz = az.mean(axis=1, keepdims=True)
    k = (C + 8) * U
    out = dict(xsum=e,
               y=g0["y"] + np.abs(gamma) * rstd * (e + e.mean(axis=1, keepdims=True) + np.abs(xh) * (e * np.abs(xh)).mean(axis=1, keepdims=True)),
               mean=(k * Mz + e.mean(axis=1, keepdims=True))[:, 0])
    if dy is None:
        return out
    zb = z if xsum is None else np.asarray(xsum, dtype=np.float64)
    gb = M.add_layernorm_gates(zb, np.zeros_like(zb), gamma, beta, dy, eps, stats=stats)
    rb = resid_layernorm(x, a, s, gamma, beta, keep, sd, dy, dres_in, xsum, stats, eps)
    out["dxsum"] = gb["dres"] + (U * np.abs(np.asarray(dres_in, dtype=np.float64)) if dres_in is not None else 0.0)
    out["dgamma"], out["dbeta"] = gb["dgamma"], gb["dbeta"]
    if a is not None:
        out["da"] = np.abs(factor(s, keep, sd, x.shape)) * out["dxsum"] + U * np.abs(rb["da"])
    return out


# ---- names ---------------------------------------------------------------------------------------------------------------------------
def sfx(l):
    return "" if l == 0 else f"_l{l}"


def sublayers(l, macaron, conv, ffn_width):
    """layer l's sub-layers in forward order: (kind, module, norm module, residual weight, dropout site of the output)"""
    x = sfx(l)
    out = [("mac", "ffn_mac" + x, "ffn_mac_norm" + x, 0.5, SITE_MAC_OUT)] if macaron else []
    out.append(("attn", "attn" + x, "attn_norm" + x, 1.0, D.SITE_ATTN_OUT))
    if conv:
        out.append(("conv", "convm" + x, "conv_norm" + x, 1.0, D.SITE_CONV_OUT))
    if ffn_width:
        out.append(("ffn", "ffn" + x, "ffn_norm" + x, 0.5 if macaron else 1.0, D.SITE_FFN_OUT))
    return out


def has_closing(l, layers, macaron):
    return macaron or l == layers - 1


def module_order(layers, macaron, conv, ffn_width, rel):
    """registration order of the head's parameter modules: every norm before its sub-layer, rel_pos behind attn, out_norm last"""
    names = []
    for l in range(layers):
        for kind, mod, norm, _, _ in sublayers(l, macaron, conv, ffn_width):
            names += [norm, mod] + (["rel_pos" + sfx(l)] if rel and kind == "attn" else [])
        if has_closing(l, layers, macaron):
            names.append("out_norm" + sfx(l))
    return names


# ---- the stack -----------------------------------------------------------------------------------------------------------------------
def _ln(x, W, name, dy=None):
    gamma = W.get(name + ".weight", np.ones(x.shape[1]))
    beta = W.get(name + ".bias", np.zeros(x.shape[1]))
    return M.add_layernorm(x, np.zeros_like(x), gamma, beta, dy)


def encoder(x, Wt, B, t, H, layers=1, ffn_width=0, act="relu", macaron=False, conv=False, window=(None, None), rel_cfg=None, state=None,
            p=0.0, pos_encoding=True, training=True, dh_out=None, mutant=None):
    """The pre-LN stack in float64.  x (B*t, C) mel-mean rows; Wt: dict by state_dict name.  conv: the convolution module (its kernel size
    is the depthwise weight's); window (left, right), None unbounded; rel_cfg: relpos_formula's checked configuration or None; state, p:
    dropout_formula's state words and probability (training only).  -> h (and the running statistics of the BatchNorms); with dh_out
    also dx and "d_" + name per parameter.  mutant: no_half_mac, no_half_ffn, post_ln, no_closing, inner_closing, shared_ffn."""
    Wt = {n: np.asarray(a, dtype=np.float64) for n, a in Wt.items()}
    cur = np.asarray(x, dtype=np.float64)
    R, C = cur.shape
    dh = C // H
    p = p if training else 0.0
    sd = float(D.thr_scale(p)[1]) if p else 1.0
    left, right = window
    if pos_encoding:
        cur = cur + np.tile(M.positional_table(t, C), (B, 1))

    def rows(l, site, N):
        return D.keep_rows(state, D.stream_id(l, site), R, N, p) if p else np.ones((R, N), dtype=np.uint8)

    tape, out = [], {}
    for l in range(layers):
        for kind, mod, norm, s, site in sublayers(l, macaron, conv, ffn_width):
            if (kind == "mac" and mutant == "no_half_mac") or (kind == "ffn" and mutant == "no_half_ffn"):
                s = 1.0
            n = cur if mutant == "post_ln" else _ln(cur, Wt, norm)["y"]
            rec = dict(kind=kind, mod=mod, norm=norm, x=cur, n=n, l=l)
            if kind == "attn":
                qkv = n @ Wt[mod + ".in_proj_weight"].T + Wt[mod + ".in_proj_bias"]
                q, k, v = M.split_qkv(qkv, B, t, H, dh)
                rel = RP.expand(Wt["rel_pos" + sfx(l) + ".weight"], rel_cfg, t) if rel_cfg is not None else np.zeros((H, 2 * t - 1))
                ka = D.keep_attn(state, D.stream_id(l, D.SITE_ATTN), B, H, t, p) if p else None
                ctx = RP.core(q, k, v, rel, left, right, keep=ka, s=sd)["ctx"].reshape(R, C)
                a = ctx @ Wt[mod + ".out_proj.weight"].T + Wt[mod + ".out_proj.bias"]
                rec.update(q=q, k=k, v=v, rel=rel, ka=ka, ctx=ctx)
            elif kind == "conv":
                Wc = {nm[len(mod) + 1:]: arr for nm, arr in Wt.items() if nm.startswith(mod + ".")}
                m = V.module(n, Wc, B, t, training)
                if training:
                    out[mod + ".bn.running_mean"], out[mod + ".bn.running_var"] = m["running_mean"], m["running_var"]
                a = m["o"]
                rec.update(Wc=Wc)
            else:
                wm = "ffn" + sfx(l) if (kind == "mac" and mutant == "shared_ffn") else mod
                kh = rows(l, D.SITE_FFN_HIDDEN if kind == "ffn" else SITE_MAC_HIDDEN, ffn_width)
                a = D.ffn(n, Wt[wm + ".linear1.weight"], Wt[wm + ".linear1.bias"], Wt[wm + ".linear2.weight"], Wt[wm + ".linear2.bias"], act, kh, sd)["y"]
                rec.update(kh=kh, wm=wm)
            f = factor(s, rows(l, site, C), sd)
            rec.update(f=f)
            cur = cur + f * a
            if mutant == "post_ln":
                rec["z"] = cur
                cur = _ln(cur, Wt, norm)["y"]
            tape.append(rec)
        if (has_closing(l, layers, macaron) and not (mutant == "no_closing" and l == layers - 1)) or mutant == "inner_closing":
            name = "out_norm" + sfx(l)
            tape.append(dict(kind="closing", norm=name, x=cur))
            cur = _ln(cur, Wt, name)["y"]
    out["h"] = cur
    if dh_out is None:
        return out
    assert mutant is None
    gs = np.asarray(dh_out, dtype=np.float64)          # the gradient of the residual stream
    for rec in reversed(tape):
        kind, norm = rec["kind"], rec["norm"]
        if kind == "closing":
            lb = _ln(rec["x"], Wt, norm, gs)
            out["d_" + norm + ".weight"], out["d_" + norm + ".bias"] = lb["dgamma"], lb["dbeta"]
            gs = lb["dres"]
            continue
        mod, n, l = rec["mod"], rec["n"], rec["l"]
        da = rec["f"] * gs
        if kind == "attn":
            out["d_" + mod + ".out_proj.weight"], out["d_" + mod + ".out_proj.bias"] = da.T @ rec["ctx"], da.sum(axis=0)
            dctx = da @ Wt[mod + ".out_proj.weight"]
            cb = RP.core(rec["q"], rec["k"], rec["v"], rec["rel"], left, right, dctx.reshape(B, t, H, dh), keep=rec["ka"], s=sd)
            dqkv = M.join_qkv(cb["dq"], cb["dk"], cb["dv"])
            if rel_cfg is not None:
                out["d_rel_pos" + sfx(l) + ".weight"] = RP.fold(cb["drel"], rel_cfg, t)
            out["d_" + mod + ".in_proj_weight"], out["d_" + mod + ".in_proj_bias"] = dqkv.T @ n, dqkv.sum(axis=0)
            dn = dqkv @ Wt[mod + ".in_proj_weight"]
        elif kind == "conv":
            mb = V.module(n, rec["Wc"], B, t, training, do=da)
            for nm, arr in mb.items():
                if nm.startswith("d_"):
                    out["d_" + mod + "." + nm[2:]] = arr
            dn = mb["dh"]
        else:
            fb = D.ffn(n, Wt[mod + ".linear1.weight"], Wt[mod + ".linear1.bias"], Wt[mod + ".linear2.weight"], Wt[mod + ".linear2.bias"], act,
                       rec["kh"], sd, da)
            for kk, vv in (("linear1.weight", "dw1"), ("linear1.bias", "db1"), ("linear2.weight", "dw2"), ("linear2.bias", "db2")):
                out[f"d_{mod}.{kk}"] = fb[vv]
            dn = fb["dx"]
        lb = _ln(rec["x"], Wt, norm, dn)
        out["d_" + norm + ".weight"], out["d_" + norm + ".bias"] = lb["dgamma"], lb["dbeta"]
        gs = gs + lb["dres"]
    out["dx"] = gs
    return out


def stack_gate(h, layers, C, Dw, t, stages=12):
    """The gate of a whole stack's output in fp32 arithmetic, ffn_formula.stack_gate's reasoning: the closing LayerNorm's output is O(1)
    per element, each sum of a layer has at most max(C, D, t) terms, and a layer is a chain of at most `stages` stages (two FFNs of two
    products, the attention's three products and softmax, the convolution module's two products, depthwise sum and BatchNorm, up to five
    LayerNorms -- twelve counts the longest dependent chain), each of whose errors the next LayerNorm passes on with a factor of order one."""
    return float(stages) * layers * (max(C, Dw, t) + 8) * U * (1.0 + np.abs(np.asarray(h, dtype=np.float64)))
