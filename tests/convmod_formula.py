"""The Conformer convolution module of csrc/sed_convmod.hip and the post-LN encoder layer around it as plain numpy formulas: the
definition the kernels are tested against (tests/test_gpu_convmod.py, tests/test_gpu_sa_conformer.py) and that is itself checked
against torch.nn.Conv1d / F.glu / BatchNorm1d / F.silu / LayerNorm in float64 on the host (tests/test_convmod_host.py).

Module.  h (R, C) with R = B t rows, k odd taps, p = (k - 1) / 2, W by torch's names:
    g  = h pointwise1.weight^T + pointwise1.bias                          (R, 2C)
    v  = g[:, :C] sigmoid(g[:, C:])                                       (GLU)
    z[b,i,c] = depthwise.bias[c] + sum_{j<k} depthwise.weight[c][0][j] v[b, i + j - p, c]      (zero outside the clip)
    y  = bn.weight (z - mean) invstd + bn.bias;  training: mean, biased variance over the R rows, running' = 0.9 running + 0.1 (mean,
         unbiased variance);  eval: the running statistics.  invstd = 1 / sqrt(var + 1e-5)
    s  = y sigmoid(y),   o = s pointwise2.weight^T + pointwise2.bias,   h_c = LayerNorm(h + o)  (conv_norm)
backward from ds (the gradient of s):
    gz = ds silu'(y), silu'(y) = sigma (1 + y (1 - sigma));  dbeta = sum gz, dgamma = sum gz xhat;
    training: dz = gamma invstd (gz - mean(gz) - xhat mean(gz xhat)) = ca gz + cb z + cc;  eval: dz = gamma invstd gz
    dv[b,i,c] = sum_j w[c][j] dz[b, i - j + p, c];  dg = (dv sigma | dv a sigma (1 - sigma));
    dw[c][j] = sum_{b,i} dz[b,i,c] v[b, i + j - p, c],  dbias[c] = sum dz
Layer l: h = LayerNorm(x + attention(x)) (tests/mhsa_formula.py), h_c as above, then LayerNorm(h_c + ffn(h_c)) with an FFN
(tests/ffn_formula.py).

Gates (derived here, not tuned on kernel output): per element |got - ref| <= gate, u = 2^-24 (U below), absolute values inside every
sum so that no cancellation in the reference shrinks a gate.  Each launch is fed the reference's values rounded to fp32, so a launch
carries its own terms only; TILE is the chain length of a per-workgroup fp32 sum (the kernel's frame tile, or its rows per workgroup).
  v       a sigmoid(gate): the device sigmoid 1 / (1 + expf(-x)) and the one product:            C_SIG u |v|
  z       k fmas on top of the bias: (k + 2) u (sum_j |w||v| + |b|), plus the error of v passed on: sum_j |w| C_SIG u |v|
  sums    (sum z, sum z^2) per channel, per-workgroup fp32 chains then fp64:  (TILE + 2) u sum |z| + sum gate_z  and
          (TILE + 3) u sum z^2 + sum 2 |z| gate_z
  finalise (the existing sed_bn_train_finalize, its own arithmetic: fp64 sums, mean = s / n, var = q / n - mean^2, results rounded to
          fp32): d_mean = d_s / n + u |mean|;  d_var = d_q / n + 2 |mean| d_s / n -- the cancellation of q / n - mean^2 makes this
          absolute error relative to mean(z^2), not to var, which is why the Gaussian family keeps |mean| <~ std;
          d_invstd = invstd^3 d_var / 2 + u invstd;  d_scale = |gamma| d_invstd + u |scale|;
          d_shift = |mean| d_scale + |scale| d_mean + 2 u (|beta| + |mean scale|);  running: 0.1 d_(mean | unbiased var) + 3 u (|0.9 r| + |0.1 x|)
  y, s    y = fma(z, scale, shift): u (|scale z| + |shift|);  s = silu(y): silu is 1.1-Lipschitz, so 1.1 d_y + C_SIG u |s|
  gz      ds silu'(y): |silu''| <= 1/2, so |ds| (d_y / 2 + C_DSILU u A(y)) + u |gz| with A(y) = sigma (1 + |y| (1 - sigma)) the
          absolute-value form of silu' (its two terms cancel for y < -1.28)
  bwd sums (sum gz, sum gz xhat):  (TILE + 2) u sum |gz| + sum gate_gz  and  (TILE + 5) u sum |gz| X + sum gate_gz X with
          X = (|z| + |mean|) invstd
  dz      ca gz + cb z + cc as two fmas: 3 u (|ca gz| + |cb z| + |cc|)
  dv      (k + 2) u sum_j |w||dz| + sum_j |w| gate_dz
  dg      value half dv sigma: sigma gate_dv + (C_SIG + 1) u |dv| sigma;  gate half dv a P, P = sigma (1 - sigma):
          d_sigma = C_SIG u sigma, d_(1 - sigma) = d_sigma + u (1 - sigma), d_P = d_sigma (1 - sigma) + sigma d_(1 - sigma) + u P,
          so |a| P gate_dv + |dv a| d_P + 2 u |dv a| P
  dw, db  (TILE + 2) u sum |dz||v| + sum gate_dz |v|  and  (TILE + 2) u sum |dz| + sum gate_dz  (fp32 per workgroup, fp64 across)
Inside the engine (tests/test_gpu_sa_at_size.py) a launch is fed the engine's own values instead, whose gate is then zero; what that
needs beyond the above is composed, not modelled anew, at the end of the gates section: gz behind the GEMM whose ds it overwrites
(gz_through_ds), the BatchNorm backward finalisations on given partial rows (bn_bwd_finalize) and the eval-mode coefficients (bn_eval).
C_SIG and C_DSILU are the accuracy of the device expf / sigmoid as the kernels use it.  The ROCm installation carries no table for
it, so both were measured once on the MI355X against float64 (tools/convmod_time.py --csig: v = a sigmoid(x) and silu'(x) over the
dense grid x in [-30, 30], step 2^-10, and x = 40) and doubled: the measured worst errors were 23.59 u |v| for the GLU (at x = -23.07),
24.06 u |s| for the SiLU (at x = -25.36) and 22.36 u A(x) for silu' (at x = -23.07) -- the error of expf(-x) grows with |x| for
x << 0; over |x| <= 8, where the tests' Gaussian operands lie, the tool reports the smaller figures of its second grid.  C_SIG covers
the GLU and the SiLU.
"""
import math

import numpy as np

import ffn_formula as F
import mhsa_formula as M

U = 2.0 ** -24
EPS = 1e-5
MOMENTUM = 0.1
C_SIG_MEASURED = 24.06       # the larger of the GLU's and the SiLU's
C_DSILU_MEASURED = 22.36
C_SIG = 49.0                 # 2 x 24.06, rounded up
C_DSILU = 45.0               # 2 x 22.36, rounded up
SILU_L = 1.1                 # sup |silu'| = 1.0998...


def sigmoid(x, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    with np.errstate(over="ignore"):
        return (dtype(1) / (dtype(1) + np.exp(-x).astype(dtype))).astype(dtype)


def silu_grad(y, dtype=np.float64):
    sg = sigmoid(y, dtype)
    return (sg * (dtype(1) + np.asarray(y, dtype=dtype) * (dtype(1) - sg))).astype(dtype)


def silu_grad_abs(y):
    sg = sigmoid(y)
    return sg * (1.0 + np.abs(y) * (1.0 - sg))


def conv_names(l):
    """the convolution module's names of layer l in Csa_AvgPooling's state_dict: convm, conv_norm (+ _l{l} from layer 1 on)"""
    s = "" if l == 0 else f"_l{l}"
    return "convm" + s, "conv_norm" + s


def shift_frames(a, d, B, t, wrap=False):
    """out[b, i] = a[b, i + d] inside the clip, zero outside (wrap: the mutant that reads the neighbouring clip's frames instead)"""
    R, C = a.shape
    if wrap:
        out = np.zeros_like(a)
        idx = np.arange(R) + d
        ok = (idx >= 0) & (idx < R)
        out[ok] = a[idx[ok]]
        return out
    a3 = a.reshape(B, t, C)
    out = np.zeros_like(a3)
    if d >= 0:
        if d < t:
            out[:, :t - d] = a3[:, d:]
    elif -d < t:
        out[:, -d:] = a3[:, :t + d]
    return out.reshape(R, C)


def glu(g, dtype=np.float64, mutant=None):
    g = np.asarray(g, dtype=dtype)
    C = g.shape[1] // 2
    a, gate = (g[:, C:], g[:, :C]) if mutant == "glu_swapped" else (g[:, :C], g[:, C:])
    return (a * sigmoid(gate, dtype)).astype(dtype)


def dwconv(v, w, bias, B, t, dtype=np.float64, mutant=None):
    """z from v (R, C), w (C, k) and bias (C,): the taps in the order the kernel takes them, each a multiply-add in `dtype`"""
    v, w, bias = (np.asarray(a, dtype=dtype) for a in (v, w, bias))
    k = w.shape[1]
    p = (k - 1) // 2
    if mutant == "flipped":
        w = w[:, ::-1]
    if mutant == "filters_swapped":
        w = w.copy()
        w[[0, 1]] = w[[1, 0]]
    z = np.zeros_like(v) if mutant == "no_dw_bias" else np.tile(bias[None, :], (v.shape[0], 1)).astype(dtype)
    off = 1 if mutant == "tap_offset" else 0
    for j in range(k):
        z = (z + w[None, :, j] * shift_frames(v, j - p + off, B, t, wrap=mutant == "halo_neighbour")).astype(dtype)
    return z


def dwconv_bwd(dz, v, w, B, t, dtype=np.float64):
    """-> dv (R, C), dw (C, k), dbias (C,)"""
    dz, v, w = (np.asarray(a, dtype=dtype) for a in (dz, v, w))
    k = w.shape[1]
    p = (k - 1) // 2
    dv = np.zeros_like(dz)
    dw = np.zeros_like(w)
    for j in range(k):
        dv = (dv + w[None, :, j] * shift_frames(dz, p - j, B, t)).astype(dtype)
        dw[:, j] = (dz * shift_frames(v, j - p, B, t)).sum(axis=0, dtype=dtype)
    return dv, dw, dz.sum(axis=0, dtype=dtype)


def bn_coeffs(z, gamma, beta, rmean, rvar, training, dtype=np.float64, mutant=None, eps=EPS):
    """-> dict mean, var (what normalises), invstd, scale, shift, and in training running_mean / running_var after the update"""
    z, gamma, beta, rmean, rvar = (np.asarray(a, dtype=dtype) for a in (z, gamma, beta, rmean, rvar))
    n = z.shape[0]
    out = {}
    if training:
        mean = z.mean(axis=0, dtype=np.float64)
        var = np.maximum((z.astype(np.float64) ** 2).mean(axis=0) - mean * mean, 0.0) if dtype != np.float64 else z.var(axis=0)
        unb = var * (n / (n - 1.0)) if n > 1 else var
        out["running_mean"] = (dtype(1 - MOMENTUM) * rmean + dtype(MOMENTUM) * mean.astype(dtype)).astype(dtype)
        out["running_var"] = (dtype(1 - MOMENTUM) * rvar + dtype(MOMENTUM) * unb.astype(dtype)).astype(dtype)
        if mutant == "unbiased_norm":
            var = unb
    else:
        mean, var = rmean.astype(np.float64), rvar.astype(np.float64)
    invstd = (1.0 / np.sqrt(var + eps)).astype(dtype)
    scale = (gamma * invstd).astype(dtype)
    out.update(mean=mean.astype(dtype), var=var, invstd=invstd, scale=scale, shift=(beta - mean.astype(dtype) * scale).astype(dtype))
    return out


def bn_silu(z, scale, shift, dtype=np.float64):
    z, scale, shift = (np.asarray(a, dtype=dtype) for a in (z, scale, shift))
    y = (z * scale + shift).astype(dtype)
    return y, (y * sigmoid(y, dtype)).astype(dtype)


def bn_silu_bwd(ds, z, scale, shift, mean, invstd, dtype=np.float64, mutant=None):
    """-> gz, sum gz, sum gz xhat"""
    ds, z, scale, shift, mean, invstd = (np.asarray(a, dtype=dtype) for a in (ds, z, scale, shift, mean, invstd))
    y = (z * scale + shift).astype(dtype)
    gz = (ds * silu_grad(z if mutant == "silu_grad_at_z" else y, dtype)).astype(dtype)
    xh = ((z - mean) * invstd).astype(dtype)
    return gz, gz.sum(axis=0, dtype=dtype), (gz * xh).sum(axis=0, dtype=dtype)


def bn_bwd_coeffs(sg, sgx, n, gamma, mean, invstd, training):
    """(ca, cb, cc) of dz = ca gz + cb z + cc, float64 (include/sed_hip.h: sed_bn_bwd_finalize / sed_bn_eval_bwd_finalize)"""
    gamma, mean, invstd = (np.asarray(a, dtype=np.float64) for a in (gamma, mean, invstd))
    ca = gamma * invstd
    if not training:
        return ca, np.zeros_like(ca), np.zeros_like(ca)
    mg, mgx = np.asarray(sg, dtype=np.float64) / n, np.asarray(sgx, dtype=np.float64) / n
    return ca, -gamma * invstd * invstd * mgx, -gamma * invstd * (mg - mean * invstd * mgx)


def glu_bwd(dv, g, dtype=np.float64):
    dv, g = np.asarray(dv, dtype=dtype), np.asarray(g, dtype=dtype)
    C = g.shape[1] // 2
    sg = sigmoid(g[:, C:], dtype)
    return np.concatenate([dv * sg, dv * g[:, :C] * (sg * (dtype(1) - sg))], axis=1).astype(dtype)


def module(h, W, B, t, training=True, do=None, dtype=np.float64, mutant=None):
    """The module from h (R, C) to o (before the residual LayerNorm).  W: pointwise1.weight (2C, C, 1), pointwise1.bias,
    depthwise.weight (C, 1, k), depthwise.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, pointwise2.weight (C, C, 1),
    pointwise2.bias.  do: the gradient of o -> also dh (without the residual branch) and "d_" + name for every parameter.
    dtype: float64 is the definition; float32 a plain implementation in that arithmetic (forward only)."""
    W = {n: np.asarray(a, dtype=dtype) for n, a in W.items() if n != "bn.num_batches_tracked"}
    h = np.asarray(h, dtype=dtype)
    R, C = h.shape
    w1, w2, wd = W["pointwise1.weight"].reshape(2 * C, C), W["pointwise2.weight"].reshape(C, C), W["depthwise.weight"].reshape(C, -1)
    g = ((h @ w1.T).astype(dtype) + W["pointwise1.bias"]).astype(dtype)
    v = glu(g, dtype, mutant)
    z = dwconv(v, wd, W["depthwise.bias"], B, t, dtype, mutant)
    bn = bn_coeffs(z, W["bn.weight"], W["bn.bias"], W["bn.running_mean"], W["bn.running_var"], training, dtype, mutant)
    y, s = bn_silu(z, bn["scale"], bn["shift"], dtype)
    o = ((s @ w2.T).astype(dtype) + W["pointwise2.bias"]).astype(dtype)
    out = dict(g=g, v=v, z=z, y=y, s=s, o=o, **{k: bn[k] for k in ("mean", "var", "invstd", "scale", "shift")})
    if training:
        out["running_mean"], out["running_var"] = bn["running_mean"], bn["running_var"]
    if do is None:
        return out
    do = np.asarray(do, dtype=dtype)
    out["d_pointwise2.weight"], out["d_pointwise2.bias"] = (do.T @ s).reshape(C, C, 1), do.sum(axis=0)
    ds = do @ w2
    gz, sg, sgx = bn_silu_bwd(ds, z, bn["scale"], bn["shift"], bn["mean"], bn["invstd"], dtype, mutant)
    out["d_bn.weight"], out["d_bn.bias"] = sgx, sg
    ca, cb, cc = bn_bwd_coeffs(sg, sgx, R, W["bn.weight"], bn["mean"], bn["invstd"], training)
    dz = ca * gz + cb * z + cc
    dv, dw, db = dwconv_bwd(dz, v, wd, B, t, dtype)
    out["d_depthwise.weight"], out["d_depthwise.bias"] = dw.reshape(C, 1, -1), db
    dg = glu_bwd(dv, g, dtype)
    out["d_pointwise1.weight"], out["d_pointwise1.bias"] = (dg.T @ h).reshape(2 * C, C, 1), dg.sum(axis=0)
    out.update(ds=ds, gz=gz, dz=dz, dv=dv, dg=dg, dh=dg @ w1, ca=ca, cb=cb, cc=cc)
    return out


def sublayer(h, W, Wn, B, t, training=True, dhc=None, dtype=np.float64, mutant=None):
    """h_c = LayerNorm(h + module(h)) with conv_norm's (weight, bias) = Wn; dhc: the gradient of h_c -> dh with the residual branch"""
    m = module(h, W, B, t, training, dtype=dtype, mutant=mutant)
    res = np.zeros_like(m["o"]) if mutant == "no_residual" else np.asarray(h, dtype=dtype)
    ln = M.add_layernorm(res, m["o"], Wn[0], Wn[1], dtype=dtype)
    out = dict(hc=ln["y"], o=m["o"])
    if training:
        out["running_mean"], out["running_var"] = m["running_mean"], m["running_var"]
    if dhc is None:
        return out
    lb = M.add_layernorm(h, m["o"], Wn[0], Wn[1], dhc)
    mb = module(h, W, B, t, training, do=lb["dres"])
    out.update({n: a for n, a in mb.items() if n.startswith("d_")})
    out["d_conv_norm.weight"], out["d_conv_norm.bias"] = lb["dgamma"], lb["dbeta"]
    out["dh"] = mb["dh"] + lb["dres"]
    return out


def conv_state(W, l):
    """layer l's module entries of a name -> array dict without the prefix (what Csa_AvgPooling.conv_module_state returns)"""
    cm, cn = conv_names(l)
    out = {n[len(cm) + 1:]: a for n, a in W.items() if n.startswith(cm + ".")}
    out.update({"conv_norm." + n[len(cn) + 1:]: a for n, a in W.items() if n.startswith(cn + ".")})
    return out


def encoder(x, W, B, t, H, layers=1, ffn_width=0, act="relu", pos_encoding=True, training=True, dh_out=None):
    """The stack with the convolution module in every layer, float64.  x (B*t, C) mel-mean rows; W by state_dict name.  -> h, the
    running statistics after a training forward ("convm.bn.running_mean" ...), and with dh_out: dx and "d_" + name per parameter."""
    W = {n: np.asarray(a, dtype=np.float64) for n, a in W.items()}
    cur = np.asarray(x, dtype=np.float64)
    saved, out = [], {}
    for l in range(layers):
        an, nn_, fn, fnn = F.layer_names(l)
        cm, cn = conv_names(l)
        Wa = {"in_proj_weight": W[an + ".in_proj_weight"], "in_proj_bias": W[an + ".in_proj_bias"], "out_proj.weight": W[an + ".out_proj.weight"],
              "out_proj.bias": W[an + ".out_proj.bias"], "norm.weight": W[nn_ + ".weight"], "norm.bias": W[nn_ + ".bias"]}
        pe = pos_encoding and l == 0
        h1 = M.head(cur, Wa, B, t, H, pos_encoding=pe)["h"]
        Wc = conv_state(W, l)
        Wn = (Wc["conv_norm.weight"], Wc["conv_norm.bias"])
        sl = sublayer(h1, Wc, Wn, B, t, training)
        if training:
            out[cm + ".bn.running_mean"], out[cm + ".bn.running_var"] = sl["running_mean"], sl["running_var"]
        rec = dict(x=cur, Wa=Wa, pe=pe, h1=h1, hc=sl["hc"], Wc=Wc, Wn=Wn)
        cur = sl["hc"]
        if ffn_width > 0:
            f = F.ffn(cur, W[fn + ".linear1.weight"], W[fn + ".linear1.bias"], W[fn + ".linear2.weight"], W[fn + ".linear2.bias"], act)
            rec["f"] = f["y"]
            cur = M.add_layernorm(cur, f["y"], W[fnn + ".weight"], W[fnn + ".bias"])["y"]
        saved.append(rec)
    out["h"] = cur
    if dh_out is None:
        return out
    g = np.asarray(dh_out, dtype=np.float64)
    for l in reversed(range(layers)):
        an, nn_, fn, fnn = F.layer_names(l)
        cm, cn = conv_names(l)
        rec = saved[l]
        if ffn_width > 0:
            lb = M.add_layernorm(rec["hc"], rec["f"], W[fnn + ".weight"], W[fnn + ".bias"], g)
            out["d_" + fnn + ".weight"], out["d_" + fnn + ".bias"] = lb["dgamma"], lb["dbeta"]
            fb = F.ffn(rec["hc"], W[fn + ".linear1.weight"], W[fn + ".linear1.bias"], W[fn + ".linear2.weight"], W[fn + ".linear2.bias"], act, lb["dres"])
            for k, v in (("linear1.weight", "dw1"), ("linear1.bias", "db1"), ("linear2.weight", "dw2"), ("linear2.bias", "db2")):
                out[f"d_{fn}.{k}"] = fb[v]
            g = fb["dx"] + lb["dres"]
        sb = sublayer(rec["h1"], rec["Wc"], rec["Wn"], B, t, training, dhc=g)
        for n, a in sb.items():
            if n.startswith("d_conv_norm."):
                out["d_" + cn + n[len("d_conv_norm"):]] = a
            elif n.startswith("d_"):
                out["d_" + cm + "." + n[2:]] = a
        hb = M.head(rec["x"], rec["Wa"], B, t, H, pos_encoding=rec["pe"], dh_out=sb["dh"])
        for k in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"):
            out[f"d_{an}.{k}"] = hb["d_" + k]
        out["d_" + nn_ + ".weight"], out["d_" + nn_ + ".bias"] = hb["d_norm.weight"], hb["d_norm.bias"]
        g = hb["dx"]
    out["dx"] = g
    return out


# ---- gates (module docstring) -------------------------------------------------------------------------------------------------------
def _conv_abs(a, w, B, t, transpose=False):
    """sum_j |w[c][j]| |a[b, i + j - p, c]| (transpose: i - j + p)"""
    a, w = np.abs(np.asarray(a, dtype=np.float64)), np.abs(np.asarray(w, dtype=np.float64))
    k = w.shape[1]
    p = (k - 1) // 2
    out = np.zeros_like(a)
    for j in range(k):
        out += w[None, :, j] * shift_frames(a, (p - j) if transpose else (j - p), B, t)
    return out


def fwd_gates(g, w, bias, B, t, tile):
    """sed_dwconv_glu_fwd: gates of v, z and the reduced statistics (sum z, sum z^2)"""
    g, w, bias = (np.asarray(a, dtype=np.float64) for a in (g, w, bias))
    k = w.shape[1]
    v = glu(g)
    z = dwconv(v, w, bias, B, t)
    gv = C_SIG * U * np.abs(v)
    gz = (k + 2) * U * (_conv_abs(v, w, B, t) + np.abs(bias)[None, :]) + _conv_abs(gv, w, B, t)
    return dict(v=gv, z=gz, sum=(tile + 2) * U * np.abs(z).sum(axis=0) + gz.sum(axis=0),
                sumsq=(tile + 3) * U * (z * z).sum(axis=0) + (2.0 * np.abs(z) * gz).sum(axis=0))


def finalize_gates(z, gate_z, gamma, beta, rmean, rvar, tile):
    """the training statistics and coefficients computed from a z that is within gate_z of the reference: mean, invstd, scale, shift,
    running_mean, running_var"""
    z, gate_z, gamma, beta, rmean, rvar = (np.asarray(a, dtype=np.float64) for a in (z, gate_z, gamma, beta, rmean, rvar))
    n = z.shape[0]
    r = bn_coeffs(z, gamma, beta, rmean, rvar, True)
    mean, invstd, scale = r["mean"], r["invstd"], r["scale"]
    d_s = ((tile + 2) * U * np.abs(z).sum(axis=0) + gate_z.sum(axis=0)) / n
    d_q = ((tile + 3) * U * (z * z).sum(axis=0) + (2.0 * np.abs(z) * gate_z).sum(axis=0)) / n
    d_mean = d_s + U * np.abs(mean)
    d_var = d_q + 2.0 * np.abs(mean) * d_s
    d_invstd = 0.5 * invstd ** 3 * d_var + U * invstd
    d_scale = np.abs(gamma) * d_invstd + U * np.abs(scale)
    d_shift = np.abs(mean) * d_scale + np.abs(scale) * d_mean + 2.0 * U * (np.abs(beta) + np.abs(mean * scale))
    unb = r["var"] * (n / (n - 1.0)) if n > 1 else r["var"]
    return dict(mean=d_mean, invstd=d_invstd, scale=d_scale, shift=d_shift,
                running_mean=MOMENTUM * d_mean + 3.0 * U * (np.abs((1 - MOMENTUM) * rmean) + np.abs(MOMENTUM * mean)),
                running_var=MOMENTUM * d_var * (n / max(n - 1.0, 1.0)) + 3.0 * U * (np.abs((1 - MOMENTUM) * rvar) + np.abs(MOMENTUM * unb)))


def bn_silu_gates(z, scale, shift):
    z, scale, shift = (np.asarray(a, dtype=np.float64) for a in (z, scale, shift))
    y, s = bn_silu(z, scale, shift)
    dy = U * (np.abs(scale * z) + np.abs(shift))
    return dict(s=SILU_L * dy + C_SIG * U * np.abs(s))


def bn_silu_bwd_gates(ds, z, scale, shift, mean, invstd, tile):
    ds, z, scale, shift, mean, invstd = (np.asarray(a, dtype=np.float64) for a in (ds, z, scale, shift, mean, invstd))
    y, _ = bn_silu(z, scale, shift)
    gz = ds * silu_grad(y)
    dy = U * (np.abs(scale * z) + np.abs(shift))
    ggz = np.abs(ds) * (0.5 * dy + C_DSILU * U * silu_grad_abs(y)) + U * np.abs(gz)
    X = (np.abs(z) + np.abs(mean)) * np.abs(invstd)
    return dict(gz=ggz, sum=(tile + 2) * U * np.abs(gz).sum(axis=0) + ggz.sum(axis=0),
                sumx=(tile + 5) * U * (np.abs(gz) * X).sum(axis=0) + (ggz * X).sum(axis=0))


def bwd_gates(gz, z, ca, cb, cc, v, g, w, B, t, tile):
    """sed_dwconv_glu_bwd: gates of dg (R, 2C), dw (C, k), dbias (C,)"""
    gz, z, ca, cb, cc, v, g, w = (np.asarray(a, dtype=np.float64) for a in (gz, z, ca, cb, cc, v, g, w))
    C, k = w.shape
    dz = ca * gz + cb * z + cc
    gdz = 3.0 * U * (np.abs(ca * gz) + np.abs(cb * z) + np.abs(cc))
    dv, _, _ = dwconv_bwd(dz, v, w, B, t)
    gdv = (k + 2) * U * _conv_abs(dz, w, B, t, transpose=True) + _conv_abs(gdz, w, B, t, transpose=True)
    a, sg = g[:, :C], sigmoid(g[:, C:])
    P = sg * (1.0 - sg)
    d_sg = C_SIG * U * sg
    d_1m = d_sg + U * (1.0 - sg)
    d_P = d_sg * (1.0 - sg) + sg * d_1m + U * P
    gval = sg * gdv + (C_SIG + 1.0) * U * np.abs(dv) * sg
    ggate = np.abs(a) * P * gdv + np.abs(dv * a) * d_P + 2.0 * U * np.abs(dv * a) * P
    p = (k - 1) // 2
    gdw = np.zeros((C, k))
    for j in range(k):
        sv = np.abs(shift_frames(v, j - p, B, t))
        gdw[:, j] = (tile + 2) * U * (np.abs(dz) * sv).sum(axis=0) + (gdz * sv).sum(axis=0)
    return dict(dg=np.concatenate([gval, ggate], axis=1), dw=gdw, dbias=(tile + 2) * U * np.abs(dz).sum(axis=0) + gdz.sum(axis=0))


# ---- the module inside the engine (tests/test_gpu_sa_at_size.py): compositions of the gates above with those of the launches around
# them.  Nothing new is modelled: the GEMM's gate comes from the caller (tests/test_gpu_crnn_exact_oracle.py's form), the BatchNorm
# finalisations' are the forms of tests/test_gpu_ops_exact_oracle.py (test_bn_bwd_finalize, test_bn_eval_coeffs) in numpy.
U64 = 2.0 ** -53
SAFE = 4.0                   # that file's safety factor over the operation count


def exact_colsum(part):
    """float64 column sums of partial rows [nparts][...] holding fp32 values, exact to the last float64 rounding"""
    a = np.asarray(part)
    if np.finfo(np.longdouble).nmant >= 63:
        return a.astype(np.longdouble).sum(axis=0).astype(np.float64)
    flat = a.reshape(a.shape[0], -1).astype(np.float64)
    return np.array([math.fsum(col) for col in flat.T]).reshape(a.shape[1:])


def gz_through_ds(ds_ref, e_ds, z, scale, shift, mean, invstd, tile):
    """sed_bn_silu_bwd_reduce writing gz over the ds a sed_gemm_nt has just produced: ds is seen only through gz = ds silu'(y).
    ds_ref: the product in float64, e_ds: its gate.  -> ((gz, sum gz, sum gz xhat) from ds_ref, their gates): the GEMM's error passed
    on, e_ds A(y) with A the absolute-value form of silu' (and its column sums, with X for the second), plus the launch's own gates
    taken at the largest |ds| the GEMM's gate allows, |ds_ref| + e_ds."""
    ds_ref, e_ds, z, scale, shift, mean, invstd = (np.asarray(a, dtype=np.float64) for a in (ds_ref, e_ds, z, scale, shift, mean, invstd))
    y, _ = bn_silu(z, scale, shift)
    own = bn_silu_bwd_gates(np.abs(ds_ref) + e_ds, z, scale, shift, mean, invstd, tile)
    passed = e_ds * silu_grad_abs(y)
    X = (np.abs(z) + np.abs(mean)) * np.abs(invstd)
    return bn_silu_bwd(ds_ref, z, scale, shift, mean, invstd), dict(gz=own["gz"] + passed, sum=own["sum"] + passed.sum(axis=0),
                                                                     sumx=own["sumx"] + (passed * X).sum(axis=0))


def bn_bwd_finalize(part, n, gamma, mean, invstd, training=True):
    """sed_bn_bwd_finalize (training) / sed_bn_eval_bwd_finalize on the partial rows part [nparts][2][C] = (sum gz, sum gz xhat) it is
    given.  -> (dbeta, dgamma, ca, cb, cc in float64 from the exact column sums, their gates): one rounding of a float64 value each
    (SAFE u), and the kernel's fp64 sum of nparts rows charged (ceil(nparts / 256) + 12) 2^-53 of the sum of magnitudes, passed on to
    cb and cc.  Eval: cb and cc are exactly 0 (gate 0)."""
    part, gm, mu, is_ = (np.asarray(a, dtype=np.float64) for a in (part, gamma, mean, invstd))
    nparts = part.shape[0]
    (s, q), (sa, qa) = exact_colsum(part), exact_colsum(np.abs(part))
    c64 = (-(-nparts // 256) + 12) * U64
    ca, cb, cc = bn_bwd_coeffs(s, q, n, gm, mu, is_, training)
    gates = dict(dbeta=SAFE * U * np.abs(s) + c64 * sa, dgamma=SAFE * U * np.abs(q) + c64 * qa, ca=SAFE * U * np.abs(ca),
                 cb=np.zeros_like(ca), cc=np.zeros_like(ca))
    if training:
        Sc = np.abs(gm * is_) * (np.abs(s) / n + np.abs(mu * is_ * q) / n)
        gates["cb"] = SAFE * U * np.abs(cb) + np.abs(gm * is_ * is_) * c64 * qa / n
        gates["cc"] = SAFE * U * Sc + np.abs(gm * is_) * c64 * (sa + np.abs(mu * is_) * qa) / n + 4.0 * U64 * Sc
    return dict(dbeta=s, dgamma=q, ca=ca, cb=cb, cc=cc), gates


def bn_eval(gamma, beta, rmean, rvar, eps=EPS):
    """sed_bn_eval_coeffs and sed_bn_eval_stats.  -> (scale, shift, mean, invstd in float64, their gates): invstd = 1 / sqrtf(rvar + eps)
    is 4 roundings, scale 5, shift 7 of |beta| + |mean scale| (test_bn_eval_coeffs); mean is the running mean's own bits (gate 0)."""
    gamma, beta, rmean, rvar = (np.asarray(a, dtype=np.float64) for a in (gamma, beta, rmean, rvar))
    r = bn_coeffs(np.zeros((1, gamma.shape[0])), gamma, beta, rmean, rvar, False, eps=eps)
    ref = {n: r[n] for n in ("scale", "shift", "mean", "invstd")}
    return ref, dict(scale=SAFE * 5 * U * np.abs(r["scale"]), shift=SAFE * 7 * U * (np.abs(beta) + np.abs(rmean * r["scale"])),
                     mean=np.zeros_like(rmean), invstd=SAFE * 4 * U * r["invstd"])


# ---- operand families ---------------------------------------------------------------------------------------------------------------
def exact_case(rng, B, t, C, k):
    """The exact-integer family: the value half of g in {-2 .. 2}, the gate half 40.0 (sigmoid rounds to exactly 1 in fp32 and in
    float64), filters in {-1, 0, 1}, bias in {-2 .. 2}; for the backward gz and z in {-2 .. 2}, ca in {1, 2}, cb in {0, 1}, cc in
    {-1, 0, 1}, v in {-2 .. 2}.  Every value is a small integer and every sum stays far below 2^24: float64 and fp32 arithmetic give
    the same values in any order."""
    R = B * t
    i32 = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float32)
    g = np.concatenate([i32(-2, 2, (R, C)), np.full((R, C), 40.0, dtype=np.float32)], axis=1)
    return dict(g=g, w=i32(-1, 1, (C, k)), bias=i32(-2, 2, C), gz=i32(-2, 2, (R, C)), z=i32(-2, 2, (R, C)), ca=i32(1, 2, C),
                cb=i32(0, 1, C), cc=i32(-1, 1, C), v=i32(-2, 2, (R, C)))


def gaussian_case(rng, B, t, C, k):
    """The Gaussian family: g standard normal with a per-channel offset of at most a quarter of a standard deviation, filters uniform
    in +-1/sqrt(k) (torch's range) and a bias within +-0.1, so that z has |mean| <~ std per channel (within 2 std, checked in
    tests/test_convmod_host.py) and the reference's own q / n - mean^2 does not cancel."""
    R = B * t
    f = lambda a: np.asarray(a, dtype=np.float32)
    g = f(rng.standard_normal((R, 2 * C)) + 0.25 * rng.uniform(-1, 1, 2 * C)[None, :])
    b = 1.0 / np.sqrt(k)
    return dict(g=g, w=f(rng.uniform(-b, b, (C, k))), bias=f(rng.uniform(-0.1, 0.1, C)), ds=f(rng.standard_normal((R, C))),
                gamma=f(rng.uniform(0.5, 1.5, C)), beta=f(rng.uniform(-0.5, 0.5, C)), rmean=f(rng.uniform(-0.2, 0.2, C)),
                rvar=f(rng.uniform(0.5, 1.5, C)))


check = M.check
