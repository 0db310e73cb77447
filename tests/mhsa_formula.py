"""The self-attention temporal head of csrc/sed_mhsa.hip as plain numpy formulas over explicit t x t matrices: the definition the
kernels are tested against (tests/test_gpu_mhsa.py, tests/test_gpu_sa_model.py) and that is itself checked against
torch.nn.MultiheadAttention + torch.nn.LayerNorm in float64 on the host (tests/test_mhsa_host.py).

Core.  q, k, v, dctx are (B, t, H, dh) (head g = columns [g*dh, (g+1)*dh) of a third of a qkv row), scale = 1/sqrt(dh); per clip
and head, i and j over the t frames of the SAME clip:
    s_ij = scale sum_c q_ic k_jc,   lse_i = max_j s_ij + ln sum_j exp(s_ij - max),   p_ij = exp(s_ij - lse_i),   ctx_ic = sum_j p_ij v_jc
    D_i = sum_c dctx_ic ctx_ic,   dv_jc = sum_i p_ij dctx_ic,   dp_ij = sum_c dctx_ic v_jc,   ds_ij = p_ij (dp_ij - D_i)
    dq_ic = scale sum_j ds_ij k_jc,   dk_jc = scale sum_i ds_ij q_ic
Add + LayerNorm.  z = x + a, mean and BIASED variance over the C columns of a row, rstd = 1/sqrt(var + eps), xhat = (z - mean) rstd,
y = xhat gamma + beta;  g = dy gamma,  dres = rstd (g - mean_c g - xhat mean_c(g xhat)) (the gradient of x and of a),
dgamma = sum_rows dy xhat, dbeta = sum_rows dy.
Head.  x' = x + pe[frame],  qkv = x' Win^T + bin,  ctx = core(qkv),  a = ctx Wout^T + bout,  h = LayerNorm(x' + a); the positional
table pe[i][2j] = sin(i / 10000^(2j/C)), pe[i][2j+1] = cos(i / 10000^(2j/C)).

Gates (derived here, not tuned on kernel output).  u = 2^-24 is fp32's unit roundoff; every gate is per element,
|got - ref| <= gate, and every gate is a rounding count times the SAME expression over absolute values, so no cancellation in the
reference can shrink it.  mode "f32": every product exact, accumulation in fp32.
  score     A scaled score is a dot product of dh terms (an fma chain: dh roundings) times the scale (1 rounding):
            |err s_ij| <= delta_i = (dh + 2) u scale max_j sum_c |q_ic| |k_jc|.
  weights   p_ij = exp(s_ij - lse_i).  Its relative error is at most the error of s_ij plus that of lse_i (each <= delta_i, the
            second because lse is a maximum plus a log-sum whose derivative with respect to the scores is a convex combination):
            2 delta_i; plus the exp and sum roundings: an expf is good to 2 ulp (4 u), its argument s_ij - m is rounded once
            (u |s_ij - m| <= 2 u S_i with S_i = max_j |s_ij|), the running maximum's rescale factors exp(m_old - m_new) telescope over
            the key tiles to another 2 u S_i plus 6 u per tile (exp, multiply, add), and a sum of t positive terms carries (t - 1) u
            whatever its order.  With ceil(t/32) tiles that is at most c1(t) u + 4 u S_i, c1(t) = 2 t + 32, linear in t.
            rho_i = 2 delta_i + c1(t) u + 4 u S_i.
  ctx       |err ctx_ic| <= (rho_i + (t + 2) u) sum_j p_ij |v_jc|: the weights' error plus the t-term product sum and the division.
  lse       |err lse_i| <= rho_i + 2^-23 |lse_i| (absolute: the logarithm of a sum with relative error rho_i, and its own roundings).
  backward  The test feeds the kernel lse and ctx as the reference rounded to fp32.  P is rebuilt with relative error
            rho'_i = delta_i + u |lse_i| + 4 u S_i + 8 u (one score, the stored lse, the exp and its argument).  Every cancelling
            difference is replaced by the sum of absolute values: with Abar_ij = sum_c |dctx_ic| |v_jc| + sum_c |dctx_ic| |ctx_ic|
            (for dp_ij - D_i; both are dh-term dot products, (dh + 3) u each counting the rounding of the stored ctx),
              |err ds_ij| <= p_ij Abar_ij (rho'_i + (dh + 5) u)                                =: ES_ij
              |err dv_jc| <= sum_i p_ij |dctx_ic| (rho'_i + (t + 2) u)
              |err dq_ic| <= scale sum_j (ES_ij + (t + 3) u p_ij Abar_ij) |k_jc|
              |err dk_jc| <= scale sum_i (ES_ij + (t + 3) u p_ij Abar_ij) |q_ic|
  mode "bf16"  The cases feed bf16-representable q, k, v and dctx, so the operand roundings of those are exact and products of two
            bf16 values are exact in fp32: everything above holds unchanged, plus the two internal operand roundings: P as the
            operand of P.V and of dV costs at most 2^-8 relative per weight (2^-8 sum_j p_ij |v_jc| on ctx, 2^-8 sum_i p_ij |dctx_ic|
            on dv), dS as the operand of dQ and dK costs 2^-8 of its absolute-value form p_ij Abar_ij (added to ES_ij).
  raw dctx  (mode "bf16", raw_dctx=True)  In the engine dctx comes out of a GEMM and is not bf16-representable: the kernel rounds it
            to nearest even where it is an MFMA operand.  With eps_ic = round(dctx_ic) - dctx_ic, half an ulp of 8 significant bits
            is between 2^-9 |dctx_ic| (top of a binade) and 2^-8 |dctx_ic| (bottom); the gate is held to 2^-9, the smaller figure.
            dctx is an operand in exactly two products, both linear in it, so the shift of the exact result is known:
              dV = P^T dctx:   dv_jc moves by sum_i p_ij eps_ic,            at most 2^-9 sum_i p_ij |dctx_ic| in absolute values
              dP = dctx V^T:   dp_ij moves by sum_c eps_ic v_jc and ds_ij = p_ij (dp_ij - D_i) by p_ij times that,
                                                                            at most 2^-9 p_ij sum_c |dctx_ic| |v_jc|
            The absolute-value forms alone are too generous: they widen the dk gate by 1.4 and the mutant without D
            (tests/test_mhsa_host.py), 10.7 gates out under the representable dctx, would pass at 7.6.  The shift itself is a
            deterministic function of the inputs (nearest-even is what the kernel documents and what the raw-operand test of
            tests/test_gpu_mhsa.py holds it to, bit for bit), so by the triangle inequality the gate adds |shift| -- the smaller of
            |sum_i p_ij eps_ic| and the absolute-value form on dv, the smaller of p_ij |sum_c eps_ic v_jc| and the absolute-value
            form added to ES_ij and so carried into dq and dk -- never more than the 2^-9 forms.  D_i = sum_c dctx_ic ctx_ic is
            taken from the fp32 dctx (the kernel header says so): its term keeps the raw dctx and does not change.  The reference
            stays the float64 definition on the raw dctx.
  teacher-forced  core(..., lse=, ctx=) and core_gates(..., lse=, ctx=): the backward half takes the lse and ctx it is GIVEN (what
            sed_mhsa_bwd is fed) in place of the definition's own: p_ij = exp(s_ij - lse_i) -- evaluated as p_ij exp(lse_i(own) -
            lse_i), the same number, so that the definition's own lse reproduces the default path bit for bit -- and
            D_i = sum_c dctx_ic ctx_ic(given).  The backward derivation above already treats lse and ctx as exact fp32 inputs, so the
            gates only read |lse| in rho' and |ctx| in Abar from the given values, and p from the rebuilt weights.
            add_layernorm(..., stats=) / add_layernorm_gates(..., stats=): the backward takes (mean, rstd) per row as given
            ((rows, 2), what sed_add_layernorm_bwd is fed) in xhat = (z - mean) rstd and in the factor rstd of dres.
  LayerNorm Held to (C + 8) u of its absolute-value expression (C-term sums for the mean and the variance, a handful of roundings
            around them).  With M = mean_c |z_c| and X_c = rstd (|z_c| + M) (the absolute-value form of xhat; the error of the
            difference z_c - mean is relative to |z_c| + M, not to the difference):
              y      A = |gamma_c| (X_c + |xhat_c| rstd^2 mean_c(|d_c| (|z_c| + M))) + |beta_c|     (the second term: rstd's own error,
                     through the centred squares)
              dres   A = rstd (|g_c| + mean_c |g| + X_c mean_c(|g| X))      (stats fed as the reference rounded to fp32)
              dgamma (rows + 8) u sum_rows |dy| X,    dbeta (rows + 8) u sum_rows |dy|
"""
import numpy as np

U = 2.0 ** -24
EPS = 1e-5


def c1(t):
    return 2.0 * t + 32.0


def positional_table(t, C):
    """(t, C) float64: pe[i][2j] = sin(i / 10000^(2j/C)), pe[i][2j+1] = cos(the same)"""
    i = np.arange(t, dtype=np.float64)[:, None]
    j2 = (np.arange(C) // 2 * 2).astype(np.float64)[None, :]
    ang = i / np.power(10000.0, j2 / C)
    return np.where(np.arange(C)[None, :] % 2 == 0, np.sin(ang), np.cos(ang))


def split_qkv(qkv, B, t, H, dh):
    """[B*t][3C] -> q, k, v (B, t, H, dh)"""
    a = np.asarray(qkv).reshape(B, t, 3, H, dh)
    return a[:, :, 0], a[:, :, 1], a[:, :, 2]


def join_qkv(q, k, v):
    B, t, H, dh = q.shape
    return np.stack([q, k, v], axis=2).reshape(B * t, 3 * H * dh)


def core(q, k, v, dctx=None, dtype=np.float64, mutant=None, bf16_operands=False, lse=None, ctx=None, round_dctx=False):
    """The definition (dtype float64) or a plain implementation of it in `dtype` arithmetic (float32: what the gates must pass).
    bf16_operands: P and dS are rounded to bf16 where they are operands (the bf16 kernel's internal roundings).
    round_dctx: dctx is rounded to bf16 where it is an MFMA operand (dp and dv), not in D.
    lse (B, H, t), ctx (B, t, H, dh): teacher-forced -- the backward half rebuilds p and D from these (module docstring).
    mutant: a deliberately wrong definition (tests/test_mhsa_host.py).  -> dict ctx, lse (B, H, t) and, with dctx, dq, dk, dv."""
    q, k, v = (np.asarray(a, dtype=dtype) for a in (q, k, v))
    B, t, H, dh = q.shape
    scale = dtype(1.0 / np.sqrt(dh))
    kk, vv = k, v
    if mutant == "neighbour_clip":                  # the keys / values of the next clip are attended to as well
        kk = np.concatenate([k, np.roll(k, -1, axis=0)], axis=1)
        vv = np.concatenate([v, np.roll(v, -1, axis=0)], axis=1)
    if mutant == "drop_last_key":
        kk, vv = k[:, :-1], v[:, :-1]
    if mutant == "swap_heads_v" and H > 1:
        vv = v[:, :, ::-1]
    s = np.einsum("bihc,bjhc->bhij", q, kk).astype(dtype)
    if mutant != "no_scale":
        s = s * scale
    ax = 2 if mutant == "softmax_over_queries" else 3
    m = s.max(axis=ax, keepdims=True)
    e = np.exp(s - m).astype(dtype)
    l = e.sum(axis=ax, keepdims=True, dtype=dtype)
    p = (e / l).astype(dtype)
    lse_own = (m + np.log(l)).astype(dtype)
    pv = round_bf16(p).astype(dtype) if bf16_operands else p
    out = dict(ctx=np.einsum("bhij,bjhc->bihc", pv, vv).astype(dtype), lse=lse_own[:, :, :, 0] if ax == 3 else lse_own[:, :, 0, :], p=p, s=s)
    if dctx is None:
        return out
    dctx = np.asarray(dctx, dtype=dtype)
    if lse is not None:
        assert ax == 3
        p = (p * np.exp(out["lse"] - np.asarray(lse, dtype=dtype))[..., None].astype(dtype)).astype(dtype)
        pv = round_bf16(p).astype(dtype) if bf16_operands else p
    out["p_bwd"] = p
    ctx = out["ctx"] if ctx is None else np.asarray(ctx, dtype=dtype)
    D = np.einsum("bihc,bihc->bhi", dctx, ctx).astype(dtype)[:, :, :, None]
    dop = round_bf16(dctx).astype(dtype) if round_dctx else dctx
    dp = np.einsum("bihc,bjhc->bhij", dop, vv).astype(dtype)
    ds = (p * dp if mutant == "no_D" else p * (dp - D)).astype(dtype)
    dso = round_bf16(ds).astype(dtype) if bf16_operands else ds
    out["dv"] = np.einsum("bhij,bihc->bjhc", pv, dop).astype(dtype)
    out["dq"] = (scale * np.einsum("bhij,bjhc->bihc", dso, kk)).astype(dtype)
    dk = np.einsum("bhij,bihc->bjhc", dso, q).astype(dtype)
    out["dk"] = dk if mutant == "dk_no_scale" else (scale * dk).astype(dtype)
    return out


def core_loops(q, k, v, dctx):
    """the same definition as plain loops (float64), for small sizes"""
    q, k, v, dctx = (np.asarray(a, dtype=np.float64) for a in (q, k, v, dctx))
    B, t, H, dh = q.shape
    scale = 1.0 / np.sqrt(dh)
    out = dict(ctx=np.zeros_like(q), lse=np.zeros((B, H, t)), dq=np.zeros_like(q), dk=np.zeros_like(q), dv=np.zeros_like(q))
    for b in range(B):
        for g in range(H):
            P = np.zeros((t, t))
            for i in range(t):
                s = np.array([scale * float(q[b, i, g] @ k[b, j, g]) for j in range(t)])
                mx = s.max()
                lse = mx + np.log(np.exp(s - mx).sum())
                out["lse"][b, g, i] = lse
                P[i] = np.exp(s - lse)
                out["ctx"][b, i, g] = P[i] @ v[b, :, g]
            for i in range(t):
                D = float(dctx[b, i, g] @ out["ctx"][b, i, g])
                for j in range(t):
                    ds = P[i, j] * (float(dctx[b, i, g] @ v[b, j, g]) - D)
                    out["dv"][b, j, g] += P[i, j] * dctx[b, i, g]
                    out["dq"][b, i, g] += scale * ds * k[b, j, g]
                    out["dk"][b, j, g] += scale * ds * q[b, i, g]
    return out


def core_gates(q, k, v, dctx, mode="f32", raw_dctx=False, lse=None, ctx=None):
    """-> dict of per-element gates for ctx, lse, dq, dk, dv (module docstring) from the float64 definition.  raw_dctx (bf16): dctx
    is not bf16-representable and the kernel rounds it.  lse, ctx: the teacher-forced backward (its gates; ctx and lse keep theirs)."""
    assert mode in ("f32", "bf16")
    q, k, v, dctx = (np.asarray(a, dtype=np.float64) for a in (q, k, v, dctx))
    B, t, H, dh = q.shape
    scale = 1.0 / np.sqrt(dh)
    r = core(q, k, v, dctx, lse=lse, ctx=ctx)
    p, s, ctx_own, lse_own = r["p"], r["s"], r["ctx"], r["lse"]
    aq, ak, av, ad = np.abs(q), np.abs(k), np.abs(v), np.abs(dctx)
    delta = (dh + 2) * U * scale * np.einsum("bihc,bjhc->bhij", aq, ak).max(axis=3)          # (B, H, t)
    S = np.abs(s).max(axis=3)
    rho = 2.0 * delta + c1(t) * U + 4.0 * U * S
    pb = 2.0 ** -8 if mode == "bf16" else 0.0
    g = {}
    pav = np.einsum("bhij,bjhc->bihc", p, av)
    g["ctx"] = (rho + (t + 2) * U + pb).transpose(0, 2, 1)[..., None] * pav
    g["lse"] = rho + 2.0 ** -23 * np.abs(lse_own)
    lse = lse_own if lse is None else np.asarray(lse, dtype=np.float64)
    ctx = ctx_own if ctx is None else np.asarray(ctx, dtype=np.float64)
    p = r["p_bwd"]
    rho_b = delta + U * np.abs(lse) + 4.0 * U * S + 8.0 * U
    dV = np.einsum("bihc,bjhc->bhij", ad, av)
    Abar = dV + np.einsum("bihc,bihc->bhi", ad, np.abs(ctx))[..., None]
    pA = p * Abar
    ES = pA * (rho_b[..., None] + (dh + 5) * U + pb)
    eps = round_bf16(dctx).astype(np.float64) - dctx          # the operand rounding of a raw dctx
    if raw_dctx and mode == "bf16":
        ES = ES + p * np.minimum(np.abs(np.einsum("bihc,bjhc->bhij", eps, v)), 2.0 ** -9 * dV)
    g["dv"] = np.einsum("bhij,bihc->bjhc", p * (rho_b[..., None] + (t + 2) * U + pb), ad)
    if raw_dctx and mode == "bf16":
        g["dv"] = g["dv"] + np.minimum(np.abs(np.einsum("bhij,bihc->bjhc", p, eps)), 2.0 ** -9 * np.einsum("bhij,bihc->bjhc", p, ad))
    tot = ES + (t + 3) * U * pA
    g["dq"] = scale * np.einsum("bhij,bjhc->bihc", tot, ak)
    g["dk"] = scale * np.einsum("bhij,bihc->bjhc", tot, aq)
    return g


def round_bf16(a):
    """nearest-even rounding of float32 values to bf16, returned as float32"""
    b = np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)
    r = ((b.astype(np.uint64) + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32).reshape(np.shape(a))


def add_layernorm(x, a, gamma, beta, dy=None, eps=EPS, dtype=np.float64, mutant=None, stats=None):
    """-> dict y, mean, rstd (rows,) and, with dy, dres, dgamma, dbeta.  stats (rows, 2): the backward uses these (mean, rstd)."""
    x, a, gamma, beta = (np.asarray(v, dtype=dtype) for v in (x, a, gamma, beta))
    C = x.shape[1]
    z = x + a
    mean = z.mean(axis=1, keepdims=True, dtype=dtype)
    d = z - mean
    var = (d * d).sum(axis=1, keepdims=True, dtype=dtype) / dtype(C - 1 if mutant == "unbiased_variance" else C)
    rstd = (1.0 / np.sqrt(var + dtype(eps))).astype(dtype)
    xh = d * rstd
    out = dict(y=(xh * gamma + beta).astype(dtype), mean=mean[:, 0], rstd=rstd[:, 0], xhat=xh, z=z)
    if dy is None:
        return out
    dy = np.asarray(dy, dtype=dtype)
    if stats is not None:
        stats = np.asarray(stats, dtype=dtype)
        rstd = stats[:, 1:2]
        xh = (z - stats[:, 0:1]) * rstd
        out["xhat_bwd"], out["rstd_bwd"] = xh, rstd[:, 0]
    g = dy * gamma
    m1 = g.mean(axis=1, keepdims=True, dtype=dtype)
    m2 = (g * xh).mean(axis=1, keepdims=True, dtype=dtype)
    out["dres"] = (rstd * (g - m1 - xh * m2)).astype(dtype)
    out["dgamma"] = (dy * xh).sum(axis=0, dtype=dtype)
    out["dbeta"] = dy.sum(axis=0, dtype=dtype)
    return out


def add_layernorm_gates(x, a, gamma, beta, dy, eps=EPS, stats=None):
    x, a, gamma, beta, dy = (np.asarray(v, dtype=np.float64) for v in (x, a, gamma, beta, dy))
    rows, C = x.shape
    r = add_layernorm(x, a, gamma, beta, dy, eps)
    z, xh, rstd = r["z"], r["xhat"], r["rstd"][:, None]
    az = np.abs(z)
    M = az.mean(axis=1, keepdims=True)
    X = rstd * (az + M)
    d = np.abs(z - r["mean"][:, None])
    k = (C + 8) * U
    g = np.abs(dy * gamma)
    y = k * (np.abs(gamma) * (X + np.abs(xh) * rstd ** 2 * (d * (az + M)).mean(axis=1, keepdims=True)) + np.abs(beta))
    if stats is not None:       # the backward's own rstd (its mean enters only through the absolute-value form |z| + M)
        rstd = np.asarray(stats, dtype=np.float64)[:, 1:2]
        X = rstd * (az + M)
    return dict(y=y, dres=k * rstd * (g + g.mean(axis=1, keepdims=True) + X * (g * X).mean(axis=1, keepdims=True)),
                dgamma=(rows + 8) * U * (np.abs(dy) * X).sum(axis=0), dbeta=(rows + 8) * U * np.abs(dy).sum(axis=0))


def head(x, W, B, t, H, pos_encoding=True, dh_out=None, mutant=None):
    """The whole head in float64.  x (B*t, C) mel-mean rows; W: dict in_proj_weight (3C, C), in_proj_bias, out_proj.weight (C, C),
    out_proj.bias, norm.weight, norm.bias.  dh_out (B*t, C): the gradient of h -> also dx and every parameter gradient."""
    x = np.asarray(x, dtype=np.float64)
    W = {n: np.asarray(v, dtype=np.float64) for n, v in W.items()}
    R, C = x.shape
    dh = C // H
    xp = x + np.tile(positional_table(t, C), (B, 1)) if pos_encoding else x
    qkv = xp @ W["in_proj_weight"].T + W["in_proj_bias"]
    q, k, v = split_qkv(qkv, B, t, H, dh)
    c = core(q, k, v)
    ctx = c["ctx"].reshape(R, C)
    a = ctx @ W["out_proj.weight"].T + W["out_proj.bias"]
    ln = add_layernorm(xp, a, W["norm.weight"], W["norm.bias"])
    out = dict(h=ln["y"], xp=xp, qkv=qkv, ctx=ctx, a=a, lse=c["lse"], mean=ln["mean"], rstd=ln["rstd"])
    if dh_out is None:
        return out
    lb = add_layernorm(xp, a, W["norm.weight"], W["norm.bias"], dh_out)
    dres = lb["dres"]
    out["d_norm.weight"], out["d_norm.bias"] = lb["dgamma"], lb["dbeta"]
    out["d_out_proj.weight"], out["d_out_proj.bias"] = dres.T @ ctx, dres.sum(axis=0)
    dctx = dres @ W["out_proj.weight"]
    cb = core(q, k, v, dctx.reshape(B, t, H, dh))
    dqkv = join_qkv(cb["dq"], cb["dk"], cb["dv"])
    out["d_in_proj_weight"], out["d_in_proj_bias"] = dqkv.T @ xp, dqkv.sum(axis=0)
    out["dx"] = dqkv @ W["in_proj_weight"] + (0.0 if mutant == "no_residual" else dres)
    out["dres"], out["dctx"], out["dqkv"] = dres, dctx, dqkv
    return out


def check(got, ref, gate, tag):
    """per element |got - ref| <= gate; prints the worst error / gate; -> (ok, worst)"""
    got, ref, gate = (np.asarray(a, dtype=np.float64) for a in (got, ref, gate))
    assert got.shape == ref.shape == gate.shape, (tag, got.shape, ref.shape, gate.shape)
    if not np.isfinite(got).all():
        print(f"{tag}: an element is NaN/inf")
        return False, float("inf")
    err = np.abs(got - ref)
    worst = float((err / np.where(gate > 0, gate, 1.0)).max()) if err.size else 0.0
    print(f"{tag}: worst error / gate {worst:.3f}")
    return bool((err <= gate).all()), worst
