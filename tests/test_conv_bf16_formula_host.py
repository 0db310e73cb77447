"""CPU: tests/conv_bf16_formula.py against torch (conv2d, autograd, batch_norm in float64), the exact family's < 2^24 conditions for
every listed shape, the random family's either-branch share, and mutation checks: each mutant is applied to a copy of the reference
output and fed to the gate functions the GPU module (tests/test_gpu_conv_bf16_exact_oracle.py) uses.

What the gates reject.  The exact gates reject every mutant.  The random gates reject every mutant but one kind: a single stored value
rounded toward zero instead of to nearest-even passes where truncation and nearest agree (the value's nearest bf16 neighbour is the
lower one) or where the truncation error exceeds half an ulp by less than the accumulator's gate C*S -- a half-ulp gate cannot tell
those from a correct store; the exact family pins the store there.  Truncating the WHOLE tensor is rejected by the random gate (a
third of the elements miss it), and so is a single element whose truncation error is over the bound.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_bf16_formula as Fm

F64 = torch.float64
MUT = (2, 6, 8, 256, 32)              # mutation shape: two images (halo), 2304 products per output (|z| > 256 occurs: the rounding mutant)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- the references against torch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Ci,Co", [(2, 5, 4, 3, 5), (1, 1, 6, 4, 2), (2, 3, 1, 5, 3), (1, 1, 1, 2, 2), (2, 4, 6, 20, 17)])
def test_conv_references_match_conv2d_and_autograd(B, H, W, Ci, Co):
    g = torch.Generator().manual_seed(B + 10 * H + 100 * W)
    Cip, Cop = 32, 32                                                        # padded channels: zeros that must change nothing
    a = torch.zeros(B, H, W, Cip, dtype=F64)
    a[..., :Ci] = torch.randn(B, H, W, Ci, generator=g, dtype=F64)
    w = torch.zeros(Cop, Cip, 3, 3, dtype=F64)
    w[:Co, :Ci] = torch.randn(Co, Ci, 3, 3, generator=g, dtype=F64)
    dz = torch.zeros(B, H, W, Cop, dtype=F64)
    dz[..., :Co] = torch.randn(B, H, W, Co, generator=g, dtype=F64)
    at, wt = nchw(a[..., :Ci]).requires_grad_(), w[:Co, :Ci].clone().requires_grad_()
    zt = F.conv2d(at, wt, padding=1)
    ga, gw = torch.autograd.grad(zt, (at, wt), nchw(dz[..., :Co]))
    z = Fm.conv_ref(a, w)
    assert torch.allclose(z[..., :Co], nhwc(zt.detach()), rtol=1e-12, atol=1e-12) and bool((z[..., Co:] == 0).all())
    da = Fm.conv_ref(dz, Fm.dgrad_w(w))
    assert torch.allclose(da[..., :Ci], nhwc(ga), rtol=1e-12, atol=1e-12) and bool((da[..., Ci:] == 0).all())
    dw = Fm.wgrad_ref(a, dz)
    assert torch.allclose(dw[:Co, :Ci], gw, rtol=1e-12, atol=1e-12) and bool((dw[Co:] == 0).all()) and bool((dw[:, Ci:] == 0).all())
    packed = Fm.to_pack_layout(dw[:Co, :Ci], Cip, Cop)
    assert torch.equal(packed.view(3, 3, Cip, Cop)[:, :, :Ci, :Co].permute(3, 2, 0, 1), dw[:Co, :Ci])
    tot = sum(Fm.pixel_dw(a, dz, b, h, x) for b in range(B) for h in range(H) for x in range(W))
    assert torch.allclose(tot, dw, rtol=1e-12, atol=1e-12)                  # the per-pixel contributions the large mutant is built from


@pytest.mark.parametrize("B,H,W,Cc,pool", [(2, 5, 4, 3, 2), (2, 4, 6, 4, 2), (1, 1, 2, 3, 2), (2, 3, 1, 2, 1), (2, 1, 1, 2, 1), (2, 7, 8, 5, 1)])
def test_dz_reference_matches_autograd_of_bn_relu_avgpool(B, H, W, Cc, pool):
    """z -> batch_norm (training) -> relu -> avg_pool -> <., dy>: autograd's dL/dz against dz_ref with the BN-backward coefficients
    ca = gamma*invstd, cb = -gamma*invstd^2 * Q/N, cc = -gamma*invstd*S/N + gamma*invstd^2*mean*Q/N (S = sum g, Q = sum g*xhat)"""
    g = torch.Generator().manual_seed(B + 10 * H + 100 * W + pool)
    z = torch.randn(B, H, W, Cc, generator=g, dtype=F64)
    gamma, beta = torch.rand(Cc, generator=g, dtype=F64) + 0.5, torch.randn(Cc, generator=g, dtype=F64) * 0.3
    gamma[0] = -gamma[0]
    dy = torch.randn(B, H // pool, W // pool, Cc, generator=g, dtype=F64)
    zt = nchw(z).requires_grad_()
    act = torch.relu(F.batch_norm(zt, None, None, gamma, beta, training=True, eps=1e-5))
    y = act if pool == 1 else (F.avg_pool2d(act, pool) if dy.numel() else act[:, :, :0])      # H = 1 under pool 2: an empty pooled tensor
    if y.numel():
        (gz,) = torch.autograd.grad(y, zt, nchw(dy))
    else:
        gz = torch.zeros_like(zt)
    n = B * H * W
    mean = z.mean(dim=(0, 1, 2))
    invstd = 1.0 / torch.sqrt(z.var(dim=(0, 1, 2), unbiased=False) + 1e-5)
    sc, sh = gamma * invstd, beta - mean * gamma * invstd
    if y.numel():
        assert torch.allclose(nhwc(y.detach()), Fm.avgpool_fwd(Fm.bn_relu(z, sc, sh), pool), rtol=1e-12, atol=1e-12)
    gfull, _ = Fm.dz_ref(dy, z, torch.ones(Cc), torch.zeros(Cc), torch.zeros(Cc), pool, sc, sh)       # the ReLU / pool backward alone
    xhat = (z - mean) * invstd
    S, Q = gfull.sum(dim=(0, 1, 2)), (gfull * xhat).sum(dim=(0, 1, 2))
    ca = gamma * invstd
    cb = -gamma * invstd * invstd * Q / n
    cc = -gamma * invstd * S / n + gamma * invstd * invstd * mean * Q / n
    dz, M = Fm.dz_ref(dy, z, ca, cb, cc, pool, sc, sh)
    assert torch.allclose(dz, nhwc(gz), rtol=1e-9, atol=1e-11)
    assert bool((M >= dz.abs() - 1e-12).all())
    # BN backward alone (dz mode BN: g given at full resolution)
    gfull_t = torch.randn(B, H, W, Cc, generator=g, dtype=F64)
    zt2 = nchw(z).requires_grad_()
    (gz2,) = torch.autograd.grad(F.batch_norm(zt2, None, None, gamma, beta, training=True, eps=1e-5), zt2, nchw(gfull_t))
    S2, Q2 = gfull_t.sum(dim=(0, 1, 2)), (gfull_t * xhat).sum(dim=(0, 1, 2))
    dz2, _ = Fm.dz_ref(gfull_t, z, ca, -gamma * invstd * invstd * Q2 / n, -gamma * invstd * S2 / n + gamma * invstd * invstd * mean * Q2 / n)
    assert torch.allclose(dz2, nhwc(gz2), rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("B,H", [(1, 1), (2, 5)])
@pytest.mark.parametrize("family", ["exact", "random"])
def test_c1_activation_restatement(B, H, family):
    """the restated block-0 activation against conv2d on the operands as the kernel rounds them; exact family: no rounding anywhere"""
    o = Fm.draw_c1(B, H, family)
    a1, pre, S, xz = Fm.c1_activation(o["x1"], o["fmean"], o["fstd"], o["w1"], o["sc1"], o["sh1"])
    xz32 = ((o["x1"] - o["fmean"]) * (1.0 / o["fstd"]))
    wf = (o["w1"] * o["sc1"][:, None, None, None]).to(Fm.BF).to(F64)
    hi = o["sh1"].to(Fm.BF).to(F64)
    lo = (o["sh1"].to(F64) - hi).to(torch.float32).to(Fm.BF).to(F64)
    ref = F.conv2d(xz32.to(Fm.BF).to(F64)[:, None], wf, padding=1) + (hi + lo)[None, :, None, None]
    assert torch.allclose(pre, nhwc(ref), rtol=1e-12, atol=1e-12)
    assert torch.equal(a1, Fm.rne(torch.relu(pre))) and bool((S >= pre.abs() - 1e-12).all())
    if family == "exact":
        exact = F.conv2d((o["x1"] / o["fstd"]).to(F64)[:, None], (o["w1"] * o["sc1"][:, None, None, None]).to(F64), padding=1)
        assert torch.equal(pre, nhwc(exact) + o["sh1"].to(F64))             # the bf16 roundings and the hi + lo split lose nothing
        assert torch.equal(a1, torch.relu(pre)) and float(pre.abs().max()) <= Fm.exact_bounds_c1(B, H)["pre"]
    g = torch.randn(B, H, 64, 32, dtype=F64, generator=torch.Generator().manual_seed(1))
    rows = Fm.c1_a_rows(g, xz)
    dwc1 = Fm.wgrad_ref(xz[..., None], g)                                    # [32][1][3][3]: the Cin = 1 weight gradient
    assert torch.allclose(rows[:9].t().reshape(32, 1, 3, 3), dwc1, rtol=1e-12, atol=1e-12)
    assert torch.allclose(rows[9], g.sum(dim=(0, 1, 2)))


def test_bf16_helpers():
    v = torch.tensor([257.0, 258.0, 259.0, 261.0, -257.0, -259.0, 1.0, 0.3, 1.00390625, 1.01171875], dtype=F64)
    assert Fm.rne(v).tolist()[:6] == [256.0, 258.0, 260.0, 260.0, -256.0, -260.0]          # ties to even, both signs
    assert Fm.rtz(v).tolist()[:6] == [256.0, 258.0, 258.0, 260.0, -256.0, -258.0]
    assert Fm.ulp_bf16(v).tolist()[:3] == [2.0, 2.0, 2.0] and float(Fm.ulp_bf16(v)[6]) == 2.0 ** -7
    assert Fm.boundary_distance(torch.tensor([257.0, 259.0, 258.0, 1.00390625], dtype=F64)).tolist() == [0.0, 0.0, 1.0, 0.0]
    v = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20, 1.75 + 2.0 ** -8 - 2.0 ** -20], dtype=F64)    # just under a rounding boundary
    assert Fm.rne(v).tolist() == [1.0, 1.75] and bool(Fm.within(Fm.rne(v), v, Fm.half_ulp(v)).all())
    assert bool(((Fm.rne(v) - v).abs() > 2.0 ** -9 * v).all())             # correct stores that a flat 2^-9 * |v| would reject
    assert Fm.half_ulp(v).tolist() == [2.0 ** -8, 2.0 ** -8]
    assert Fm.flip_mask(torch.tensor([257.0 + 1e-6, 258.0], dtype=F64), torch.tensor([1e-5, 1e-5], dtype=F64)).tolist() == [True, False]


FUSED_SHAPES = ([(B, H, W, Ci, Co) for (W, Ci, Co) in Fm.GEOM_C1 for (B, H, _) in Fm.FUSED_CASES]
                + [(B, H, W, Cc, Cc) for (W, Cc, _, _) in Fm.GEOM_C2 for (B, H, _) in Fm.FUSED_CASES])
POOL_LAYERS = [(B, H, W, Cc, Cd) for (B, H, W, Cd, Cc) in Fm.POOLSTATS_SHAPES]       # as the GPU module draws them: the layer C -> Cd


# ---- the exact family's conditions and the random family's either-branch share ------------------------------------------------------
@pytest.mark.parametrize("shape", Fm.WGRAD_SHAPES + FUSED_SHAPES + Fm.ANYW_SHAPES + Fm.COL_SHAPES + POOL_LAYERS)
def test_exact_ok_for_every_conv_shape(shape):
    b = Fm.exact_bounds_conv(shape)
    assert Fm.exact_ok(*b.values()), (shape, b)


@pytest.mark.parametrize("B,H", Fm.BLOCK0)
def test_exact_ok_for_block0(B, H):
    b = Fm.exact_bounds_c1(B, H)
    assert Fm.exact_ok(*b.values()), (B, H, b)


def test_exact_family_is_dense_and_within_its_stated_magnitudes():
    o = Fm.draw_conv((2, 13, 16, 20, 17), "exact")
    for k in ("x", "dz", "zref", "z", "g"):
        t = o[k]
        Cn = 20 if k in ("x", "zref") else 17
        assert bool((t[..., Cn:] == 0).all()) and float(t.abs().max()) == 2 and bool((t == t.round()).all())
        assert float((t[..., :Cn] != 0).double().mean()) > 0.7              # not sparse
    assert bool((o["g2"] % 4 == 0).all()) and float((o["w"] != 0).double().mean()) > 0.7
    assert bool((o["w"] != 0).flatten(2).any(0).any(0).all())               # every tap carries weight
    assert set(o["sc_i"][:20].tolist()) <= {1.0, 2.0} and set(o["invstd_i"][:20].tolist()) <= {0.5, 1.0, 2.0}
    a = Fm.bn_relu(o["x"], o["sc_i"], o["sh_i"])
    dz, M = Fm.dz_ref(o["g2"], o["z"], o["ca"], o["cb"], o["cc"], 2, o["sc_o"], o["sh_o"])
    assert float(a.abs().max()) <= 6 and float(dz.abs().max()) <= 10 and bool((dz == dz.round()).all())


@pytest.mark.parametrize("shape", POOL_LAYERS)
def test_either_branch_share_of_the_pooled_activations(shape):
    o = Fm.draw_conv(shape, "random")
    z = Fm.draw_pool_z(shape, "random")
    assert z.shape[1] == 2 * shape[1] + 1 and float(Fm.relu_either(z, o["sc_i"], o["sh_i"]).double().mean()) <= Fm.EITHER_SHARE
    ze = Fm.draw_pool_z(shape, "exact")
    assert float(ze.abs().max()) == 2 and bool((ze == ze.round()).all())


@pytest.mark.parametrize("shape", Fm.WGRAD_SHAPES + Fm.ANYW_SHAPES + Fm.COL_SHAPES + FUSED_SHAPES)
def test_either_branch_share_of_the_random_cases(shape):
    """the share of elements whose fp32 ReLU decision float64 cannot settle, for the seeds the GPU module uses"""
    o = Fm.draw_conv(shape, "random")
    Ci, Co = shape[3], shape[4]
    for z, es, et, Cn in ((o["zref"], o["sc_i"], o["sh_i"], Ci), (o["z"], o["sc_o"], o["sh_o"], Co), (o["x"], o["sc_i"], o["sh_i"], Ci)):
        share = float(Fm.relu_either(z[..., :Cn], es[:Cn], et[:Cn]).double().mean())
        assert share <= Fm.EITHER_SHARE, (shape, share)


@pytest.mark.parametrize("B,H", Fm.BLOCK0)
def test_either_branch_share_of_block0(B, H):
    o = Fm.draw_c1(B, H, "random")
    _, pre, S, _ = Fm.c1_activation(o["x1"], o["fmean"], o["fstd"], o["w1"], o["sc1"], o["sh1"])
    assert float((pre.abs() <= Fm.C * S).double().mean()) <= Fm.EITHER_SHARE       # conv1's ReLU: the accumulator's own gate
    assert float(Fm.relu_either(o["z2"], o["sc2"], o["sh2"]).double().mean()) <= Fm.EITHER_SHARE


# ---- mutation checks ---------------------------------------------------------------------------------------------------------
def _fwd_case(family):
    o = Fm.draw_conv(MUT, family)
    a, w = o["x"].to(F64), o["w"].to(F64)
    z, S = Fm.conv_ref(a, w), Fm.conv_ref(a.abs(), w.abs())
    return o, a, w, z, S


def _fwd_gate(family, mut, z, S):
    """the stored bf16 output `mut` (a float64 accumulator value, stored with the correct rounding) against the family's gate"""
    got = Fm.rne(mut)
    return Fm.eq_bf16(got, z) if family == "exact" else Fm.within(got, z, Fm.bound_bf16(z, S))


@pytest.mark.parametrize("family", ["exact", "random"])
def test_forward_mutants_are_rejected(family):
    o, a, w, z, S = _fwd_case(family)
    assert family != "exact" or Fm.exact_ok(float(S.max()))
    assert bool(_fwd_gate(family, z, z, S).all())                            # the unmutated output passes
    m1 = Fm.mutant_corner_product(z, a, w)
    assert float((m1 - z).abs().max()) > 0 and not bool(_fwd_gate(family, m1, z, S).all()), "corner product"
    m2 = z.clone()
    m2[1, 0] += Fm.mutant_halo_row(a, w)
    assert not bool(_fwd_gate(family, m2, z, S).all()), "halo row from the neighbouring image"
    full = Fm.conv_ref(a.reshape(1, 12, 8, 256), w)                          # cross-check: the two images stacked share that halo
    assert torch.allclose(m2[1, 0], full[0, 6], rtol=1e-12, atol=1e-12)
    m3 = Fm.mutant_tap_zeroed(z, a, w)
    assert not bool(_fwd_gate(family, m3, z, S)[..., 0].all()) and bool(_fwd_gate(family, m3, z, S)[..., 1:].all()), "tap zeroed"
    row, mags = z.sum(dim=(0, 1, 2)), z.abs().sum(dim=(0, 1, 2))
    m4 = Fm.mutant_stat_missing_pixel(row, z, 1, 5, 7)
    if family == "exact":
        assert Fm.exact_ok(float(mags.max())) and not bool(Fm.eq_f32(m4, row).all()), "statistics row missing a pixel"
    else:
        bound = Fm.sum_bound(Fm.bound_bf16(z, S), z.abs())
        assert bool(Fm.within(Fm.rne(z).sum(dim=(0, 1, 2)), row, bound).all())
        assert not bool(Fm.within(m4, row, bound).all()), "statistics row missing a pixel"


def test_rounding_mutant_exact_family():
    """a stored value rounded toward zero: rejected wherever truncation and nearest-even differ (here: odd integers above 256)"""
    o, a, w, z, S = _fwd_case("exact")
    differs = Fm.rtz(z) != Fm.rne(z)
    assert int(differs.sum()) >= 1 and float(z.abs().max()) > 256
    idx = tuple(differs.nonzero()[0].tolist())
    got = Fm.rne(z)
    got[idx] = Fm.rtz(z)[idx]
    ok = Fm.eq_bf16(got, z)
    assert not bool(ok[idx]) and int((~ok).sum()) == 1
    ties = (z.abs() > 256) & (z.abs() < 512) & (z % 2 == 1)                  # odd integers in (256, 512) lie midway between two bf16 values
    assert int(ties.sum()) >= 1 and bool(Fm.eq_bf16(Fm.rne(z), z).all())
    other = torch.where(ties, 2.0 * z - Fm.rne(z), Fm.rne(z))                # a tie sent to its other neighbour (odd last mantissa bit)
    assert bool((other[ties] % 4 == 2).all()) and int((~Fm.eq_bf16(other, z)).sum()) == int(ties.sum())


def test_rounding_mutant_random_family():
    o, a, w, z, S = _fwd_case("random")
    bound = Fm.bound_bf16(z, S)
    whole = Fm.within(Fm.rtz(z), z, bound)
    assert float((~whole).double().mean()) > 0.2                             # the whole tensor truncated: rejected
    err = (Fm.rtz(z) - z).abs()
    over = err > bound
    idx = tuple(over.nonzero()[0].tolist())
    got = Fm.rne(z)
    got[idx] = Fm.rtz(z)[idx]
    assert not bool(Fm.within(got, z, bound)[idx])                           # one element truncated by more than the bound: rejected
    same = Fm.rtz(z) == Fm.rne(z)
    assert bool(same.any()) and bool(Fm.within(Fm.rtz(z), z, bound)[same].all())     # truncation = nearest: indistinguishable, passes


@pytest.mark.parametrize("family", ["exact", "random"])
def test_weight_gradient_mutants_are_rejected(family):
    o = Fm.draw_conv(MUT, family)
    a = Fm.rne(Fm.bn_relu(o["x"], o["sc_i"], o["sh_i"]))
    dz = Fm.rne(Fm.dz_ref(o["g"], o["z"], o["ca"], o["cb"], o["cc"])[0])
    dw, S = Fm.wgrad_ref(a, dz), Fm.wgrad_ref(a.abs(), dz.abs())
    gate = (lambda got: Fm.eq_f32(got, dw)) if family == "exact" else (lambda got: Fm.within(got, dw, Fm.bound_f32(S)))
    assert family != "exact" or Fm.exact_ok(float(S.max()))
    assert bool(gate(dw).all())
    twice = Fm.mutant_strip_pixel_twice(dw, a, dz, 0, 3)
    assert not bool(gate(twice).all()), "last pixel of a strip counted twice"
    dropped = dw - Fm.pixel_dw(a, dz, 1, 0, 0)
    assert not bool(gate(dropped).all()), "pixel dropped at an image corner"
    halo = dw.clone()                                                        # image 1's top halo row read from image 0's last row
    ap = F.pad(a[0, -1], (0, 0, 1, 1))                                       # [W + 2][Ci]
    for j in range(3):
        halo[:, :, 0, j] += dz[1, 0].t() @ ap[j:j + a.shape[2]]
    assert not bool(gate(halo).all()), "halo row from the neighbouring image"


@pytest.mark.parametrize("family", ["exact", "random"])
def test_weight_gradient_mutant_at_the_bench_grid_size(family):
    """(300, 20, 16, 128, 128): 96000 pixels per dW entry, where the max-norm gate of the older tests lets a dropped pixel pass.  The
    mutated dW is the reference +- one pixel's contribution, so only that contribution and the gate's bound are needed: exact
    family -- any non-zero change of an integer below 2^24 changes the fp32 value; random family -- |delta| against C*S with S
    bounded ABOVE by Cauchy-Schwarz, S[o][c][tap] <= ||a[..c]||_2 * ||dz[..o]||_2 (a rejection under the larger bound is one under S)."""
    shape = (300, 20, 16, 128, 128)
    o = Fm.draw_conv(shape, family)
    a, dz = o["x"].to(F64), o["dz"].to(F64)
    delta = Fm.pixel_dw(a, dz, 299, 19, 15)                                  # the last pixel of the last strip
    inner = Fm.pixel_dw(a, dz, 150, 3, 15)                                   # the last pixel of a row inside the batch
    if family == "exact":
        assert Fm.exact_ok(Fm.exact_bounds_conv(shape)["wgrad"])
        assert float(delta.abs().max()) >= 1 and float(inner.abs().max()) >= 1      # ref + delta != ref in fp32 below 2^24
    else:
        s_up = torch.outer(dz.reshape(-1, 128).norm(dim=0), a.reshape(-1, 128).norm(dim=0))[:, :, None, None]
        for d in (delta, inner):
            assert bool((d.abs() > Fm.C * s_up).any()), "the per-element gate lets a dropped pixel pass"
