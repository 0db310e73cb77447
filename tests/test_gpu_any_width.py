"""Width-general 3x3 convolution kernels (csrc/sed_conv_anyw.hip) and models declared with a mel-bin count outside the specialised
widths (Cnn_AvgPooling / Crnn_AvgPooling(..., mel_bins=F)).  Needs the MI355X:  pytest -m gpu.

Kernel level: operands through the C ABI, expected results from oracle/cnn_oracle.py's float64 formulas on the same (bf16-rounded
where the kernel stores bf16) values -- the style and gates of tests/test_gpu_kernels_oracle.py.
Model level: train steps against oracle/cnn_oracle.py (fp32, f16x3), oracle/cnn_oracle_bf16.py (bf16) and oracle/crnn_oracle.py."""
import importlib

import pytest
import torch

from oracle import cnn_oracle as O
from oracle import cnn_oracle_bf16 as OB
from oracle import crnn_oracle as RO

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
BF = torch.bfloat16
F64 = torch.float64
MAIN_CFG = [(32, 2), (64, 2), (128, 2), (128, 1)]
WIDTHS = [1, 3, 5, 12, 40, 48, 100, 128, 200, 256]
CHANNELS = [(32, 32), (64, 128), (128, 64), (32, 64), (128, 128), (64, 32)]     # (Cin, Cout), cycled over the widths
DTYPES = ["bf16", "fp32"]


@pytest.fixture(scope="module")
def sed():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def L(sed):
    return sed._lib


def st():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def shape_of(W, i):
    """B, H for width W: a few thousand pixels, heights that leave a partial last tile"""
    H = max(3, min(37, 3000 // (2 * W)) | 1)
    return 2, H


def rnd(dt, t):
    """the values the kernel sees, in float64"""
    return t.to(BF).to(F64) if dt == "bf16" else t.to(F64)


def dev(dt, t_nchw):
    """float64 NCHW -> device NHWC in the storage dtype"""
    return t_nchw.permute(0, 2, 3, 1).contiguous().to(BF if dt == "bf16" else torch.float32).cuda()


def host(t_nhwc):
    return t_nhwc.detach().to(F64).cpu().permute(0, 3, 1, 2).contiguous()


def cv(v):
    return v.to(F64)[None, :, None, None]


def assert_close(dt, got, ref, what):
    """stored tensors: 2 bf16 ulps (+ accumulation noise near 0) in bf16, 1e-4 of the tensor's scale in fp32"""
    scale = max(ref.abs().max().item(), 1e-6)
    if dt == "bf16":
        tol = 2.0 ** -7 * torch.maximum(got.abs(), ref.abs()) + 2e-3 * scale
    else:
        tol = 1e-5 * ref.abs() + 1e-4 * scale
    bad = ((got - ref).abs() > tol).double().mean().item()
    assert bad == 0.0, f"{what}: {100 * bad:.4f}% of the elements off (max |err| {(got - ref).abs().max().item():.3e}, scale {scale:.3e})"


def assert_sums(dt, got, ref, what, quantum):
    """fp32 sums: relative 2e-3 (bf16: plus a few bf16 roundings that went the other way) / 1e-4 (fp32) of the scale"""
    scale = max(ref.abs().max().item(), 1e-6)
    tol = (2e-3 * ref.abs() + 2e-3 * scale + 4 * quantum) if dt == "bf16" else (1e-5 * ref.abs() + 1e-4 * scale)
    err = (got.to(F64).cpu() - ref).abs()
    assert bool((err <= tol).all()), f"{what}: max |err| {err.max().item():.3e} (scale {scale:.3e})"


def pack(L, dt, w, transpose):
    Cout, Cin = w.shape[:2]
    out = torch.empty(9 * Cin * Cout, dtype=BF if dt == "bf16" else torch.float32, device="cuda")
    wd = w.float().contiguous().cuda()
    L.check(L.lib().sed_pack_conv_weight(L.SED_BF16 if dt == "bf16" else L.SED_F32, ptr(wd), ptr(out), Cout, Cin, Cout, Cin,
                                         1 if transpose else 0, st()), "pack")
    return out


def make_layer(dt, B, H, W, Cin, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = rnd(dt, torch.randn(B, Cin, H, W, generator=g))
    w = rnd(dt, torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5))
    sc = (0.5 + torch.rand(Cin, generator=g)).to(F64)
    sh = (0.3 * torch.randn(Cin, generator=g)).to(F64)
    return g, x, w, sc, sh


def fwd_call(L, entry, dt, pro, epi, x, ps, ph, wpack, z, zref, es, et, em, ei, part, B, H, W, Cinp, Coutp):
    fn = getattr(L.lib(), entry)
    L.check(fn(L.SED_BF16 if dt == "bf16" else L.SED_F32, pro, epi, ptr(x), ptr(ps), ptr(ph), ptr(wpack), ptr(z), ptr(zref), ptr(es),
               ptr(et), ptr(em), ptr(ei), ptr(part), B, H, W, Cinp, Coutp, st()), entry)


# ---------------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------------
def check_forward(L, entry, dt, W, Cin, Cout, seed):
    B, H = shape_of(W, seed)
    g, x, w, sc, sh = make_layer(dt, B, H, W, Cin, Cout, seed)
    xd, wp = dev(dt, x), pack(L, dt, w, False)
    scd, shd = sc.float().cuda(), sh.float().cuda()
    nparts = L.lib().sed_conv_nparts(B, H, W)
    for pro in (L.PRO_NONE, L.PRO_BNRELU):
        a = x if pro == L.PRO_NONE else rnd(dt, torch.relu(x * cv(sc) + cv(sh)))
        ref = O.conv3x3_fwd(a, w)
        for epi in (L.EPI_STORE, L.EPI_STATS):
            z = torch.full((B, H, W, Cout), float("nan"), dtype=xd.dtype, device="cuda")
            part = torch.full((nparts, 2, Cout), float("nan"), device="cuda")
            fwd_call(L, entry, dt, pro, epi, xd, scd if pro else None, shd if pro else None, wp, z, None, None, None, None, None,
                     part if epi == L.EPI_STATS else None, B, H, W, Cin, Cout)
            torch.cuda.synchronize()
            assert_close(dt, host(z), rnd(dt, ref), f"{entry} W{W} {Cin}->{Cout} pro{pro} epi{epi}")
            if epi == L.EPI_STATS:      # statistics from the fp32 accumulator: every one of the W columns counts
                s = part.double().cpu().sum(0)
                q = 2.0 ** -8 * ref.abs().max().item()
                assert_sums(dt, s[0], ref.sum((0, 2, 3)), f"sum z W{W}", q * B * H * W ** 0.5)
                assert_sums(dt, s[1], (ref * ref).sum((0, 2, 3)), f"sum z^2 W{W}", q * ref.abs().max().item() * B * H * W ** 0.5)
    # data gradient: conv^T(dz) gated by the ReLU of BN1(zref) + BN1 backward sums (SED_EPI_RELUBWD), operator packed transposed
    dz = rnd(dt, torch.randn(B, Cout, H, W, generator=g))
    zr = rnd(dt, torch.randn(B, Cin, H, W, generator=g))
    es, et = sc.clone(), sh.clone()
    em = (0.1 * torch.randn(Cin, generator=g)).to(F64)
    ei = (0.5 + torch.rand(Cin, generator=g)).to(F64)
    wpt = pack(L, dt, w, True)
    gout = torch.empty((B, H, W, Cin), dtype=xd.dtype, device="cuda")
    part = torch.full((nparts, 2, Cin), float("nan"), device="cuda")
    fwd_call(L, entry, dt, L.PRO_NONE, L.EPI_RELUBWD, dev(dt, dz), None, None, wpt, gout, dev(dt, zr), es.float().cuda(),
             et.float().cuda(), em.float().cuda(), ei.float().cuda(), part, B, H, W, Cout, Cin)
    torch.cuda.synchronize()
    gref = O.conv3x3_dgrad(dz, w) * ((zr * cv(es) + cv(et)) > 0)
    assert_close(dt, host(gout), rnd(dt, gref), f"{entry} dgrad W{W} {Cout}->{Cin}")
    s = part.double().cpu().sum(0)
    q = 2.0 ** -8 * gref.abs().max().item() * B * H * W ** 0.5
    assert_sums(dt, s[0], gref.sum((0, 2, 3)), f"sum g W{W}", q)
    assert_sums(dt, s[1], (gref * (zr - cv(em)) * cv(ei)).sum((0, 2, 3)), f"sum g*xhat W{W}", 4 * q)


def run_wgrad(L, entry_kind, dt, pro, dzmode, x, sc, sh, dz_or_g, z, coef, pool, B, H, W, Cin, Cout):
    lib = L.lib()
    ws = torch.empty(lib.sed_conv_wgrad_ws_floats(B, H, W, Cin, Cout), device="cuda")
    dwp = torch.full((9 * Cin * Cout,), float("nan"), device="cuda")
    dtc = L.SED_BF16 if dt == "bf16" else L.SED_F32
    ps = sc.float().cuda() if pro else None
    ph = sh.float().cuda() if pro else None
    dz_out = None
    if dzmode == 0:
        fn = lib.sed_conv3x3_wgrad_anyw if entry_kind == "anyw" else lib.sed_conv3x3_wgrad
        L.check(fn(dtc, pro, ptr(x), ptr(ps), ptr(ph), ptr(dz_or_g), ptr(dwp), ptr(ws), B, H, W, Cin, Cout, st()), "wgrad")
    else:
        ca, cb, cc, scz, shz = [c.float().cuda() for c in coef]
        dz_out = torch.full((B, H, W, Cout), float("nan"), dtype=x.dtype, device="cuda")
        L.check(lib.sed_conv3x3_wgrad_fused(dtc, pro, ptr(x), ptr(ps), ptr(ph), dzmode, ptr(dz_or_g), ptr(z), ptr(scz), ptr(shz),
                                            ptr(ca), ptr(cb), ptr(cc), pool, ptr(dz_out), ptr(dwp), ptr(ws), B, H, W, Cin, Cout, st()),
                "wgrad_fused")
    torch.cuda.synchronize()
    return dwp.double().cpu().view(9, Cin, Cout), dz_out


def wref(dW):
    return dW.permute(2, 3, 1, 0).reshape(9, dW.shape[1], dW.shape[0])


def check_wgrad(L, entry_kind, dt, W, Cin, Cout, seed, modes=("given", "pool1", "pool2", "bn")):
    B, H = shape_of(W, seed)
    g, x, w, sc, sh = make_layer(dt, B, H, W, Cin, Cout, seed)
    xd = dev(dt, x)
    for pro in (L.PRO_NONE, L.PRO_BNRELU):
        a = x if pro == L.PRO_NONE else rnd(dt, torch.relu(x * cv(sc) + cv(sh)))
        for mode in modes:
            if mode == "given":
                dz = rnd(dt, torch.randn(B, Cout, H, W, generator=g))
                dW, _ = run_wgrad(L, entry_kind, dt, pro, 0, xd, sc, sh, dev(dt, dz), None, None, 1, B, H, W, Cin, Cout)
            else:
                z = rnd(dt, torch.randn(B, Cout, H, W, generator=g))
                ca, cb, cc = (0.5 + torch.rand(Cout, generator=g)).to(F64), (0.2 * torch.randn(Cout, generator=g)).to(F64), \
                    (0.1 * torch.randn(Cout, generator=g)).to(F64)
                scz, shz = (0.5 + torch.rand(Cout, generator=g)).to(F64), (0.3 * torch.randn(Cout, generator=g)).to(F64)
                if mode == "bn":
                    gin = rnd(dt, torch.randn(B, Cout, H, W, generator=g))
                    dzr = cv(ca) * gin + cv(cb) * z + cv(cc)
                    dzmode, pool = L.DZ_BN, 1
                else:
                    pool = 2 if mode == "pool2" else 1
                    if pool == 2 and (H < 2 or W < 2):
                        continue
                    dy = rnd(dt, torch.randn(B, Cout, H // pool, W // pool, generator=g))
                    up = torch.zeros(B, Cout, H, W, dtype=F64)
                    # avg-pool backward with the floor: rows / columns past 2*(H//2) / 2*(W//2) get no gradient
                    up[:, :, :(H // pool) * pool, :(W // pool) * pool] = dy.repeat_interleave(pool, 2).repeat_interleave(pool, 3) / pool ** 2
                    gin = up * ((z * cv(scz) + cv(shz)) > 0)
                    dzr = cv(ca) * gin + cv(cb) * z + cv(cc)      # (a dropped column still gets cb*z + cc)
                    dzmode = L.DZ_POOL
                coef = (ca, cb, cc, scz, shz)
                dW, dz_out = run_wgrad(L, entry_kind, dt, pro, dzmode, xd, sc, sh, dev(dt, gin if mode == "bn" else dy), dev(dt, z),
                                       coef, pool, B, H, W, Cin, Cout)
                assert_close(dt, host(dz_out), rnd(dt, dzr), f"dz_out W{W} {mode}")
                dz = rnd(dt, dzr)
            ref = wref(O.conv3x3_wgrad(a, dz))
            scale = ref.abs().max().item()
            err = (dW - ref).abs().max().item()
            assert err <= (1e-3 if dt == "bf16" else 1e-4) * scale, f"wgrad W{W} {Cin}->{Cout} pro{pro} {mode}: {err:.3e} of {scale:.3e}"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("i,W", list(enumerate(WIDTHS)))
def test_forward_and_data_gradient_any_width(L, dt, i, W):
    Cin, Cout = CHANNELS[i % len(CHANNELS)]
    check_forward(L, "sed_conv3x3_fwd", dt, W, Cin, Cout, 10 + i)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("i,W", list(enumerate(WIDTHS)))
def test_weight_gradient_any_width(L, dt, i, W):
    Cin, Cout = CHANNELS[(i + 1) % len(CHANNELS)]
    check_wgrad(L, "generic", dt, W, Cin, Cout, 30 + i)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("W", [16, 64])
def test_anyw_entries_at_specialised_widths(L, dt, W):
    check_forward(L, "sed_conv3x3_fwd_anyw", dt, W, 64, 64, 50 + W)
    check_wgrad(L, "anyw", dt, W, 32, 64, 60 + W, modes=("given",))


def test_split_operand_dtypes_refused_at_uncovered_widths(L):
    lib = L.lib()
    B, H, W, C = 1, 4, 40, 32
    x = torch.zeros(B, H, W, C, device="cuda")
    wp = torch.zeros(9 * C * C, dtype=torch.int16, device="cuda")
    z = torch.empty_like(x)
    for dtc in (L.SED_F32X3, L.SED_F32H3):
        rc = lib.sed_conv3x3_fwd(dtc, L.PRO_NONE, L.EPI_STORE, ptr(x), None, None, ptr(wp), ptr(z), None, None, None, None, None,
                                 None, B, H, W, C, C, st())
        assert rc != 0 and b"SED_BF16 and SED_F32" in lib.sed_last_error()
    for Wb in (0, 257):
        rc = lib.sed_conv3x3_fwd(L.SED_F32, L.PRO_NONE, L.EPI_STORE, ptr(x), None, None, ptr(wp), ptr(z), None, None, None, None, None,
                                 None, B, H, Wb, C, C, st())
        assert rc != 0
    # the fused weight gradient at such a width needs dz_out (the library allocates nothing)
    ws = torch.empty(lib.sed_conv_wgrad_ws_floats(B, H, W, C, C), device="cuda")
    v = torch.zeros(C, device="cuda")
    rc = lib.sed_conv3x3_wgrad_fused(L.SED_F32, L.PRO_NONE, ptr(x), None, None, L.DZ_BN, ptr(x), ptr(x), None, None, ptr(v), ptr(v),
                                     ptr(v), 1, None, ptr(ws), ptr(ws), B, H, W, C, C, st())
    assert rc != 0 and b"dz_out" in lib.sed_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("W", [5, 40, 128])
def test_first_layer_kernels_at_any_width(L, dt, W):
    """the Cin = 1 block-0 kernels (run-time W): forward + statistics, weight-gradient partials"""
    lib = L.lib()
    B, H, Cout = 2, 23, 32
    g = torch.Generator().manual_seed(W)
    x = torch.randn(B, H, W, generator=g)
    mean, std = 0.1 * torch.randn(W, generator=g), 0.5 + torch.rand(W, generator=g)
    w = torch.randn(Cout, 1, 3, 3, generator=g) / 3.0
    xn = ((x.to(F64) - mean.to(F64)) / std.to(F64))[:, None]
    ref = O.conv3x3_fwd(xn, w.to(F64))
    nparts = lib.sed_conv_c1_nparts(B, H, W)
    z = torch.empty(B, H, W, Cout, dtype=BF if dt == "bf16" else torch.float32, device="cuda")
    part = torch.empty(nparts, 2, Cout, device="cuda")
    dtc = L.SED_BF16 if dt == "bf16" else L.SED_F32
    xd, md, sd, wd = x.cuda(), mean.cuda(), std.cuda(), w.cuda().contiguous()
    L.check(lib.sed_conv3x3_c1_fwd(dtc, ptr(xd), ptr(md), ptr(sd), ptr(wd), ptr(z), ptr(part), B, H, W, Cout, Cout, st()), "c1_fwd")
    torch.cuda.synchronize()
    tol = 2.0 ** -7 if dt == "bf16" else 1e-5
    assert (host(z) - ref).abs().max().item() <= tol * ref.abs().max().item() + 1e-5
    # statistics: the float64 sums of the float64 z and z^2 (the kernel sums its fp32 accumulators in either storage type) under the
    # propagated gates of tests/test_gpu_c1_exact_oracle.py: z's gate gz = 4 (9 + 2) u sum |xp||w| through the sums, plus the thread's
    # chain n_t = ceil(W / PPB) * 8 * ceil(bands / grid) and the PPB = 256 / (Cout / 8) lanes (one more for the fma of z^2)
    assert not bool(torch.isnan(part).any()), "a partial row was not written"
    s = part.double().cpu().sum(0)
    u, ppb = 2.0 ** -24, 256 // (Cout // 8)
    n_t = -(-W // ppb) * 8 * -(-(B * -(-H // 8)) // nparts)
    gz = 4 * 11 * u * O.conv3x3_fwd(xn.abs(), w.to(F64).abs())
    a1, a2 = ref.abs().sum((0, 2, 3)), (ref * ref).sum((0, 2, 3))
    gate1 = gz.sum((0, 2, 3)) + 4 * (n_t + ppb) * u * a1
    gate2 = (2 * ref.abs() * gz + gz * gz).sum((0, 2, 3)) + 4 * (n_t + ppb + 1) * u * a2
    assert bool((gate1 <= 1e-4 * ref.abs().sum().item() / Cout + 1e-3).all())      # (never looser than the bound it replaces)
    assert bool(((s[0] - ref.sum((0, 2, 3))).abs() <= gate1).all()), ((s[0] - ref.sum((0, 2, 3))).abs() / gate1).max().item()
    assert bool(((s[1] - a2).abs() <= gate2).all()), ((s[1] - a2).abs() / gate2).max().item()
    dz = torch.randn(B, Cout, H, W, generator=g).to(F64)
    dz = rnd(dt, dz)
    ws = torch.empty(nparts, 9, Cout, device="cuda")
    L.check(lib.sed_conv3x3_c1_wgrad(dtc, ptr(xd), ptr(md), ptr(sd), ptr(dev(dt, dz)), ptr(ws), B, H, W, Cout, st()), "c1_wgrad")
    torch.cuda.synchronize()
    got = ws.double().cpu().sum(0)                                   # [9][Cout]
    want = O.conv3x3_wgrad(xn, dz)[:, 0].permute(1, 2, 0).reshape(9, Cout)
    assert (got - want).abs().max().item() <= 1e-4 * want.abs().max().item()


# ---------------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------------
def batch(B, T, F, K=1, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, T, F, generator=g)
    y = (torch.rand(B, T, K, generator=g) < 0.2).float()
    return x, y


def fp32_step_against_oracle(sed, F, prec, B=2, T=30):
    torch.manual_seed(0)
    model = sed.Cnn_AvgPooling(1, MAIN_CFG, precision=prec, mel_bins=F)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x, y = batch(B, T, F)
    loss_o, logits_o, grads_o, _, _ = O.train_step_grads(x.double(), y.double(), {k: v.double() for k, v in sd.items()}, MAIN_CFG, 5.0)
    model.cuda()
    tr = sed.FusedTrainer(model, lr=1e-3, recall_factor=5.0)
    loss = tr.forward_backward(x.cuda(), y.cuda())
    plan = next(iter(model.engine._plans.values()))
    logits = model.engine.interpolate(plan)
    assert (logits.double().cpu() - logits_o).abs().max().item() < 1e-3
    assert abs(loss.item() - float(loss_o)) < 1e-5 * max(1.0, abs(float(loss_o)))
    for n in tr.flat.names:
        gr, ref = tr.flat.G[n].double().cpu(), grads_o[n].double().view(tr.flat.G[n].shape)
        gn = ref.norm().item()
        assert abs(gr.norm().item() - gn) <= 2e-4 * max(gn, 1e-3), n
        assert ((gr - ref).abs() <= 3e-5 * max(1.0, ref.abs().max().item()) + 2e-3 * ref.abs()).all(), n
    # one Adam-amsgrad step against the oracle's
    params = {k: v.double() for k, v in sd.items() if k in grads_o}
    ast = O.AdamState()
    O.adam_amsgrad_step(params, {k: grads_o[k].double() for k in params}, ast, 1e-3)
    tr.optimizer_step()
    for n, p in model.named_parameters():
        assert (p.detach().double().cpu() - params[n]).abs().max().item() <= 2.5e-4, n
    return model


@pytest.mark.parametrize("F", [40, 100, 128])
def test_fp32_train_step_matches_oracle(sed, F):
    fp32_step_against_oracle(sed, F, "fp32")


def test_f16x3_train_step_matches_oracle_at_40(sed):
    model = fp32_step_against_oracle(sed, 40, "f16x3")
    plan = next(iter(model.engine._plans.values()))
    # the uncovered widths (40, 20, 10, 5 -- every block) run the exact fp32 kernels; nothing at a covered width here
    assert all(ly.dt_mm == sed._lib.SED_F32 for blk in plan.layers for ly in blk)


def test_bf16_train_step_at_128_tracks_the_bf16_storage_oracle(sed):
    torch.manual_seed(1)
    B, T, F = 4, 501, 128
    model = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="bf16", mel_bins=F)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x, y = batch(B, T, F, seed=7)
    model.cuda().train()
    out = model(x.cuda())
    loss = sed.WeightedBCE(5, True)(out, y.cuda())
    loss.backward()
    torch.cuda.synchronize()
    plan = next(iter(model.engine._plans.values()))
    assert not plan.c1_mode
    loss_r, logits_r, grads_r, _ = OB.train_step_grads_bf16(x, y, sd, MAIN_CFG, 5.0, c1_mode=False)
    a, r = out.detach().double().cpu().flatten(), logits_r.double().flatten()
    assert float((a @ r) / (a.norm() * r.norm())) >= 0.999
    for n, p in model.named_parameters():
        a, r = p.grad.double().cpu().flatten(), grads_r[n].double().flatten()
        cos = float((a @ r) / (a.norm() * r.norm() + 1e-30))
        # the gradients are held to the 0.95 that tests/test_gpu_parity.py::test_c1_mode_matches_default_dataflow allows the bf16
        # dataflow without C1 mode (conv1's output stored in bf16), which block 0 takes at this width: measured 0.962 at the worst
        # tensor (block 0 / block 1 conv weights), >= 0.999 elsewhere.  The fp32 / f16x3 steps at these widths hold the exact gates.
        assert cos >= 0.95, (n, cos)


def test_eval_logits_at_40_running_statistics(sed):
    torch.manual_seed(2)
    F = 40
    model = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="fp32", mel_bins=F)
    sd = model.state_dict()
    g = torch.Generator().manual_seed(4)
    for k in sd:
        if k.endswith("running_mean"):
            sd[k].copy_(0.1 * torch.randn(sd[k].shape, generator=g))
        elif k.endswith("running_var"):
            sd[k].copy_(0.5 + torch.rand(sd[k].shape, generator=g))
    model.load_state_dict(sd)
    x, _ = batch(2, 30, F)
    ref, _ = O.model_fwd(x.double(), {k: v.double() for k, v in sd.items()}, MAIN_CFG, training=False)
    model.cuda().eval()
    with torch.no_grad():
        out = model(x.cuda())
    assert (out.double().cpu() - ref).abs().max().item() < 1e-3


def test_crnn_bf16_step_at_40(sed):
    ms = importlib.import_module(PKG + ".models.spectogram_models")
    F, H = 40, 64
    sd = RO.make_state(1, MAIN_CFG, hidden=H, seed=3)
    model = ms.Crnn_AvgPooling(1, MAIN_CFG, precision="bf16", gru_hidden=H, mel_bins=F)
    model.load_state_dict(sd, strict=False)
    model.cuda().train()
    x, y = batch(2, 64, F, seed=5)
    stp = RO.CrnnAutogradStepper({k: v.double() for k, v in sd.items()}, MAIN_CFG, 5.0, 1e-3, hidden=H)
    stp.pos_weight = stp.pos_weight.double()
    out_t = stp.forward(x.double(), True)
    N = min(out_t.shape[1], 64)
    loss_t = torch.nn.functional.binary_cross_entropy_with_logits(out_t[:, :N], y.double()[:, :N], pos_weight=stp.pos_weight)
    loss_t.backward()
    out = model(x.cuda())
    loss = sed.WeightedBCE(5, True)(out, y.cuda())
    loss.backward()
    assert abs(loss.item() - float(loss_t)) < 5e-3 * max(1.0, float(loss_t))
    for n, p in model.named_parameters():
        a, r = p.grad.double().cpu().flatten(), stp.params[n].grad.double().flatten()
        cos = float((a @ r) / (a.norm() * r.norm() + 1e-30))
        assert cos >= 0.95, (n, cos)     # (bf16 outside C1 mode: as in test_bf16_train_step_at_128_tracks_the_bf16_storage_oracle)


def test_declaring_64_changes_nothing(sed):
    torch.manual_seed(3)
    m0 = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="bf16").cuda()
    m1 = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="bf16", mel_bins=64).cuda()
    m1.load_state_dict(m0.state_dict())
    x, y = batch(4, 128, 64, seed=9)
    x, y = x.cuda(), y.cuda()
    t0 = sed.FusedTrainer(m0, lr=1e-3, recall_factor=5.0)
    t1 = sed.FusedTrainer(m1, lr=1e-3, recall_factor=5.0)
    for _ in range(2):
        l0, l1 = t0.train_step(x, y), t1.train_step(x, y)
        assert torch.equal(l0, l1)
    for n in t0.flat.names:
        assert torch.equal(t0.flat.G[n], t1.flat.G[n]), n
    for (n, a), (_, b) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(a, b), n
    with torch.no_grad():
        assert torch.equal(m0(x), m1(x))


def test_graph_replay_at_40_matches_eager(sed):
    torch.manual_seed(0)
    F = 40
    m1 = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="bf16", mel_bins=F).cuda()
    m2 = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="bf16", mel_bins=F).cuda()
    m2.load_state_dict(m1.state_dict())
    t1 = sed.FusedTrainer(m1, lr=1e-4, recall_factor=5.0)
    t2 = sed.FusedTrainer(m2, lr=1e-4, recall_factor=5.0, graph=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(4, 1, 30, F, device="cuda", generator=g) for _ in range(3)]
    ys = [(torch.rand(4, 30, 1, device="cuda", generator=g) < 0.2).float() for _ in range(3)]
    for i in range(8):
        l1 = float(t1.train_step(xs[i % 3], ys[i % 3]))
        l2 = float(t2.train_step(xs[i % 3], ys[i % 3]))
        # (the graph's optimizer kernel keeps its step counter on the device and rounds differently in the last bit,
        #  tests/test_gpu_train_loop.py): the same tolerance as the young trajectories there
        assert abs(l1 - l2) < 1e-5 * max(1.0, abs(l1)), (i, l1, l2)
    assert len(t2._graphs) == 1


def test_declared_model_refuses_other_widths(sed):
    m = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="bf16", mel_bins=40).cuda()
    with pytest.raises(ValueError, match="differs from the declared"):
        m(torch.randn(1, 1, 30, 64, device="cuda"))
    m = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="bf16", mel_bins=300).cuda()
    with pytest.raises(ValueError, match="unsupported"):
        m(torch.randn(1, 1, 30, 300, device="cuda"))
