"""Input gradients and eval-mode (frozen-BatchNorm) backward of the CNN / CRNN models.  Needs the MI355X:  pytest -m gpu.

Kernel level (csrc/sed_c1_dx.hip, through the C ABI): conv1's data gradient onto the single input channel with BN1's backward
produced on load, and the eval-mode BatchNorm finalizes, against float64 formulas on the values the kernels see.
Model level: x.grad and every parameter gradient against oracle/cnn_oracle.py (and a torch CRNN with the same weights) run in
float64 and differentiated by torch.autograd, in training and in eval mode."""
import importlib

import pytest
import torch
import torch.nn.functional as Fn

from oracle import cnn_oracle as O
from oracle import crnn_oracle as RO

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
BF = torch.bfloat16
F64 = torch.float64
MAIN_CFG = [(32, 2), (64, 2), (128, 2), (128, 1)]
WIDTHS = [1, 3, 5, 12, 40, 64, 100, 128, 200, 256]


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


# ---------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------
def c1_dgrad_case(L, dt, W, H, Cout, zmode, zscore, seed):
    g = torch.Generator().manual_seed(seed)
    B, Cp = 2, (Cout + 31) // 32 * 32
    sto = BF if dt == "bf16" else torch.float32
    x = torch.randn(B, H, W, generator=g) * 2 + 0.5
    w1 = torch.randn(Cout, 1, 3, 3, generator=g)
    gr = torch.zeros(B, H, W, Cp)
    gr[..., :Cout] = torch.randn(B, H, W, Cout, generator=g)
    ca, cb, cc = (torch.zeros(Cp) for _ in range(3))
    ca[:Cout] = torch.rand(Cout, generator=g) + 0.5
    cb[:Cout] = torch.randn(Cout, generator=g) * 0.3
    cc[:Cout] = torch.randn(Cout, generator=g)                 # large offset: must not leak into the zero padding
    mean = torch.randn(W, generator=g) if zscore else None
    std = (torch.rand(W, generator=g) + 0.5) if zscore else None
    xn = x.double() if not zscore else (x.double() - mean.double()) / std.double()
    zref = O.conv3x3_fwd(xn[:, None], w1.double()).permute(0, 2, 3, 1)          # [B][H][W][Cout] float64
    if zmode == "given":
        zt = torch.zeros(B, H, W, Cp)
        zt[..., :Cout] = torch.randn(B, H, W, Cout, generator=g)
        zd = zt.to(sto).cuda()
        z64 = zd.double().cpu()[..., :Cout]
    else:
        zd, z64 = None, zref
    gd = gr.to(sto).cuda()
    g64 = gd.double().cpu()[..., :Cout]
    dz1 = (ca[:Cout].double() * g64 + cb[:Cout].double() * z64 + cc[:Cout].double()).permute(0, 3, 1, 2)
    ref = Fn.conv_transpose2d(dz1, w1.double(), padding=1)[:, 0]
    S = Fn.conv_transpose2d(dz1.abs(), w1.double().abs(), padding=1)[:, 0]
    if zscore:
        ref, S = ref / std.double(), S / std.double()
    dx = torch.full((B, H, W), float("nan"), device="cuda")
    dtc = L.SED_BF16 if dt == "bf16" else L.SED_F32
    # (device copies held in names: a temporary freed before the launch would hand its memory to the next copy)
    xd, wd, cad, cbd, ccd = (t.cuda() for t in (x, w1, ca, cb, cc))
    md, sd = (mean.cuda(), std.cuda()) if zscore else (None, None)
    L.check(L.lib().sed_conv3x3_c1_dgrad(dtc, ptr(gd), ptr(zd), ptr(xd), ptr(md), ptr(sd), ptr(wd), ptr(cad), ptr(cbd), ptr(ccd),
                                         ptr(dx), B, H, W, Cout, Cp, st()), "c1_dgrad")
    torch.cuda.synchronize()
    got = dx.double().cpu()
    what = f"{dt} W={W} H={H} Cout={Cout} z={zmode} zscore={zscore}"
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    tol = 2.0 ** -16 * S + 1e-30
    assert (err <= tol).all(), f"{what}: max err/S {(err / S.clamp_min(1e-30)).max().item():.3e}"
    # the image border (where the padding starts) explicitly
    for sl in ((slice(None), 0), (slice(None), H - 1), (slice(None), slice(None), 0), (slice(None), slice(None), W - 1)):
        assert (err[sl] <= tol[sl]).all(), f"{what}: border"


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("W", WIDTHS)
def test_c1_dgrad_kernel_matches_float64(L, dt, W):
    for i, (H, zscore) in enumerate(((1, False), (11, True), (19, False))):
        Cout = (32, 64, 40)[(W + i) % 3]
        c1_dgrad_case(L, dt, W, H, Cout, "given", zscore, seed=W * 7 + i)
    # z1 recomputed from the input (C1 mode: bf16, W = 64, 32 channels; the form is shape-general)
    if dt == "bf16" and W in (64, 5, 100):
        for H, zscore in ((1, True), (13, False), (9, True)):
            c1_dgrad_case(L, dt, W, H, 32, "recompute", zscore, seed=W + H)


def test_eval_bn_kernels_match_float64(L):
    g = torch.Generator().manual_seed(5)
    C, Cp, npart = 40, 64, 37
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.2
    gamma = torch.randn(C, generator=g)
    mean, invstd = torch.full((Cp,), float("nan"), device="cuda"), torch.full((Cp,), float("nan"), device="cuda")
    rmd, rvd, gd = rm.cuda(), rv.cuda(), gamma.cuda()
    L.check(L.lib().sed_bn_eval_stats(ptr(rmd), ptr(rvd), 1e-5, ptr(mean), ptr(invstd), C, Cp, st()), "eval_stats")
    torch.cuda.synchronize()
    assert torch.equal(mean[:C].cpu(), rm) and (mean[C:] == 0).all() and (invstd[C:] == 0).all()
    assert torch.allclose(invstd[:C].cpu(), 1.0 / torch.sqrt(rv + 1e-5), rtol=1e-6, atol=0)
    part = torch.randn(npart, 2, Cp, generator=g)
    outs = [torch.full((Cp,), float("nan"), device="cuda") for _ in range(5)]
    pd = part.cuda()
    L.check(L.lib().sed_bn_eval_bwd_finalize(ptr(pd), npart, ptr(gd), ptr(mean), ptr(invstd),
                                             *[ptr(o) for o in outs], C, Cp, st()), "eval_bwd_finalize")
    torch.cuda.synchronize()
    dgam, dbet, ca, cb, cc = (o.double().cpu() for o in outs)
    s, q = part[:, 0].double().sum(0), part[:, 1].double().sum(0)
    is64 = invstd.double().cpu()
    assert torch.allclose(dbet[:C], s[:C], rtol=1e-6, atol=1e-6) and torch.allclose(dgam[:C], q[:C], rtol=1e-6, atol=1e-6)
    assert torch.allclose(ca[:C], gamma.double() * is64[:C], rtol=1e-6)
    assert (cb == 0).all() and (cc == 0).all() and (ca[C:] == 0).all()
    # C1 form: sum g from row 0, sum g*z1 = w1 . A
    A = torch.randn(9, Cp, generator=g)
    w1 = torch.randn(C, 9, generator=g)
    outs = [torch.full((Cp,), float("nan"), device="cuda") for _ in range(5)]
    Ad, w1d = A.cuda(), w1.cuda()
    L.check(L.lib().sed_bn_eval_bwd_finalize_c1(ptr(pd), npart, ptr(Ad), ptr(w1d), ptr(gd), ptr(mean),
                                                ptr(invstd), *[ptr(o) for o in outs], C, Cp, st()), "eval_bwd_finalize_c1")
    torch.cuda.synchronize()
    dgam, dbet, ca, cb, cc = (o.double().cpu() for o in outs)
    sgz = (w1.double() * A[:, :C].double().t()).sum(1)
    want = is64[:C] * (sgz - rm.double() * s[:C])
    assert torch.allclose(dbet[:C], s[:C], rtol=1e-6, atol=1e-6)
    assert torch.allclose(dgam[:C], want, rtol=1e-5, atol=1e-5)
    assert torch.allclose(ca[:C], gamma.double() * is64[:C], rtol=1e-6) and (cb == 0).all() and (cc == 0).all()
    amax = torch.empty(1, device="cuda")
    v = torch.randn(100003, generator=g)
    v[77777] = -1234.5
    vd = v.cuda()
    L.check(L.lib().sed_absmax(ptr(vd), v.numel(), ptr(amax), st()), "absmax")
    assert amax.item() == 1234.5


# ---------------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------------
def randomize_bn(module, seed):
    """non-trivial running statistics and affine parameters (BatchNorm far from the identity)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, b in module.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g) * 0.3)
            elif n.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g) * 1.5 + 0.3)
        for n, p in module.named_parameters():
            if ".bn" in n or n.startswith("bn"):
                p.copy_(1 + 0.3 * torch.randn(p.shape, generator=g) if n.endswith("weight") else 0.2 * torch.randn(p.shape, generator=g))


def make_model(sed, prec, F, K=3, seed=0, crnn=False):
    torch.manual_seed(seed)
    mb = None if F == 64 else F
    if crnn:
        model = sed.Crnn_AvgPooling(K, MAIN_CFG, precision=prec, gru_hidden=32, mel_bins=mb)
    else:
        model = sed.Cnn_AvgPooling(K, MAIN_CFG, precision=prec, mel_bins=mb)
    randomize_bn(model, seed + 1)
    return model


def ref_grads(model, x, R, training):
    """float64 reference: oracle forward differentiated by torch.autograd; returns (logits, x.grad, {name: grad})"""
    sd = {k: v.detach().double().cpu().clone() for k, v in model.state_dict().items()}
    names = [n for n, _ in model.named_parameters()]
    for n in names:
        sd[n].requires_grad_(True)
    x64 = x.detach().double().cpu().requires_grad_(True)
    out, _ = O.model_fwd(x64, sd, MAIN_CFG, training)
    (out * R).sum().backward()
    return out.detach(), x64.grad, {n: sd[n].grad for n in names}


def model_grads(model, x, R):
    for p in model.parameters():
        p.grad = None
    xd = x.cuda().requires_grad_(True)
    out = model(xd)
    (out * R.cuda().float()).sum().backward()
    return out.detach(), xd.grad, {n: p.grad for n, p in model.named_parameters()}


def gate(got, ref, what, scale=1.0):
    got, ref = got.detach().double().cpu() / scale, ref.double() / scale
    tol = 3e-5 * max(1.0, ref.abs().max().item()) + 1e-3 * ref.abs()
    err = (got - ref).abs()
    assert torch.isfinite(got).all() and (err <= tol).all(), f"{what}: max err {err.max().item():.3e} (ref max {ref.abs().max().item():.3e})"


def cosine(a, b):
    a, b = a.detach().double().cpu().flatten(), b.double().flatten()
    return (a @ b / (a.norm() * b.norm()).clamp_min(1e-300)).item()


def batch(B, T, F, K=3, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 1, T, F, generator=g), torch.randn(B, T, K, generator=g).double()


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("F", [64, 40, 100])
def test_train_input_grad_matches_float64(sed, prec, F):
    model = make_model(sed, prec, F)
    x, R = batch(2, 32, F)
    _, xg_o, g_o = ref_grads(model, x, R, True)
    model.cuda()
    _, xg, gr = model_grads(model, x, R)
    assert xg is not None and xg.shape == x.shape
    gate(xg, xg_o, f"{prec} F={F} x.grad")
    for n in g_o:
        gate(gr[n], g_o[n], f"{prec} F={F} {n}")
    if prec == "fp32":
        # the input gradient only adds a read of buffers that exist: the parameter gradients are the same bits
        for p in model.parameters():
            p.grad = None
        out = model(x.cuda())
        (out * R.cuda().float()).sum().backward()
        for n, p in model.named_parameters():
            assert torch.equal(p.grad, gr[n]), n


@pytest.mark.parametrize("F", [64, 40])
def test_bf16_train_input_grad_cosine(sed, F):
    model = make_model(sed, "bf16", F)
    x, R = batch(2, 32, F)
    _, xg_o, g_o = ref_grads(model, x, R, True)
    model.cuda()
    _, xg, gr = model_grads(model, x, R)
    if F == 64:
        assert next(iter(model.engine._plans.values())).c1_mode, "F = 64 under bf16 runs C1 mode"
    cs = {"x": cosine(xg, xg_o)}
    cs.update({n: cosine(gr[n], g_o[n]) for n in g_o})
    print(f"bf16 F={F} cosines: min {min(cs.values()):.5f}  x {cs['x']:.5f}")
    if F == 64:
        # C1 mode: the input gradient takes the unfused block-0 route, so every gradient is gated
        assert min(cs.values()) >= 0.95, cs
        return
    # elsewhere the backward is the training step's own (bf16 parameter-gradient noise of that dataflow: ~0.95 at worst on this
    # sum-reduced upstream gradient): the parameter gradients must be its bits, the new input gradient is gated
    assert cs["x"] >= 0.95, cs
    for p in model.parameters():
        p.grad = None
    out = model(x.cuda())
    (out * R.cuda().float()).sum().backward()
    for n, p in model.named_parameters():
        assert torch.equal(p.grad, gr[n]), n


@pytest.mark.parametrize("prec", ["fp32", "f16x3", "bf16"])
def test_eval_backward_cnn(sed, prec):
    model = make_model(sed, prec, 64, seed=3)
    x, R = batch(2, 32, 64, seed=4)
    out_o, xg_o, g_o = ref_grads(model, x, R, False)
    model.cuda().eval()
    bufs = {n: b.clone() for n, b in model.named_buffers()}
    with torch.no_grad():
        out_ng = model(x.cuda())
    out, xg, gr = model_grads(model, x, R)
    assert torch.equal(out, out_ng), "eval logits with grad enabled differ from the no_grad forward"
    model._flush_counters()
    for n, b in model.named_buffers():
        assert torch.equal(b, bufs[n]), n
    if prec == "bf16":
        cs = [cosine(xg, xg_o)] + [cosine(gr[n], g_o[n]) for n in g_o]
        print(f"bf16 eval cosines: min {min(cs):.5f}  x {cs[0]:.5f}")
        assert min(cs) >= 0.95
        return
    assert (out.double().cpu() - out_o).abs().max().item() < 1e-3
    gate(xg, xg_o, f"{prec} eval x.grad")
    for n in g_o:
        gate(gr[n], g_o[n], f"{prec} eval {n}")


@pytest.mark.parametrize("prec", ["fp32", "f16x3", "bf16"])
def test_eval_backward_conv_block(sed, prec):
    ms = importlib.import_module(PKG + ".models.spectogram_models")
    torch.manual_seed(0)
    blk = ms.ConvBlock(32, 64, 2, precision=prec)
    randomize_bn(blk, 7)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 32, 12, 32, generator=g)
    sd = {"b." + k: v.detach().double().clone() for k, v in blk.state_dict().items()}
    names = ["b." + n for n, _ in blk.named_parameters()]
    for n in names:
        sd[n].requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    out_o, _ = O.conv_block_fwd(x64, sd, "b", 2, False)
    R = torch.randn(out_o.shape, generator=g).double()
    (out_o * R).sum().backward()
    blk.cuda().eval()
    bufs = {n: b.clone() for n, b in blk.named_buffers()}
    with torch.no_grad():
        out_ng = blk(x.cuda())
    xd = x.cuda().requires_grad_(True)
    out = blk(xd)
    (out * R.cuda().float()).sum().backward()
    assert torch.equal(out.detach(), out_ng)
    for n, b in blk.named_buffers():
        assert torch.equal(b, bufs[n]), n
    got = {"b." + n: p.grad for n, p in blk.named_parameters()}
    if prec == "bf16":
        cs = [cosine(xd.grad, x64.grad)] + [cosine(got[n], sd[n].grad) for n in names]
        assert min(cs) >= 0.95, cs
        return
    gate(xd.grad, x64.grad, f"{prec} block x.grad")
    for n in names:
        gate(got[n], sd[n].grad, f"{prec} block {n}")


def crnn_reference(model, x, R, training):
    sd = {k: v.detach().double().cpu().clone() for k, v in model.state_dict().items()}
    stp = RO.CrnnAutogradStepper(sd, MAIN_CFG, 5.0, 1e-3, hidden=32)
    x64 = x.double().requires_grad_(True)
    out = stp.forward(x64, training)
    (out * R).sum().backward()
    return x64.grad, {n: p.grad for n, p in stp.params.items()}


def test_crnn_input_grad_and_eval_backward(sed):
    model = make_model(sed, "fp32", 64, seed=5, crnn=True)
    x, R = batch(2, 32, 64, seed=6)
    for training in (True, False):
        xg_o, g_o = crnn_reference(model, x, R, training)
        model.cuda().train(training)
        _, xg, gr = model_grads(model, x, R)
        model.cpu()
        for n, ref in [("x", xg_o)] + sorted(g_o.items()):
            got = (xg if n == "x" else gr[n]).double().cpu()
            err = (got - ref).abs().max().item()
            assert err <= 1e-3 * max(1.0, ref.abs().max().item()), f"training={training} {n}: {err:.3e}"


@pytest.mark.parametrize("training", [True, False])
def test_f16x3_upstream_scale_sweep(sed, training):
    """a sum-reduced / one-hot upstream gradient is 2^17..2^26 x the mean-reduced loss's: the f16x3 pre-scale follows its magnitude"""
    model = make_model(sed, "f16x3", 64, seed=9)
    x, R = batch(2, 32, 64, seed=10)
    _, xg_o, g_o = ref_grads(model, x, R, training)
    _, xs_o, s_o = ref_grads(model, x, torch.ones_like(R), training)
    model.cuda().train(training)
    for k in list(range(-12, 25, 4)) + [None]:
        scale = 1.0 if k is None else 2.0 ** k
        Rk = torch.ones_like(R) if k is None else R * scale
        _, xg, gr = model_grads(model, x, Rk)
        rx, rg = (xs_o, s_o) if k is None else (xg_o, g_o)
        gate(xg, rx * scale, f"k={k} x.grad", scale)
        for n in rg:
            gate(gr[n], rg[n] * scale, f"k={k} {n}", scale)


def test_infer_saliency_cli(tmp_path):
    import numpy as np
    from scipy.io import wavfile
    sed = importlib.import_module(PKG)
    infer = importlib.import_module(PKG + ".infer")
    sr = 48000
    wav = (0.05 * np.random.default_rng(1).standard_normal(sr * 6)).astype(np.float32)
    p = str(tmp_path / "clip.wav")
    wavfile.write(p, sr, wav)
    torch.manual_seed(0)
    model = sed.Cnn_AvgPooling(1, MAIN_CFG)          # (the CLI builds the config's one-class model)
    randomize_bn(model, 11)
    ck = str(tmp_path / "m.pth")
    torch.save({"iterations": 0, "model": model.state_dict()}, ck)
    infer.main([p, "--ckpt", ck, "--outputs_dir", str(tmp_path / "plain"), "--precision", "fp32"])
    infer.main([p, "--ckpt", ck, "--outputs_dir", str(tmp_path / "sal"), "--precision", "fp32", "--saliency"])
    z0, z1 = np.load(tmp_path / "plain" / "clip.npz"), np.load(tmp_path / "sal" / "clip.npz")
    assert sorted(z0.files) == ["decisions", "onset_frames", "onset_seconds", "probabilities"]
    assert sorted(z1.files) == sorted(z0.files + ["saliency"])
    assert np.array_equal(z0["probabilities"], z1["probabilities"])
    res = infer.infer_file(p, ck, precision="fp32")
    x = torch.from_numpy(res["log_mel"]).cuda()[None, None]
    K = res["probabilities"].shape[1]
    sal = z1["saliency"]
    assert sal.shape == (x.shape[2], x.shape[3], K) and np.isfinite(sal).all() and np.abs(sal).max() > 0
    m = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="fp32").cuda()
    m.load_state_dict(torch.load(ck)["model"])
    m.eval()
    for k in range(K):
        xg = x.clone().requires_grad_(True)
        torch.sigmoid(m(xg))[0, :, k].sum().backward()
        assert np.array_equal(sal[:, :, k], xg.grad[0, 0].cpu().numpy()), k
