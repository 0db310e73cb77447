"""Input gradient and eval-mode (frozen-BatchNorm) backward of the raw-waveform M5 model.  Needs the MI355X:  pytest -m gpu.

1. The conv_block1 data-gradient kernel (csrc/sed_m5_dgrad.hip) through the C ABI, per element against the float64 gradient of
   F.conv1d(x, w, stride=4, padding=39).  Bounds are derived, not measured: with S = conv_transpose(|dz|, |w|),
   * dz given as a tensor: products of bf16 (or fp32) operands accumulated in fp32, at most 64 x 20 = 1280 terms per output, so
     |err| <= (n - 1) * 2^-24 * S = 2^-13.7 * S for any summation order; asserted at 2^-13 * S;
   * dz rebuilt on load (bf16): one more bf16 rounding of dz (2^-9): asserted at 2^-8 * S.
2. - 5. The model against torch.autograd on the float64 oracle (oracle/m5_oracle.forward is differentiable torch code), training and
   eval mode, fp32 at the gate tests/test_gpu_m5.py applies to M5's fp32 parameter gradients (max-relative 2e-3), bf16 at that file's
   cosine gate (0.9, full-size frames only).
"""
import importlib

import pytest
import torch
import torch.nn.functional as F

from oracle import m5_oracle as M

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
SED_F32, SED_BF16 = 0, 1
LENGTHS = [316, 2048, 2049, 2050, 2051, 31680]      # all four (L-1) % 4, L1 not a multiple of the tile, one full frame


def _pkg():
    return importlib.import_module(PKG)


def _lib():
    return importlib.import_module(PKG + "._lib")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def _to_frames(t):
    """engine layout [B/8][L1][8][C] -> (B, C, L1)"""
    n, l1, f, c = t.shape
    return t.permute(0, 2, 3, 1).reshape(n * f, c, l1)


def _ref_dx(dz64, w64, L):
    """float64 gradient of F.conv1d(x, w, stride=4, padding=39) w.r.t. x (B, 1, L) for the output gradient dz64 (B, 64, L1)"""
    return torch.nn.grad.conv1d_input((dz64.shape[0], 1, L), w64, dz64, stride=4, padding=39)


def _check(dx, ref, S, bound, what):
    dx = dx.cpu().double()
    assert not torch.isnan(dx).any(), f"{what}: NaN left in dx"
    err = (dx - ref).abs()
    for name, sl in (("head", slice(0, 40)), ("tail", slice(-43, None)), ("all", slice(None))):
        e, s = err[:, :, sl], S[:, :, sl]
        ratio = float((e / s.clamp_min(1e-300)).max())
        print(f"{what} {name}: max |err| / S = 2^{torch.log2(torch.tensor(ratio + 1e-300)).item():.2f} (bound 2^{torch.log2(torch.tensor(bound)).item():.0f})")
        assert bool((e <= bound * s).all()), (what, name, ratio)


@pytest.mark.parametrize("B", [8, 16])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_kernel_dz_given(mode, L, B):
    L_ = _lib()
    lib = L_.lib()
    dt, tdt = (SED_BF16, torch.bfloat16) if mode == "bf16" else (SED_F32, torch.float32)
    gen = torch.Generator().manual_seed(1000 + L + B)
    L1 = lib.sed_m5_conv1_len(L)
    assert L1 == (L + 78 - 79) // 4 + 1
    dz = torch.randn(B // 8, L1, 8, 64, generator=gen).to(tdt)
    w = torch.randn(64, 1, 79, generator=gen) * 0.1
    wq = w.to(tdt).double()
    dz64 = _to_frames(dz.double())
    ref = _ref_dx(dz64, wq, L)
    S = _ref_dx(dz64.abs(), wq.abs(), L)
    dzc, wc = dz.cuda(), w.cuda()
    outs = []
    for _ in range(2):
        dx = torch.full((B, 1, L), float("nan"), device="cuda")
        L_.check(lib.sed_m5_conv1_dgrad(dt, ptr(dzc), ptr(wc), ptr(dx), B, L, _stream()), "sed_m5_conv1_dgrad")
        torch.cuda.synchronize()
        outs.append(dx)
    _check(outs[0], ref, S, 2.0 ** -13, f"dz given {mode} L={L} B={B}")
    assert torch.equal(outs[0], outs[1])


def _pool_case(B, L1, gen):
    """z (bf16-exact), scale, shift such that inside every pooling window the four pre-activations scale*z + shift are pairwise
    at least |scale|/8 apart and none is closer to zero than |scale|/16: z = k/8 with four distinct integers k per window and
    shift = scale*(j + 1/2)/8.  The arg-max / ReLU decisions then cannot depend on fp32 against float64 rounding."""
    N, Ho = B // 8, L1 // 4
    scale = (torch.rand(64, generator=gen) + 0.5) * (torch.randint(0, 2, (64,), generator=gen) * 2 - 1).float()
    shift = scale * (torch.randint(-6, 6, (64,), generator=gen).float() + 0.5) / 8
    z = torch.randint(-24, 25, (N, L1, 8, 64), generator=gen).float() / 8
    base = torch.randint(-20, 9, (N, Ho, 1, 8, 64), generator=gen)
    perm = torch.rand(N, Ho, 4, 8, 64, generator=gen).argsort(dim=2)
    k = base + 3 * perm + torch.randint(0, 3, (N, Ho, 4, 8, 64), generator=gen)
    z[:, :4 * Ho] = (k.float() / 8).reshape(N, 4 * Ho, 8, 64)
    return z.bfloat16(), scale, shift


@pytest.mark.parametrize("B", [8, 16])
@pytest.mark.parametrize("L", LENGTHS)
def test_kernel_dz_rebuilt_on_load(L, B):
    L_ = _lib()
    lib = L_.lib()
    gen = torch.Generator().manual_seed(2000 + L + B)
    L1 = lib.sed_m5_conv1_len(L)
    N, Ho = B // 8, L1 // 4
    z, scale, shift = _pool_case(B, L1, gen)
    assert torch.equal(z.float().bfloat16(), z) and float(z.float().abs().max()) <= 4.0
    dy = torch.randn(N, Ho, 8, 64, generator=gen).bfloat16()
    ca = torch.rand(64, generator=gen) + 0.5
    cb = torch.randn(64, generator=gen) * 0.1
    cc = torch.randn(64, generator=gen) * 0.1
    w = torch.randn(64, 1, 79, generator=gen) * 0.1
    # ---- the property of the inputs the comparison rests on, asserted before anything is launched
    pre = z.double() * scale.double() + shift.double()                  # [N][L1][8][64]
    win = pre[:, :4 * Ho].reshape(N, Ho, 4, 8, 64)
    margin = 1e-3                                                       # fp32 fma error here is < 4 * 2^-24
    assert float(pre.abs().min()) > margin, "a pre-activation within rounding of zero"
    srt = win.sort(dim=2).values
    assert float((srt[:, :, 1:] - srt[:, :, :-1]).min()) > margin, "two pre-activations of a pooling window tie"
    # ---- float64 reference: MaxPool1d(4) arg-max + ReLU backward, BatchNorm backward, transposed convolution
    a = win.clamp_min(0)
    best, am = a.max(dim=2, keepdim=True)
    g = torch.zeros_like(win)
    g.scatter_(2, am, dy.double().unsqueeze(2) * (best > 0))
    gfull = torch.zeros_like(pre)
    gfull[:, :4 * Ho] = g.reshape(N, 4 * Ho, 8, 64)
    dz64 = _to_frames(ca.double() * gfull + cb.double() * z.double() + cc.double())
    wq = w.bfloat16().double()
    ref = _ref_dx(dz64, wq, L)
    S = _ref_dx(dz64.abs(), wq.abs(), L)
    dev = [t.cuda() for t in (dy, z, scale, shift, ca, cb, cc, w)]
    outs = []
    for _ in range(2):
        dx = torch.full((B, 1, L), float("nan"), device="cuda")
        L_.check(lib.sed_m5_conv1_dgrad_fused_pool(SED_BF16, *[ptr(t) for t in dev], ptr(dx), B, L, _stream()),
                 "sed_m5_conv1_dgrad_fused_pool")
        torch.cuda.synchronize()
        outs.append(dx)
    _check(outs[0], ref, S, 2.0 ** -8, f"dz rebuilt L={L} B={B}")
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------------------
# model level
def _is_conv_bias(n):
    return n.startswith("conv_block") and n.endswith(".bias") and n.split(".")[1] in ("0", "3")


def _model_and_sd(seed, K, precision):
    """M5 with randomised BatchNorm parameters and running statistics; returns (cuda model, CPU float32 state_dict)"""
    sed = _pkg()
    torch.manual_seed(seed)
    m = sed.M5(K, precision=precision)
    gen = torch.Generator().manual_seed(100 + seed)
    sd = m.state_dict()
    for k in sd:
        parts = k.split(".")
        if k.startswith("conv_block") and parts[1] in ("1", "4"):
            if k.endswith(".weight"):
                sd[k] = 1.0 + 0.2 * torch.randn(sd[k].shape, generator=gen)
            elif k.endswith(".bias"):
                sd[k] = 0.1 * torch.randn(sd[k].shape, generator=gen)
            elif k.endswith("running_mean"):
                sd[k] = 0.05 * torch.randn(sd[k].shape, generator=gen)
            elif k.endswith("running_var"):
                sd[k] = torch.rand(sd[k].shape, generator=gen) * 0.5 + 0.05
    m.load_state_dict(sd)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    return m.to("cuda:0"), sd


def _inputs(seed, B, L, K):
    gen = torch.Generator().manual_seed(seed)
    return 0.1 * torch.randn(B, 1, L, generator=gen), torch.randn(B, K, generator=gen)


def _oracle_grads(sd, x, R, training):
    sd64 = {}
    for k, v in sd.items():
        sd64[k] = v.double().requires_grad_() if (v.is_floating_point() and "running" not in k) else (v.double() if v.is_floating_point() else v)
    x64 = x.double().requires_grad_()
    logits, _ = M.forward(x64, sd64, training)
    (logits * R.double()).sum().backward()
    return logits.detach(), x64.grad, {k: v.grad for k, v in sd64.items() if torch.is_tensor(v) and v.requires_grad}


def _run(m, x, R, x_grad):
    for p in m.parameters():
        p.grad = None
    xc = x.cuda().requires_grad_(x_grad)
    out = m(xc)
    (out * R.cuda()).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), xc.grad, {n: p.grad.clone() for n, p in m.named_parameters()}


def _relerr(got, ref):
    return float((got.cpu().double() - ref).abs().max()) / (float(ref.abs().max()) + 1e-300)


def _cos(got, ref):
    a, b = got.cpu().double().reshape(-1), ref.reshape(-1)
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-300))


CASES = [(8, 2048, 1), (16, 4096, 3), (8, 31680, 1)]


@pytest.mark.parametrize("case", list(enumerate(CASES, 1)), ids=lambda c: "B%d-L%d-K%d" % c[1])
def test_model_train_fp32(case):
    seed, (B, L, K) = case
    m, sd = _model_and_sd(seed, K, "fp32")
    m.train()
    x, R = _inputs(seed, B, L, K)
    _, dx_ref, g_ref = _oracle_grads(sd, x, R, True)
    out, dx, grads = _run(m, x, R, True)
    assert dx is not None and dx.shape == x.shape
    e = _relerr(dx, dx_ref)
    print(f"train fp32 B={B} L={L} K={K}: x.grad max-relative error {e:.3e}")
    assert e < 2e-3, ("x.grad", e)
    for n, g in grads.items():
        if _is_conv_bias(n):
            assert float(g.abs().max()) == 0.0, n
            continue
        e = _relerr(g, g_ref[n])
        assert e < 2e-3, (n, e)
    out2, dx2, grads2 = _run(m, x, R, False)
    assert dx2 is None
    assert torch.equal(out, out2)
    for n in grads:
        assert torch.equal(grads[n], grads2[n]), n


@pytest.mark.parametrize("case", list(enumerate(CASES + [(5, 2048, 1)], 1)), ids=lambda c: "B%d-L%d-K%d" % c[1])
def test_model_eval_fp32(case):
    seed, (B, L, K) = case
    m, sd = _model_and_sd(seed, K, "fp32")
    m.eval()
    x, R = _inputs(seed, B, L, K)
    _, dx_ref, g_ref = _oracle_grads(sd, x, R, False)
    with torch.no_grad():
        out0 = m(x.cuda())
    out, dx, grads = _run(m, x, R, True)
    assert torch.equal(out, out0)
    after = m.state_dict()
    for k, v in sd.items():
        if "running" in k or k.endswith("num_batches_tracked"):
            assert torch.equal(after[k].cpu(), v), k
    assert dx.shape == x.shape
    e = _relerr(dx, dx_ref)
    print(f"eval fp32 B={B} L={L} K={K}: x.grad max-relative error {e:.3e}")
    assert e < 2e-3, ("x.grad", e)
    for n, g in grads.items():
        e = _relerr(g, g_ref[n])
        assert e < 2e-3, (n, e)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_model_bf16_full_frame(training):
    B, L, K = 8, 31680, 1
    m, sd = _model_and_sd(4, K, "bf16")
    m.train(training)
    x, R = _inputs(4, B, L, K)
    _, dx_ref, g_ref = _oracle_grads(sd, x, R, training)
    out, dx, grads = _run(m, x, R, True)
    cx, cw = _cos(dx, dx_ref), _cos(grads["conv_block1.0.weight"], g_ref["conv_block1.0.weight"])
    print(f"bf16 {'train' if training else 'eval'}: cosine x.grad {cx:.4f}, conv_block1.0.weight {cw:.4f}")
    out2, dx2, grads2 = _run(m, x, R, False)
    assert dx2 is None
    for n in grads:
        assert torch.equal(grads[n], grads2[n]), n
    assert cx > 0.9, (cx, cw)


def test_front_end_parameter_gets_its_gradient():
    B, L, K = 8, 2048, 1
    m, sd = _model_and_sd(5, K, "fp32")
    m.train()
    x, R = _inputs(5, B, L, K)
    a0 = 0.75
    _, dx_ref, _ = _oracle_grads(sd, a0 * x, R, True)
    ref = float((dx_ref * x.double()).sum())
    a = torch.nn.Parameter(torch.tensor(a0, device="cuda"))
    xc = x.cuda()
    out = m(a * xc)
    (out * R.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert a.grad is not None
    e = abs(float(a.grad) - ref) / (abs(ref) + 1e-300)
    print(f"front-end gain: a.grad {float(a.grad):.6e} reference {ref:.6e} relative error {e:.3e}")
    assert e < 2e-3, e
