"""GPU: sed_pcen_fwd / sed_pcen_bwd (csrc/sed_pcen.hip) through the C ABI, the PCEN layer under autograd, and the layer inside
Cnn_AvgPooling and FusedTrainer.

Reference: tests/pcen_formula.py (float64 loops over t; checked against torch autograd on the host in tests/test_pcen_host.py).
Bound, for every element of y and dx and every entry of dtheta: |got - ref| <= 2^-23 |ref| + 2^-40 A, A the formula's companion
(the same expression over absolute values): the one fp32 rounding of a double result plus the slack of the project's
double-arithmetic kernels.  The worst error / bound is printed per check (-s).
Every output lies in a sentinel-filled buffer between two canary regions; every input must be unmodified afterwards."""
import importlib

import numpy as np
import pytest
import torch

import pcen_formula as PF

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
MAIN_CFG = [(32, 2), (64, 2), (128, 2), (128, 1)]
EPS, GAIN = 1e-6, 1.5
PAD = 512               # canary floats on either side of an output
NAMES = ("log_alpha", "log_delta", "log_r", "logit_s")


@pytest.fixture(scope="module")
def sed():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def chunk(sed):
    c = sed._lib.lib().sed_pcen_chunk()
    assert c >= 2
    return c


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """an fp32 output of `shape` inside a buffer of sentinels"""

    def __init__(self, shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * PAD,), -777.25, dtype=torch.float32, device="cuda")
        self.view = self.buf[PAD:PAD + self.n].view(shape)

    def get(self):
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        assert np.all(h[:PAD] == -777.25) and np.all(h[PAD + self.n:] == -777.25), "a write outside the output"
        out = h[PAD:PAD + self.n].reshape(tuple(self.view.shape))
        assert not np.any(out == -777.25), "an output element was not written"
        return out.copy()


def draw(B, T, F, kind, norm, memory, seed):
    """fp32 inputs (as float32 numpy arrays): x, theta (4, F), mean, std, g"""
    rng = np.random.default_rng(seed)
    theta = np.stack([np.log(0.98) + 0.1 * rng.standard_normal(F), np.log(2.0) + 0.2 * rng.standard_normal(F),
                      np.log(0.5) + 0.1 * rng.standard_normal(F), np.log(0.025 / 0.975) + 0.5 * rng.standard_normal(F)])
    if memory == "long":
        theta[3] = -9.0
    elif memory == "short":
        theta[3] = 9.0
    mean = std = None
    if kind == 0:
        x = -30.0 + 10.0 * rng.standard_normal((B, T, F))
        if norm:
            mean, std = (-30.0 + rng.standard_normal(F)).astype(np.float32), (10.0 + rng.standard_normal(F)).astype(np.float32)
            x = (x - mean) / std
    else:
        x = np.maximum(rng.standard_normal((B, T, F)), -0.2) * 1e-3
        x[rng.random((B, T, F)) < 0.1] = 0.0
        x[0, 0, 0] = 0.0                       # an exact zero and a negative input in every case, also the smallest
        x[-1, -1, -1] = -1e-3
    g = rng.standard_normal((B, T, F))
    return x.astype(np.float32), theta.astype(np.float32), mean, std, g.astype(np.float32)


def run_fwd(L, x, theta, mean, std, kind, ws=None):
    B, T, F = x.shape
    y = Guarded((B, T, F))
    ws = torch.empty((L.lib().sed_pcen_ws_bytes(B, T, F) + 7) // 8, dtype=torch.float64, device="cuda") if ws is None else ws
    L.check(L.lib().sed_pcen_fwd(L.ptr(x), L.ptr(mean), L.ptr(std), L.ptr(theta), kind, EPS, GAIN, L.ptr(y.view), L.ptr(ws), B, T, F,
                                 stream()), "sed_pcen_fwd")
    return y.get()


def run_bwd(L, x, theta, mean, std, kind, g, want_dx=True, want_dtheta=True):
    B, T, F = x.shape
    dx = Guarded((B, T, F)) if want_dx else None
    dth = Guarded((4, F)) if want_dtheta else None
    ws = torch.full(((L.lib().sed_pcen_ws_bytes(B, T, F) + 7) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    L.check(L.lib().sed_pcen_bwd(L.ptr(x), L.ptr(mean), L.ptr(std), L.ptr(theta), kind, EPS, GAIN, L.ptr(g),
                                 None if dx is None else L.ptr(dx.view), None if dth is None else L.ptr(dth.view), L.ptr(ws), B, T, F,
                                 stream()), "sed_pcen_bwd")
    return (None if dx is None else dx.get()), (None if dth is None else dth.get())


def check(name, got, ref, A, worst):
    ratio = PF.worst_ratio(got, ref, A)
    worst[name] = max(worst.get(name, 0.0), ratio)
    print(f"  {name}: worst error / bound {ratio:.3f}")
    assert np.all(np.isfinite(got)), name
    assert ratio <= 1.0, f"{name}: error {ratio:.3f} x the bound 2^-23 |ref| + 2^-40 A"


# (B, T as a function of the chunk, F, kind, mean / std, memory): every T of {1, 2, c - 1, c, c + 1, 3c + 5}, every F of
# {1, 5, 64, 70, 256}, both B; (3, 3c + 5) with F = 5 and F = 64; both kinds; mean / std given and NULL; sigma = -9 and +9
CASES = [
    (1, lambda c: 1, 1, 0, False, "drawn"),
    (3, lambda c: 2, 5, 0, True, "drawn"),
    (1, lambda c: c - 1, 70, 1, False, "drawn"),
    (3, lambda c: c, 256, 0, True, "drawn"),
    (1, lambda c: c + 1, 64, 1, False, "drawn"),
    (3, lambda c: 3 * c + 5, 5, 0, True, "drawn"),
    (3, lambda c: 3 * c + 5, 64, 0, False, "drawn"),
    (3, lambda c: 3 * c + 5, 5, 1, False, "drawn"),
    (3, lambda c: 3 * c + 5, 64, 0, True, "long"),
    (3, lambda c: 3 * c + 5, 5, 0, True, "short"),
    (3, lambda c: 3 * c + 5, 64, 1, False, "long"),
    (1, lambda c: 3 * c + 5, 70, 1, False, "short"),
    (1, lambda c: 1, 256, 1, False, "drawn"),
]
WORST = {}


@pytest.mark.parametrize("case", range(len(CASES)))
def test_kernels_against_the_formula(sed, chunk, case):
    """y, dx and dtheta within the bound; dx = NULL and dtheta = NULL each leave the other output's bits unchanged; a second run
    gives the same bits; kind 1: the gradient at zero and negative inputs is exactly 0; the inputs are not modified"""
    L = sed._lib
    B, Tf, F, kind, norm, memory = CASES[case]
    T = Tf(chunk)
    x, theta, mean, std, g = draw(B, T, F, kind, norm, memory, seed=100 + case)
    print(f"B {B} T {T} F {F} kind {kind} mean/std {norm} memory {memory}")
    y_ref, A_y = PF.forward(x, theta, kind, EPS, GAIN, mean, std)
    bw = PF.backward(x, theta, kind, EPS, GAIN, g, mean, std)
    ins = [dev(x), dev(theta), dev(mean), dev(std), dev(g)]
    xd, td, md, sd_, gd = ins
    y = run_fwd(L, xd, td, md, sd_, kind)
    check("y", y, y_ref, A_y, WORST)
    dx, dth = run_bwd(L, xd, td, md, sd_, kind, gd)
    check("dx", dx, bw["dx"], bw["A_dx"], WORST)
    check("dtheta", dth, bw["dtheta"], bw["A_dtheta"], WORST)
    if kind == 1:
        assert np.any(x == 0) and np.any(x < 0) and np.all(dx[x <= 0] == 0.0)
    # NULL outputs
    dx_only, none = run_bwd(L, xd, td, md, sd_, kind, gd, want_dtheta=False)
    assert none is None and np.array_equal(dx_only.view(np.uint32), dx.view(np.uint32))
    none, dth_only = run_bwd(L, xd, td, md, sd_, kind, gd, want_dx=False)
    assert none is None and np.array_equal(dth_only.view(np.uint32), dth.view(np.uint32))
    # determinism
    assert np.array_equal(run_fwd(L, xd, td, md, sd_, kind).view(np.uint32), y.view(np.uint32))
    dx2, dth2 = run_bwd(L, xd, td, md, sd_, kind, gd)
    assert np.array_equal(dx2.view(np.uint32), dx.view(np.uint32)) and np.array_equal(dth2.view(np.uint32), dth.view(np.uint32))
    for t, h in zip(ins, (x, theta, mean, std, g)):
        if t is not None:
            assert np.array_equal(t.cpu().numpy(), h), "an input was modified"
    print("  worst so far:", {k: round(v, 3) for k, v in WORST.items()})


def layer_for(sed, F, kind, mean, std, theta, trainable=True):
    layer = sed.PCEN(F, input="db" if kind == 0 else "power", mean=mean, std=std, eps=EPS, gain=GAIN, trainable=trainable).cuda()
    with torch.no_grad():
        for i, n in enumerate(NAMES):
            getattr(layer, n).copy_(torch.as_tensor(theta[i]))
    return layer


@pytest.mark.parametrize("four_d", [True, False])
def test_layer_under_autograd(sed, chunk, four_d):
    """PCEN under autograd with a non-contiguous upstream gradient: the same bits as the direct calls"""
    L = sed._lib
    B, T, F = 2, chunk + 3, 70
    x, theta, mean, std, g = draw(B, T, F, 0, True, "drawn", seed=7)
    layer = layer_for(sed, F, 0, mean, std, theta)
    xd, td, md, sd_, gd = dev(x), dev(theta), dev(mean), dev(std), dev(g)
    y_ref = run_fwd(L, xd, td, md, sd_, 0)
    dx_ref, dth_ref = run_bwd(L, xd, td, md, sd_, 0, gd)
    shape = (B, 1, T, F) if four_d else (B, T, F)
    xin = xd.view(shape).clone().requires_grad_(True)
    y = layer(xin)
    assert y.shape == shape and np.array_equal(y.detach().cpu().numpy().reshape(B, T, F), y_ref)
    wide = torch.zeros(shape[:-1] + (2 * F,), device="cuda")
    wide[..., ::2] = gd.view(shape)
    up = wide[..., ::2]
    assert not up.is_contiguous()
    y.backward(up)
    assert np.array_equal(xin.grad.cpu().numpy().reshape(B, T, F), dx_ref)
    for i, n in enumerate(NAMES):
        assert np.array_equal(getattr(layer, n).grad.cpu().numpy(), dth_ref[i]), n
    assert layer.backward_calls == 1


def test_fixed_layer(sed, chunk):
    """trainable=False: no .grad anywhere, no backward launch when the input needs none, dx alone when it does"""
    L = sed._lib
    B, T, F = 1, chunk + 1, 5
    x, theta, _, _, g = draw(B, T, F, 1, False, "drawn", seed=8)
    layer = layer_for(sed, F, 1, None, None, theta, trainable=False)
    assert list(layer.parameters()) == []
    xd, td, gd = dev(x), dev(theta), dev(g)
    y = layer(xd.view(B, 1, T, F))
    assert not y.requires_grad and layer.backward_calls == 0
    assert np.array_equal(y.cpu().numpy().reshape(B, T, F), run_fwd(L, xd, td, None, None, 1))
    xin = xd.clone().requires_grad_(True)
    layer(xin).backward(gd)
    dx_ref, _ = run_bwd(L, xd, td, None, None, 1, gd, want_dtheta=False)
    assert layer.backward_calls == 1 and np.array_equal(xin.grad.cpu().numpy(), dx_ref)
    assert all(getattr(layer, n).grad is None for n in NAMES)
    with pytest.raises(RuntimeError, match="no CPU path"):
        layer(torch.zeros(1, 1, 4, F))
    with pytest.raises(ValueError, match="mel bins"):
        layer(torch.zeros(1, 1, 4, F + 1, device="cuda"))


def model_input(B=2, T=64, F=64, seed=11):
    rng = np.random.default_rng(seed)
    x = (-30.0 + 10.0 * rng.standard_normal((B, 1, T, F))).astype(np.float32)
    y = (rng.random((B, T, 1)) > 0.8).astype(np.float32)
    return x, y


def make_model(sed, layer=None, seed=0):
    torch.manual_seed(seed)
    return sed.Cnn_AvgPooling(1, MAIN_CFG, precision="fp32", frontend=layer).cuda().train()


def drawn_layer(sed, trainable=True, F=64):
    _, theta, _, _, _ = draw(1, 1, F, 0, False, "drawn", seed=12)
    return layer_for(sed, F, 0, None, None, theta, trainable=trainable), theta


def test_composition_with_autograd(sed):
    """model(x) with a trainable layer, loss.backward(): frontend.*.grad and x.grad within the bound of the formula's backward
    applied to the gradient that reached the layer's output; the other parameters' gradients the same bits as those of a model
    without the layer fed the layer's output"""
    x, tgt = model_input()
    layer, theta = drawn_layer(sed)
    model = make_model(sed, layer)
    crit = sed.WeightedBCE(5, True)
    seen = {}

    def keep_output(module, inputs, output):        # the layer's output and the gradient that reaches it
        seen["y"] = output.detach().clone()
        output.register_hook(lambda gr: seen.__setitem__("g", gr.detach().clone()))

    model.frontend.register_forward_hook(keep_output)
    xin = dev(x).requires_grad_(True)
    loss = crit(model(xin), dev(tgt))
    loss.backward()
    torch.cuda.synchronize()
    assert np.isfinite(loss.item()) and seen["g"].shape == (2, 1, 64, 64)
    gy = seen["g"].cpu().numpy().reshape(2, 64, 64)
    assert np.abs(gy).max() > 0
    bw = PF.backward(x.reshape(2, 64, 64), theta, 0, EPS, GAIN, gy)
    worst = {}
    check("x.grad", xin.grad.cpu().numpy().reshape(2, 64, 64), bw["dx"], bw["A_dx"], worst)
    got = np.stack([getattr(model.frontend, n).grad.cpu().numpy() for n in NAMES])
    check("frontend.*.grad", got, bw["dtheta"], bw["A_dtheta"], worst)
    plain = make_model(sed, None)
    plain.load_state_dict({k: v for k, v in model.state_dict().items() if not k.startswith("frontend.")})
    yin = seen["y"].requires_grad_(True)
    crit(plain(yin), dev(tgt)).backward()
    torch.cuda.synchronize()
    for n, p in plain.named_parameters():
        assert torch.equal(p.grad, dict(model.named_parameters())[n].grad), n
    assert torch.equal(yin.grad, seen["g"])


def test_composition_with_the_trainer(sed):
    x, tgt = model_input()
    layer, theta = drawn_layer(sed)
    model = make_model(sed, layer)
    tr = sed.FusedTrainer(model, lr=1e-2, recall_factor=5.0)
    assert tr.flat.names[:4] == ["frontend." + n for n in NAMES]
    xd, yd = dev(x), dev(tgt)
    model.engine.timer = sed.engine.KernelTimer()
    loss = tr.forward_backward(xd, yd)
    torch.cuda.synchronize()
    names = [lbl.split(":")[0] for lbl, _, _ in model.engine.timer.records]
    model.engine.timer = None
    assert names[0] == "sed_pcen_fwd" and names[-1] == "sed_pcen_bwd" and "sed_conv3x3_c1_dgrad" in names, names
    assert np.isfinite(loss.item())
    plan = next(iter(model.engine._plans.values()))
    gy = plan.dx_in.cpu().numpy().reshape(2, 64, 64)
    bw = PF.backward(x.reshape(2, 64, 64), theta, 0, EPS, GAIN, gy)
    got = np.stack([tr.flat.G["frontend." + n].cpu().numpy() for n in NAMES])
    check("flat.G[frontend.*]", got, bw["dtheta"], bw["A_dtheta"], {})
    before = np.stack([tr.flat.P["frontend." + n].cpu().numpy() for n in NAMES])
    loss = tr.train_step(xd, yd)
    torch.cuda.synchronize()
    after = np.stack([tr.flat.P["frontend." + n].cpu().numpy() for n in NAMES])
    assert np.isfinite(loss.item()) and np.all(np.isfinite(after))
    for i, n in enumerate(NAMES):
        assert np.any(after[i] != before[i]), f"{n} did not move"
        assert getattr(model.frontend, n).data_ptr() == tr.flat.P["frontend." + n].data_ptr()
    sd = tr.state_dict()
    assert len(sd["state"]) == len(tr.flat.names) and sd["state"][0]["exp_avg"].shape == (64,)
    # a fixed layer: its forward only, and the step's own launches without the input gradient
    fixed, _ = drawn_layer(sed, trainable=False)
    m2 = make_model(sed, fixed)
    tr2 = sed.FusedTrainer(m2, lr=1e-2, recall_factor=5.0)
    assert not any(n.startswith("frontend.") for n in tr2.flat.names)
    tr2.train_step(xd, yd)
    m2.engine.timer = sed.engine.KernelTimer()
    loss2 = tr2.train_step(xd, yd)
    torch.cuda.synchronize()
    names2 = [lbl.split(":")[0] for lbl, _, _ in m2.engine.timer.records]
    assert names2[0] == "sed_pcen_fwd" and "sed_pcen_bwd" not in names2 and "sed_conv3x3_c1_dgrad" not in names2, names2
    assert np.isfinite(loss2.item())
    # and the same launches as a model without a layer, the layer's forward aside
    m3 = make_model(sed, None)
    tr3 = sed.FusedTrainer(m3, lr=1e-2, recall_factor=5.0)
    tr3.train_step(xd, yd)
    m3.engine.timer = sed.engine.KernelTimer()
    tr3.train_step(xd, yd)
    torch.cuda.synchronize()
    assert names2[1:] == [lbl.split(":")[0] for lbl, _, _ in m3.engine.timer.records]


def test_refusals_on_the_device(sed, tmp_path, monkeypatch):
    layer, _ = drawn_layer(sed)
    model = make_model(sed, layer)
    before = [p.data_ptr() for p in model.parameters()]
    with pytest.raises(RuntimeError, match="graph=True"):
        sed.FusedTrainer(model, lr=1e-3, graph=True)
    with pytest.raises(RuntimeError, match="mean_teacher"):
        sed.FusedTrainer(model, lr=1e-3, mean_teacher=True)
    import torch.distributed as dist
    assert not dist.is_initialized()
    monkeypatch.setenv("SED_DDP_FORCE", "1")
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'store'}", rank=0, world_size=1)
    try:
        with pytest.raises(RuntimeError, match="single process"):
            sed.FusedTrainer(model, lr=1e-3)
    finally:
        dist.destroy_process_group()
        monkeypatch.delenv("SED_DDP_FORCE")
    assert before == [p.data_ptr() for p in model.parameters()]
    x, tgt = model_input()
    assert np.isfinite(sed.FusedTrainer(model, lr=1e-3).train_step(dev(x), dev(tgt)).item())      # and is as usable as before


def test_no_frontend_adds_nothing(sed):
    """A model without a layer: the same bits as an engine forward called directly on the same input and parameters"""
    x, _ = model_input()
    model = make_model(sed, None, seed=3).eval()
    assert model.frontend is None
    xd = dev(x)
    model.engine.timer = sed.engine.KernelTimer()
    with torch.no_grad():
        out = model(xd).clone()
    torch.cuda.synchronize()
    names = [lbl.split(":")[0] for lbl, _, _ in model.engine.timer.records]
    model.engine.timer = None
    assert names and not [n for n in names if "pcen" in n], names
    plan = model.engine.forward(xd, model._tensor_dict(), training=False)
    direct = model.engine.interpolate(plan)
    torch.cuda.synchronize()
    assert torch.equal(out, direct)
