"""GPU: the gradient-norm kernel (sed_grad_norm), the extended optimizer step (sed_adam_step_ex / sed_adam_step_ex_dev: L2 or
decoupled weight decay, amsgrad on or off, a device-resident clip factor) and the FusedTrainer options built on them, per element
against float64.

Reference: torch.optim.Adam / torch.optim.AdamW (single-tensor form) and torch.nn.utils.clip_grad_norm_ on CPU float64 copies of
the very fp32 state the kernel reads, one step at a time (no compounding).  No kernel of this library serves as a reference, except
where the property IS equality with an existing kernel (section 3).  Outputs live in NaN-filled buffers with canaries on both sides.

Gate, per element, as tests/test_gpu_ops_exact_oracle.py does for Adam: |got - ref| <= bound, u = 2^-24 per fp32 rounding, every
operation count multiplied by SAFE = 4; nothing was set from a measurement.
  norm     fp64 accumulation of the squares of the fp32 products g * grad_scale (exact for the power-of-two scales used where the
           norm is gated), one rounding of the square root to fp32: within 1 fp32 ulp of the float64 norm.
  coef     min(1, max_norm / (norm + 1e-6f)) in fp32: bit for bit the numpy-float32 expression of the kernel's own norm.  Against
           the float64 reference its relative error is the norm's ulp (2u), the rounding of g * grad_scale (u), the sum with
           1e-6f (u), 1e-6f against 1e-6 (< u), the quotient (u), and the product grad_scale * coef (u): 7u.  min(1, .) does not
           amplify it.
  gr       the gradient that enters m and v: G = |g s coef| + wd |p| (L2 form) takes the place of |g s| in the bounds below, and
           its extra error eg = 7u |g s coef| (clipping) + 2u G (L2: the product wd * p and the sum) is propagated.
  m        m' = m + (1-b1)(gr - m): 5 roundings (20u) of |m| + (1-b1)(G + |m|), plus (1-b1) eg.
  v        v' = b2 v + (1-b2) gr^2: 6 roundings (24u), plus (1-b2)(2 G eg + eg^2).  vmax' = max: v's bound.
  p        decoupled: p (1 - lr wd), the factor rounded once and the product once: 2 roundings (8u) of |p|.  Then p' = p - ss m' /
           (sqrt(d) isb + eps), d = vmax' (amsgrad) or v': m's and d's bounds propagated through the quotient (the square root's
           with its steeper, lower side), plus 8 roundings (32u) of the update and 1 (4u) of |p| + |update|.
  device   against the host form on identical inputs: m bit-equal (same operations), v, vmax, p within the bounds above.
  exact    the reduction to sed_adam_amsgrad_step / _dev (weight_decay 0, coef NULL or 1.0f, vmax given), two runs of the norm, the
           graph replay against eager launches of the same kernels, the resume from a state_dict, canaries, untouched vmax.

The graph-mode test compares replays with EAGER launches of the device-scalar step (a graph=True trainer driven through
_step_dev without capture).  The host-scalar step of a graph=False trainer is a different kernel whose vectorised arithmetic
contracts differently (v differs in the last bit, as the existing host-against-device Adam gate records), so bit equality
between those two is not a property of this library, before or after this feature.

The m equality of the device row holds because the decay terms (wd * p, the sum with g s coef, p (1 - lr wd)) are rounded on
their own in the kernels: left to contraction, the vectorised host form fused gr + wd p one way and the scalar forms the other, and
m differed in the last bit from n = 4 on (the first size with a vector body).

Max err / gate is printed per check with -s and summarised at the end of the module.  Worst observed fractions on the MI355X, from
the one device run so far, which ended at that n = 4 mismatch (so n = 1 and 3 of every configuration, and the norm at every size):
norm 0.46 ulp; l2 m 0.04, v 0.06, vmax 0.06, p 0.21; no_amsgrad m 0.04, v 0.06, p 0.22; host vs device 0.  The same fp32 arithmetic emulated on the CPU (torch float32, no fused
multiply-adds, n = 1023, 25 steps) against this file's reference and bounds gave, per configuration: m 0.05-0.13, v 0.08-0.09,
vmax 0.07-0.09, p 0.17-0.25.
"""
import importlib
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SAFE = 4.0
GUARD = 1024
CANARY = {torch.float32: -1024.0, torch.float64: -1024.0, torch.int32: 0x5A5A5A5A}
RATIOS = {}
MAIN_CFG = [(32, 2), (64, 2), (128, 2), (128, 1)]


def f32(x):
    """a python float rounded to fp32 (what a float argument of the C ABI carries)"""
    return float(np.float32(x))


B1, B2, EPS_A = f32(0.9), f32(0.999), f32(1e-8)
ADAM_N = [1, 3, 4, 5, 1023, (1 << 20) | 3]
NORM_N = [1, 3, 5, 1023, (1 << 20) + 3, (1 << 22) + 5]


@pytest.fixture(scope="module")
def sed():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module("soundeventdetection-pytorch_amd")


@pytest.fixture(scope="module")
def L(sed):
    return sed._lib


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if RATIOS:
        print("\nmax err / gate by check (1.0 = at the derived bound)")
        for k in sorted(RATIOS):
            print(f"  {k:52s} {RATIOS[k]:.3e}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


class Guards:
    """output / workspace buffers: NaN inside (0 for int), a canary region on both sides, checked by intact()"""

    def __init__(self):
        self.bufs = []

    def new(self, n, dtype=torch.float32, fill=float("nan")):
        buf = torch.full((n + 2 * GUARD,), CANARY[dtype], dtype=dtype, device="cuda")
        inner = buf[GUARD:GUARD + n]
        inner.fill_(fill)
        self.bufs.append((buf, n, CANARY[dtype]))
        return inner

    def intact(self):
        torch.cuda.synchronize()
        for buf, n, can in self.bufs:
            assert bool((buf[:GUARD] == can).all()) and bool((buf[GUARD + n:] == can).all()), "write outside a buffer"


def gate(what, got, ref, bound):
    got, ref = got.double(), torch.as_tensor(ref, dtype=torch.float64, device=got.device)
    bound = torch.as_tensor(bound, dtype=torch.float64, device=got.device).expand_as(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: an element is NaN/inf (not written, or overflowed)"
    err = (got - ref).abs()
    pos = bound > 0
    exact_ok = bool((err[~pos] == 0).all())
    r = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    RATIOS[what] = max(RATIOS.get(what, 0.0), r)
    assert exact_ok, f"{what}: an element whose bound is 0 is not exactly the reference"
    assert r <= 1.0, f"{what}: max err/gate {r:.3e} > 1"


def fp32_ulp(x):
    """the spacing of fp32 numbers at |x| (a python float)"""
    _, e = math.frexp(max(abs(x), 2.0 ** -126))
    return 2.0 ** (e - 24)


def host_coef(norm32, max_norm):
    """clip_grad_norm_'s factor in fp32 from an fp32 norm, numpy arithmetic"""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6))
    return c if not (c > np.float32(1.0)) else np.float32(1.0)


# =================================================================================================================================
# 1. the norm kernel
# =================================================================================================================================
def _grad_norm(L, g, gs, max_norm):
    lib = L.lib()
    n = g.numel()
    nparts = lib.sed_grad_norm_nparts(n)
    assert 1 <= nparts <= 1024
    G = Guards()
    partial = G.new(nparts, torch.float64)
    out = G.new(2)
    L.check(lib.sed_grad_norm(L.ptr(g), n, gs, max_norm, L.ptr(partial), nparts, L.ptr(out), _stream()), "grad_norm")
    G.intact()
    assert bool(torch.isfinite(partial).all()) or not bool(torch.isfinite(g).all())
    return out.clone(), partial.clone()


@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("n", NORM_N)
def test_grad_norm(L, n, gs):
    g = torch.randn(n, device="cuda", generator=gen(n)) * 3.0
    ref = float((g.double().cpu() * gs).norm())
    out, part = _grad_norm(L, g, gs, 0.0)
    out2, part2 = _grad_norm(L, g, gs, 0.0)
    assert torch.equal(out, out2) and torch.equal(part, part2), "two runs must give the same bits"
    norm = float(out[0])
    r = abs(norm - ref) / fp32_ulp(ref)
    RATIOS["norm: err / fp32 ulp"] = max(RATIOS.get("norm: err / fp32 ulp", 0.0), r)
    assert r <= 1.0, (n, gs, norm, ref)
    assert float(out[1]) == 1.0, "max_norm <= 0 measures only"
    out_neg, _ = _grad_norm(L, g, gs, -1.0)
    assert float(out_neg[1]) == 1.0 and torch.equal(out_neg[:1], out[:1])
    for max_norm in (f32(0.5 * ref), f32(2.0 * ref), f32(ref)):          # clipping, not clipping, at the edge
        o, _ = _grad_norm(L, g, gs, max_norm)
        assert torch.equal(o[:1], out[:1])
        want = host_coef(o[0].item(), max_norm)
        assert np.float32(o[1].item()).tobytes() == np.float32(want).tobytes(), (n, gs, max_norm, o.tolist(), want)
    assert float(_grad_norm(L, g, gs, f32(0.5 * ref))[0][1]) < 1.0 and float(_grad_norm(L, g, gs, f32(2.0 * ref))[0][1]) == 1.0


@pytest.mark.parametrize("n", NORM_N)
def test_grad_norm_large_and_zero(L, n):
    big = torch.full((n,), 1e20, device="cuda")                           # squares overflow fp32
    out, _ = _grad_norm(L, big, 1.0, 1.0)
    ref = f32(1e20) * math.sqrt(n)
    assert math.isfinite(float(out[0])) and abs(float(out[0]) - ref) <= fp32_ulp(ref), (float(out[0]), ref)
    assert np.float32(out[1].item()).tobytes() == np.float32(host_coef(out[0].item(), 1.0)).tobytes()
    zero = torch.zeros(n, device="cuda")
    out, _ = _grad_norm(L, zero, 1.0, 0.0)
    assert float(out[0]) == 0.0 and float(out[1]) == 1.0
    out, _ = _grad_norm(L, zero, 1.0, 1.0)                                # torch: 1 / (0 + 1e-6) clamped to 1
    assert float(out[0]) == 0.0 and float(out[1]) == 1.0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_grad_norm_nonfinite_propagates_like_torch(L, bad):
    g = torch.randn(1023, device="cuda", generator=gen(9))
    g[517] = bad
    out, _ = _grad_norm(L, g, 1.0, 1.0)
    P = torch.nn.Parameter(torch.zeros(1023, dtype=torch.float32))
    P.grad = g.cpu().clone()
    tn = torch.nn.utils.clip_grad_norm_([P], 1.0, error_if_nonfinite=False)
    tcoef = torch.clamp(1.0 / (tn + 1e-6), max=1.0)
    for got, want in ((out[0], tn), (out[1], tcoef)):
        assert (math.isnan(float(got)) and math.isnan(float(want))) or float(got) == float(want), (out.tolist(), tn, tcoef)


# =================================================================================================================================
# 2. the extended step against torch.optim on CPU float64
# =================================================================================================================================
def ref_step(p, g, m, v, x, lr, step, gs, wd, dec, max_norm):
    """One torch.optim.Adam / AdamW step (after clip_grad_norm_) in float64 on the CPU from fp32 state; x None: amsgrad off.
    Returns refs and per-element bounds ((m, bm), (v, bv), (vmax, bv) or None, (p, bp)) on the GPU, the norm and the factor."""
    dev = p.device
    P = torch.nn.Parameter(p.double().cpu())
    P.grad = g.double().cpu() * gs
    cls = torch.optim.AdamW if dec else torch.optim.Adam
    opt = cls([P], lr=lr, betas=(B1, B2), eps=EPS_A, weight_decay=wd, amsgrad=x is not None, foreach=False)
    st = {"step": torch.tensor(float(step - 1)), "exp_avg": m.double().cpu(), "exp_avg_sq": v.double().cpu()}
    if x is not None:
        st["max_exp_avg_sq"] = x.double().cpu()
    opt.state[P] = st
    norm, coef = None, 1.0
    if max_norm is not None:
        norm = float(torch.nn.utils.clip_grad_norm_([P], max_norm, foreach=False))
        coef = min(1.0, max_norm / (norm + 1e-6))
    gclip = P.grad.abs().to(dev)                                          # |g s coef|
    opt.step()
    st = opt.state[P]
    m1, v1, p1 = st["exp_avg"].to(dev), st["exp_avg_sq"].to(dev), P.detach().to(dev)
    d1 = st["max_exp_avg_sq"].to(dev) if x is not None else v1
    pd, md, vd = p.double(), m.double(), v.double()
    l2 = wd if not dec else 0.0
    Gm = gclip + l2 * pd.abs()
    eg = SAFE * U * ((7 * gclip if max_norm is not None else 0.0) + (2 * Gm if l2 else 0.0))
    bm = SAFE * 5 * U * (md.abs() + (1 - B1) * (Gm + md.abs())) + (1 - B1) * eg
    bv = SAFE * 6 * U * (B2 * vd + (1 - B2) * Gm * Gm) + (1 - B2) * (2 * Gm * eg + eg * eg)
    ss, isb = lr / (1 - B1 ** step), 1.0 / math.sqrt(1 - B2 ** step)
    den = d1.sqrt() * isb + EPS_A
    bden = isb * (d1.sqrt() - (d1 - bv).clamp_min(0.0).sqrt())
    assert bool((bden < den).all())
    upd = ss * m1 / den
    pdec = pd * (1 - lr * wd) if dec else pd
    bu = ss * (bm / (den - bden) + m1.abs() * bden / (den * (den - bden))) + SAFE * 8 * U * upd.abs()
    bp = bu + SAFE * U * (pdec.abs() + upd.abs()) + (SAFE * 2 * U * pd.abs() if dec and wd else 0.0)
    return ((m1, bm), (v1, bv), (d1, bv) if x is not None else None, (p1, bp)), norm, coef


def _state(n, seed, amsgrad=True):
    g = gen(seed)
    G = Guards()
    p, m, v, x = (G.new(n) for _ in range(4))
    p.copy_(torch.randn(n, device="cuda", generator=g)), m.copy_(torch.randn(n, device="cuda", generator=g) * 0.1)
    v.copy_(torch.rand(n, device="cuda", generator=g) * 0.01)
    r = torch.rand(n, device="cuda", generator=g)
    x.copy_(v * (1 + (r < 0.5) * torch.rand(n, device="cuda", generator=g)))
    if not amsgrad:
        x.fill_(-7.0)                                                     # must stay untouched
    return G, p, m, v, x, g


def _grad_seq(g, n, steps=25):
    """the sequence of the existing Adam test -- large early gradients, then small ones, so that v falls below vmax -- with three
    ten times smaller still (steps 6, 13, 20): their norm is under half the median norm, so a clip at half the median leaves them"""
    return [torch.randn(n, device="cuda", generator=g) * (2.0 if i < 3 else (1e-3 if i % 7 == 6 else 1e-2)) for i in range(steps)]


CONFIGS = {                     # weight_decay, decoupled, amsgrad, clip, grad_scale
    "l2": (1e-2, False, True, False, 1.0 / 3.0),
    "decoupled": (1e-2, True, True, False, 1.0 / 3.0),
    "no_amsgrad": (0.0, False, False, False, 1.0 / 3.0),
    "clip": (0.0, False, True, True, 0.5),
    "all_l2": (1e-2, False, False, True, 0.5),
    "all_decoupled": (1e-2, True, False, True, 0.5),
}


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_ex_host_and_device_forms(L, n, cfg):
    lib, P, st = L.lib(), L.ptr, _stream()
    wd, dec, ams, clip, gs = CONFIGS[cfg]
    wd, gs, lr, lr_decay, decay_every = f32(wd), f32(gs), f32(1e-3), f32(0.5), 3
    G, p, m, v, x, g = _state(n, n + 11, ams)
    G2, p2, m2, v2, x2, _ = _state(n, n + 11, ams)                        # the device form, on the same inputs every step
    hyper = G2.new(4)
    hyper.copy_(torch.tensor([lr, float("nan"), float("nan"), float("nan")]))
    step = G2.new(1, torch.int32, fill=0)
    grads = _grad_seq(g, n)
    max_norm = None
    nparts = lib.sed_grad_norm_nparts(n)
    partial, out = G.new(nparts, torch.float64), G.new(2)
    coef = None
    if clip:
        norms = sorted(float((gr.double().cpu() * gs).norm()) for gr in grads)
        max_norm = f32(0.5 * norms[len(norms) // 2])
        coef = out[1:2]
    ref_coefs, got_coefs, fell = [], [], False
    for i, gr in enumerate(grads):
        refs, rnorm, rcoef = ref_step(p, gr, m, v, x if ams else None, lr, i + 1, gs, wd, dec, max_norm)
        for a, b in ((p2, p), (m2, m), (v2, v), (x2, x)):
            a.copy_(b)
        if clip:
            L.check(lib.sed_grad_norm(P(gr), n, gs, max_norm, P(partial), nparts, P(out), st), "grad_norm")
        xa, xb = (P(x), P(x2)) if ams else (None, None)
        L.check(lib.sed_adam_step_ex(P(p), P(gr), P(m), P(v), xa, n, lr, B1, B2, EPS_A, i + 1, gs, wd, int(dec), P(coef), st), "ex")
        L.check(lib.sed_adam_step_ex_dev(P(p2), P(gr), P(m2), P(v2), xb, n, P(hyper), P(step), B1, B2, EPS_A, gs, lr_decay,
                                         decay_every, wd, int(dec), P(coef), st), "ex_dev")
        G.intact(), G2.intact()
        if clip:
            assert abs(float(out[0]) - rnorm) <= fp32_ulp(rnorm), (i, float(out[0]), rnorm)
            ref_coefs.append(rcoef), got_coefs.append(float(out[1]))
        for name, host, devf, rb in zip(("m", "v", "vmax", "p"), (m, v, x, p), (m2, v2, x2, p2), refs):
            if rb is None:
                assert bool((host == -7.0).all()) and bool((devf == -7.0).all()), "amsgrad off must not touch vmax"
                continue
            gate(f"{cfg}: host {name}", host, rb[0], rb[1])
            gate(f"{cfg}: device {name}", devf, rb[0], rb[1])
            if name == "m":
                assert torch.equal(host, devf), "m: the host and device forms run the same operations"
            else:
                gate(f"{cfg}: host vs device {name}", host, devf.double(), rb[1])
        assert int(step.item()) == i + 1
        if ams:
            fell = fell or float((v < x).float().mean()) > 0.9
        if (i + 1) % decay_every == 0:
            lr = f32(lr * lr_decay)                                       # effective from the next step, on both sides
        assert float(hyper[0]) == lr
    assert fell or not ams or n < 16, "the sequence is meant to make v fall below vmax on (nearly) every element"
    if clip:
        assert any(c < 1.0 for c in ref_coefs) and any(c == 1.0 for c in ref_coefs), "the reference must clip some steps only"
        assert all((a < 1.0) == (b < 1.0) for a, b in zip(ref_coefs, got_coefs)), (ref_coefs, got_coefs)


def test_clip_engagement_of_the_sequence():
    """the property test_adam_ex_host_and_device_forms asserts of its reference, for every size, from the sequence alone"""
    for n in ADAM_N:
        _, _, _, _, _, g = _state(n, n + 11)
        norms = [float((gr.double().cpu() * 0.5).norm()) for gr in _grad_seq(g, n)]
        max_norm = f32(0.5 * sorted(norms)[len(norms) // 2])
        coefs = [min(1.0, max_norm / (nn + 1e-6)) for nn in norms]
        assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), (n, coefs)


# =================================================================================================================================
# 3. reduction to the existing kernels: the same bits
# =================================================================================================================================
@pytest.mark.parametrize("with_coef", [False, True], ids=["coef_null", "coef_one"])
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_ex_reduces_to_the_existing_kernels(L, n, with_coef):
    lib, P, st = L.lib(), L.ptr, _stream()
    gs, lr = f32(1.0 / 3.0), f32(1e-3)
    sets = [_state(n, n + 5) for _ in range(4)]                          # old host, new host, old device, new device
    hy = [torch.tensor([lr, 0.0, 0.0, 0.0], device="cuda") for _ in range(2)]
    sp = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2)]
    one = torch.ones(1, device="cuda") if with_coef else None
    g = sets[0][5]
    for i, gr in enumerate(_grad_seq(g, n, 8)):
        (_, p0, m0, v0, x0, _), (_, p1, m1, v1, x1, _), (_, p2, m2, v2, x2, _), (_, p3, m3, v3, x3, _) = sets
        L.check(lib.sed_adam_amsgrad_step(P(p0), P(gr), P(m0), P(v0), P(x0), n, lr, B1, B2, EPS_A, i + 1, gs, st))
        L.check(lib.sed_adam_step_ex(P(p1), P(gr), P(m1), P(v1), P(x1), n, lr, B1, B2, EPS_A, i + 1, gs, 0.0, 0, P(one), st))
        L.check(lib.sed_adam_amsgrad_step_dev(P(p2), P(gr), P(m2), P(v2), P(x2), n, P(hy[0]), P(sp[0]), B1, B2, EPS_A, gs, f32(0.5), 3,
                                              st))
        L.check(lib.sed_adam_step_ex_dev(P(p3), P(gr), P(m3), P(v3), P(x3), n, P(hy[1]), P(sp[1]), B1, B2, EPS_A, gs, f32(0.5), 3,
                                         0.0, 1, P(one), st))
        for s in sets:
            s[0].intact()
        for a, b in ((p0, p1), (m0, m1), (v0, v1), (x0, x1), (p2, p3), (m2, m3), (v2, v3), (x2, x3), (hy[0][:3], hy[1][:3]),
                     (sp[0], sp[1])):
            assert torch.equal(a, b), (i, "the extended step must reduce to the existing kernel bit for bit")


# =================================================================================================================================
# 4. FusedTrainer: the optimizer isolated from the model arithmetic
# =================================================================================================================================
def _model_and_batch(sed, kind):
    g = torch.Generator().manual_seed(4)
    if kind == "m5":
        make = lambda: sed.M5(1, precision="bf16")
        x = (0.1 * torch.randn(8, 1, 2048, generator=g)).cuda()
        y = (torch.rand(8, generator=g) > 0.5).float().cuda()
    else:
        if kind == "crnn":
            make = lambda: sed.Crnn_AvgPooling(1, MAIN_CFG, precision="bf16", gru_hidden=32)
        else:
            make = lambda: sed.Cnn_AvgPooling(1, MAIN_CFG, precision=kind.split("_")[1])
        x = torch.randn(2, 1, 16, 64, generator=g).cuda()
        y = (torch.rand(2, 16, 1, generator=g) < 0.3).float().cuda()
    return make, x, y


TRAINER_CASES = {               # model -> weight_decay, decoupled, amsgrad
    "cnn_fp32": (1e-2, False, True),
    "cnn_bf16": (1e-2, True, False),
    "crnn": (1e-2, True, True),
    "m5": (1e-2, False, False),
}


@pytest.mark.parametrize("kind", list(TRAINER_CASES))
def test_trainer_options_against_torch(sed, kind):
    wd, dec, ams = TRAINER_CASES[kind]
    make, x, y = _model_and_batch(sed, kind)
    lr = 1e-3

    def fresh(**kw):
        torch.manual_seed(0)
        mdl = make().cuda()
        return mdl, sed.FusedTrainer(mdl, lr=lr, recall_factor=5.0, **kw)

    _, probe = fresh()                                                    # the first step's norm, to clip at half of it
    probe.forward_backward(x, y)
    n0 = float(probe.flat.g.double().norm())
    assert math.isfinite(n0) and n0 > 0
    opts = dict(weight_decay=wd, decoupled_weight_decay=dec, amsgrad=ams, max_grad_norm=0.5 * n0)
    model, tr = fresh(**opts)
    assert (tr.vmax is None) == (not ams)
    lrf, clipped = f32(lr), 0
    for i in range(4):
        p, m, v = tr.flat.p.clone(), tr.m.clone(), tr.v.clone()
        xm = tr.vmax.clone() if ams else None
        tr.forward_backward(x, y)
        g = tr.flat.g.clone()
        refs, rnorm, rcoef = ref_step(p, g, m, v, xm, lrf, i + 1, 1.0, f32(wd), dec, f32(0.5 * n0))
        tr.optimizer_step()
        assert abs(float(tr.last_grad_norm) - rnorm) <= fp32_ulp(rnorm), (i, float(tr.last_grad_norm), rnorm)
        clipped += rcoef < 1.0
        for name, got, rb in zip(("m", "v", "vmax", "p"), (tr.m, tr.v, tr.vmax, tr.flat.p), refs):
            if rb is not None:
                gate(f"trainer {kind}: {name}", got, rb[0], rb[1])
    assert clipped >= 1, "half the first step's norm must clip the first step"
    # state_dict: torch's optimizer of the same options accepts it; a fresh trainer resumes with the same bits
    sd_opt = tr.state_dict()
    grp = sd_opt["param_groups"][0]
    assert grp["weight_decay"] == wd and grp["amsgrad"] is ams and grp["decoupled_weight_decay"] is dec
    assert ("max_exp_avg_sq" in sd_opt["state"][0]) == ams
    params = [torch.nn.Parameter(q.detach().cpu().clone()) for q in model.parameters()]
    topt = (torch.optim.AdamW if dec else torch.optim.Adam)(params, lr=123.0, weight_decay=wd, amsgrad=ams)
    topt.load_state_dict(sd_opt)
    assert topt.param_groups[0]["lr"] == pytest.approx(lr) and int(topt.state[params[0]]["step"]) == 4
    assert topt.param_groups[0]["weight_decay"] == wd and topt.param_groups[0]["amsgrad"] is ams
    sd_model = {k: t.clone() for k, t in model.state_dict().items()}
    model2, tr2 = fresh(**opts)
    model2.load_state_dict(sd_model)
    tr2.load_state_dict(topt.state_dict())
    assert tr2.step_count == 4
    tr.train_step(x, y), tr2.train_step(x, y)
    assert torch.equal(tr.flat.p, tr2.flat.p) and torch.equal(tr.m, tr2.m) and torch.equal(tr.v, tr2.v)
    assert torch.equal(tr.last_grad_norm, tr2.last_grad_norm)
    _, tr3 = fresh(amsgrad=not ams)
    with pytest.raises(ValueError, match="amsgrad"):
        tr3.load_state_dict(sd_opt)


def test_facade_takes_the_same_options(sed):
    torch.manual_seed(0)
    model = sed.Cnn_AvgPooling(1, [(4, 2), (8, 2), (8, 2), (8, 1)], precision="fp32").cuda().train()
    opt = sed.FusedAdamAmsgrad(model, lr=1e-3, weight_decay=1e-2, decoupled_weight_decay=True, amsgrad=False, max_grad_norm=1e-3)
    assert opt.vmax is None
    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(2, 1, 16, 64, generator=g).cuda(), (torch.rand(2, 16, 1, generator=g) < 0.3).float().cuda()
    sed.WeightedBCE(5, True)(model(x), y).backward()
    p, gflat = opt.flat.p.clone(), torch.zeros_like(opt.flat.g)
    for nme, q in model.named_parameters():
        o = opt.flat.offsets[nme]
        gflat[o:o + q.numel()] = q.grad.reshape(-1)
    refs, rnorm, rcoef = ref_step(p, gflat, opt.m.clone(), opt.v.clone(), None, f32(1e-3), 1, 1.0, f32(1e-2), True, f32(1e-3))
    opt.step()
    assert rcoef < 1.0 and abs(float(opt.last_grad_norm) - rnorm) <= fp32_ulp(rnorm)
    for name, got, rb in zip(("m", "v", "vmax", "p"), (opt.m, opt.v, None, opt.flat.p), refs):
        if rb is not None:
            gate(f"facade: {name}", got, rb[0], rb[1])


# =================================================================================================================================
# 5. graph mode, 6. defaults
# =================================================================================================================================
def test_graph_replay_with_options_matches_eager_launches(sed):
    cfg = [(4, 2), (8, 2), (8, 2), (8, 1)]
    opts = dict(max_grad_norm=1e-2, weight_decay=1e-2, decoupled_weight_decay=True)

    def fresh():
        torch.manual_seed(0)
        mdl = sed.Cnn_AvgPooling(1, cfg, precision="fp32").cuda()
        return mdl, sed.FusedTrainer(mdl, lr=1e-3, recall_factor=5.0, graph=True, **opts)

    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(4, 1, 30, 64, device="cuda", generator=g) for _ in range(5)]
    ys = [(torch.rand(4, 30, 1, device="cuda", generator=g) < 0.2).float() for _ in range(5)]
    m1, t1 = fresh()                                                      # eager launches of the device-scalar step
    m2, t2 = fresh()                                                      # 2 eager steps, the capture, 3 replays
    assert t2.hyper.numel() == 4
    coefs = []
    for i in range(5):
        t1._step_dev(xs[i], ys[i])
        t1._host_mirror()
        t2.train_step(xs[i], ys[i])
        assert len(t2._graphs) == (1 if i >= 2 else 0) and not t1._graphs
        assert torch.equal(t1.flat.p, t2.flat.p), f"step {i}: replayed parameters differ from the eager launches"
        assert torch.equal(t1.m, t2.m) and torch.equal(t1.v, t2.v) and torch.equal(t1.vmax, t2.vmax)
        assert torch.equal(t1.last_grad_norm, t2.last_grad_norm) and float(t2.last_grad_norm) > 0
        coefs.append(float(t2._coef))
    assert any(c < 1.0 for c in coefs), coefs
    host = (t2.step_count, t2.lr)
    t2._sync_host_scalars()
    assert (t2.step_count, f32(t2.lr)) == (host[0], f32(host[1])) == (5, f32(1e-3)) and int(t2.step_dev.item()) == 5


def test_default_trainer_launches_nothing_new(sed):
    cfg = [(4, 2), (8, 2), (8, 2), (8, 1)]
    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(2, 1, 16, 64, generator=g).cuda(), (torch.rand(2, 16, 1, generator=g) < 0.3).float().cuda()
    new = ("sed_grad_norm", "sed_adam_step_ex", "sed_adam_step_ex_dev")

    def names(**kw):
        torch.manual_seed(0)
        mdl = sed.Cnn_AvgPooling(1, cfg, precision="fp32").cuda()
        tr = sed.FusedTrainer(mdl, lr=1e-3, recall_factor=5.0, **kw)
        mdl.engine.timer = sed.engine.KernelTimer()
        for _ in range(2):
            tr.train_step(x, y)
        torch.cuda.synchronize()
        return tr, {lbl.split(":")[0] for lbl, _, _ in mdl.engine.timer.records}

    tr, seen = names()
    assert "sed_adam_amsgrad_step" in seen and not seen & set(new), seen
    assert tr._gn_out is None and tr.last_grad_norm is None and tr.vmax is not None
    tr, seen = names(decoupled_weight_decay=True)                         # without a decay there is nothing to decouple
    assert "sed_adam_amsgrad_step" in seen and not seen & set(new), seen
    tr, seen = names(max_grad_norm=1.0)
    assert {"sed_grad_norm", "sed_adam_step_ex"} <= seen and "sed_adam_amsgrad_step" not in seen, seen
    tr, seen = names(weight_decay=1e-2)
    assert "sed_adam_step_ex" in seen and "sed_grad_norm" not in seen and tr.last_grad_norm is None, seen
