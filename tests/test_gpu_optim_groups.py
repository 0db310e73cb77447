"""GPU: the grouped optimizer step (sed_adam_groups_step: parameter groups with their own learning-rate scale and weight decay,
frozen groups, a warm-up + decay schedule evaluated on the device), the clipping norm over the non-frozen groups
(sed_grad_norm_groups) and FusedTrainer(lr_schedule=, param_groups=) built on them, per element against float64.

Reference: tests/optim_formula.py (float64 numpy; tests/test_optim_groups_host.py holds it to torch.optim.Adam / AdamW with real
param_groups and to LambdaLR at 1e-12) on float64 copies of the very fp32 state the kernel reads, one step at a time (no
compounding).  No kernel of this library serves as a reference, except where the property IS equality with an existing kernel
(section 3).  Outputs live in NaN-filled buffers with canaries on both sides.

Gate, per element, as tests/test_gpu_optimizer_ext.py has it -- the derivations apply unchanged and are re-stated here: |got - ref| <=
bound, u = 2^-24 per fp32 rounding, every operation count multiplied by SAFE = 4; nothing was set from a measurement.
  schedule hyper[0] = (float)lr(s), hyper[2] = (float)lr(s + 1): one fp32 rounding of the float64 value, 2^-24 relative, doubled to
           2^-23 for a device cos / pow that lands on the other side of a rounding tie.  gh[g] likewise.
  norm     fp64 accumulation of the squares of the fp32 products g * grad_scale (exact for the power-of-two scales used), one
           rounding of the square root to fp32: within 1 fp32 ulp of the float64 norm over the non-frozen elements.  The partial sums
           are per tile, not per 1024-element stride as sed_grad_norm's, so the two kernels add in different orders: bit equality with
           sed_grad_norm on a buffer whose frozen slices were zeroed by hand is not claimed, the ulp gate is the check.
  coef     min(1, max_norm / (norm + 1e-6f)) in fp32: bit for bit the numpy-float32 expression of the kernel's own norm.  Against
           the float64 reference its relative error is the norm's ulp (2u), the rounding of g * grad_scale (u), the sum with
           1e-6f (u), 1e-6f against 1e-6 (< u), the quotient (u), and the product grad_scale * coef (u): 7u.
  gr       the gradient that enters m and v: G = |g s coef| + wd |p| (L2 form) takes the place of |g s| in the bounds below, and
           its extra error eg = 7u |g s coef| (a clip factor) + 2u G (L2: the product wd * p and the sum) is propagated.
  m        m' = m + (1-b1)(gr - m): 5 roundings (20u) of |m| + (1-b1)(G + |m|), plus (1-b1) eg.
  v        v' = b2 v + (1-b2) gr^2: 6 roundings (24u), plus (1-b2)(2 G eg + eg^2).  vmax' = max: v's bound.
  p        decoupled: p (1 - lr wd), the factor rounded once and the product once: 2 roundings (8u) of |p|.  Then p' = p - ss m' /
           (sqrt(d) isb + eps), d = vmax' (amsgrad) or v': m's and d's bounds propagated through the quotient (the square root's
           with its steeper, lower side), plus 8 roundings (32u) of the update and 1 (4u) of |p| + |update|.
           The only roundings the grouped step adds are the fp64 -> fp32 ones of gh[g] = {lr scale / (1 - b1^s), 1 - lr scale wd}:
           the counts above already hold one for step_size and one for the decay factor.
  exact    frozen tiles (NaN gradients planted in them), padding lanes (zeros stay zeros), the reduction to sed_adam_step_ex_dev,
           two runs of the norm, eager against graph steps, the resume from a state_dict, canaries, untouched vmax.

Max err / gate is printed per check with -s and summarised at the end of the module.
"""
import importlib
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import optim_formula as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SAFE = 4.0
GUARD = 1024
CANARY = {torch.float32: -1024.0, torch.float64: -1024.0, torch.int32: 0x5A5A5A5A}
RATIOS = {}
PKG = "soundeventdetection-pytorch_amd"
SIZES = [1, 3, 4, 5, 4 * 1024 - 1, 4 * 1024, 4 * 1024 + 1, 8 * 1024 + 4]
GROUP_OF_PARAM = [0, 1, 2, 3, 0, 1, 2, 3]
KIND_ID = {"const": 0, "step": 1, "cosine": 2, "linear": 3, "invsqrt": 4}


def f32(x):
    """a python float rounded to fp32 (what a float argument of the C ABI, or a row of the group table, carries)"""
    return float(np.float32(x))


B1, B2, EPS_A = f32(0.9), f32(0.999), f32(1e-8)
WD = f32(1e-2)
SPECS = [(1.0, WD, False), (f32(0.1), 0.0, False), (2.5, f32(3 * WD), False), (1.0, WD, True)]


@pytest.fixture(scope="module")
def sed():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)


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


def close23(got, ref):
    """|got - ref| <= 2^-23 |ref|"""
    return abs(float(got) - ref) <= 2.0 ** -23 * abs(ref)


# ---- the layout: the host test's parameter sizes in four interleaved groups ------------------------------------------------------
@pytest.fixture(scope="module")
def layout(sed):
    tr = sed.train
    names = [f"p{i}" for i in range(len(SIZES))]
    offsets, off = {}, 0
    for n, k in zip(names, SIZES):
        offsets[n] = off
        off += (k + 3) // 4 * 4
    flat = SimpleNamespace(names=names, offsets=offsets, numel=off, P={n: torch.empty(k) for n, k in zip(names, SIZES)})
    tiles, groups = tr.build_tiles(flat, GROUP_OF_PARAM, SPECS)
    elem_group = np.zeros(off, dtype=np.int64)
    real = np.zeros(off, dtype=bool)                                      # False on the padding lanes
    for n, k, g in zip(names, SIZES, GROUP_OF_PARAM):
        elem_group[offsets[n]:offsets[n] + (k + 3) // 4 * 4] = g
        real[offsets[n]:offsets[n] + k] = True
    t = torch.from_numpy(tiles).cuda()
    assert [int(v) for v in t[:, 2].tolist()] == [0, 1, 2, 3, 0, 1, 2, 2, 3, 3, 3]       # neighbours differ wherever a parameter ends
    return SimpleNamespace(n=off, tiles=t, groups=torch.from_numpy(groups).cuda(), nt=tiles.shape[0], ng=4, elem_group=elem_group,
                           real=torch.from_numpy(real).cuda(), frozen=torch.from_numpy(elem_group == 3).cuda(), flat=flat)


def _groups_step(L, p, g, m, v, x, n, tiles, nt, groups, ng, gh, hyper, step, base_lr, sched, gs=1.0, dec=False, coef=None):
    P = L.ptr
    L.check(L.lib().sed_adam_groups_step(P(p), P(g), P(m), P(v), P(x), n, P(tiles), nt, P(groups), ng, P(gh), P(hyper), P(step),
                                         base_lr, KIND_ID[sched["kind"]], sched.get("warmup", 0), sched.get("total", 0),
                                         sched.get("every", 200), sched.get("gamma", 0.997), sched.get("floor", 0.0), B1, B2, EPS_A,
                                         gs, int(dec), P(coef), _stream()), "adam_groups_step")


# =================================================================================================================================
# 1. the schedule on the device
# =================================================================================================================================
SCHEDULES = [dict(kind="const"), dict(kind="step", every=4, gamma=0.5), dict(kind="cosine", total=9, floor=0.1),
             dict(kind="cosine", total=9), dict(kind="linear", total=9, floor=0.25), dict(kind="invsqrt")]


@pytest.mark.parametrize("warmup", [0, 1, 3])
@pytest.mark.parametrize("kw", SCHEDULES, ids=["const", "step", "cosine_floor", "cosine", "linear", "invsqrt"])
def test_schedule_on_the_device(L, kw, warmup):
    sched = dict(kw, warmup=warmup)
    base = 3e-3                                                           # a double that is no fp32 number
    G = Guards()
    p, g, m, v, x = (G.new(4, fill=0.0) for _ in range(5))
    g.fill_(0.25)
    tiles = torch.tensor([[0, 1, 0, 0]], dtype=torch.int32, device="cuda")
    rows = [(1.0, 0.0), (f32(0.1), f32(0.02)), (2.5, f32(0.03))]
    groups = torch.tensor([[s, w, 0.0, 0.0] for s, w in rows], dtype=torch.float32, device="cuda")
    gh, hyper, step = G.new(12), G.new(3), G.new(1, torch.int32, fill=0)
    total, every = sched.get("total", 0), sched.get("every", 200)
    # steps 1..12, then the counter set to just before and after `total` and to a multiple of `every` (and far out)
    starts = [(0, 12), (max(total - 2, 0), 4), (3 * every - 2, 4), (100000, 2)]
    for s0, count in starts:
        step.fill_(s0)
        for s in range(s0 + 1, s0 + count + 1):
            _groups_step(L, p, g, m, v, x, 4, tiles, 1, groups, 3, gh, hyper, step, base, sched)
            G.intact()
            assert int(step.item()) == s, "*step must advance by exactly 1"
            lr, nxt = F.lr_at(base, s, **sched), F.lr_at(base, s + 1, **sched)
            h = hyper.tolist()
            assert close23(h[0], lr) and close23(h[2], nxt), (sched, s, h, lr, nxt)
            assert close23(h[1], 1.0 / math.sqrt(1.0 - B2 ** s))
            for k, (sc, w) in enumerate(rows):
                row = gh[4 * k:4 * k + 4].tolist()
                assert close23(row[0], lr * sc / (1.0 - B1 ** s)) and close23(row[1], 1.0 - lr * sc * w) and row[2:] == [0.0, 0.0]
    if kw["kind"] == "cosine" and "floor" not in kw:
        step.fill_(total - 1)
        _groups_step(L, p, g, m, v, x, 4, tiles, 1, groups, 3, gh, hyper, step, base, sched)
        assert float(hyper[0]) == 0.0, "cos(pi) = -1: the rate at `total` without a floor is exactly 0"
    assert bool(torch.isfinite(p).all()) and float(p.abs().max()) > 0, "the element kernel ran with the scheduled rate"


# =================================================================================================================================
# 2. the update per element against float64
# =================================================================================================================================
def _state(n, seed, real, amsgrad=True):
    g = gen(seed)
    G = Guards()
    p, m, v, x = (G.new(n) for _ in range(4))
    p.copy_(torch.randn(n, device="cuda", generator=g) * real), m.copy_(torch.randn(n, device="cuda", generator=g) * 0.1 * real)
    v.copy_(torch.rand(n, device="cuda", generator=g) * 0.01 * real)
    r = torch.rand(n, device="cuda", generator=g)
    x.copy_(v * (1 + (r < 0.5) * torch.rand(n, device="cuda", generator=g)))
    if not amsgrad:
        x.fill_(-7.0)                                                     # must stay untouched
    return G, p, m, v, x, g


def bounds(p, gclip, m, v, m1, v1, d1, lr_e, wd_e, dec, step, clipped):
    """the per-element bounds of the module docstring (float64 tensors on the GPU); lr_e, wd_e: the element's group rate and decay"""
    pd, md, vd = p.double(), m.double(), v.double()
    l2 = torch.zeros_like(wd_e) if dec else wd_e
    Gm = gclip + l2 * pd.abs()
    eg = SAFE * U * ((7 * gclip if clipped else 0.0) + 2 * Gm * (l2 != 0))
    bm = SAFE * 5 * U * (md.abs() + (1 - B1) * (Gm + md.abs())) + (1 - B1) * eg
    bv = SAFE * 6 * U * (B2 * vd + (1 - B2) * Gm * Gm) + (1 - B2) * (2 * Gm * eg + eg * eg)
    ss, isb = lr_e / (1 - B1 ** step), 1.0 / math.sqrt(1 - B2 ** step)
    den = d1.sqrt() * isb + EPS_A
    bden = isb * (d1.sqrt() - (d1 - bv).clamp_min(0.0).sqrt())
    assert bool((bden < den).all())
    upd = ss * m1 / den
    pdec = pd * (1 - lr_e * wd_e) if dec else pd
    bu = ss * (bm / (den - bden) + m1.abs() * bden / (den * (den - bden))) + SAFE * 8 * U * upd.abs()
    bp = bu + SAFE * U * (pdec.abs() + upd.abs()) + (SAFE * 2 * U * pd.abs() * (wd_e != 0) if dec else 0.0)
    return bm, bv, bp


COSINE = dict(kind="cosine", warmup=3, total=8, floor=0.1)


@pytest.mark.parametrize("ams", [True, False], ids=["amsgrad", "plain"])
@pytest.mark.parametrize("dec", [False, True], ids=["l2", "decoupled"])
def test_update_per_element(L, layout, dec, ams):
    n, eg = layout.n, layout.elem_group
    base = 2e-3
    dev = "cuda"
    scale_e = torch.tensor([SPECS[k][0] for k in eg], dtype=torch.float64, device=dev)
    wd_e = torch.tensor([SPECS[k][1] for k in eg], dtype=torch.float64, device=dev)
    live, real = ~layout.frozen, layout.real
    tag = f"{'decoupled' if dec else 'l2'} {'amsgrad' if ams else 'plain'}"
    for ci, (coef_v, gs) in enumerate([(None, 1.0), (1.0, 0.5), (0.37, 1.0), (None, 0.5), (0.37, 0.5), (1.0, 1.0)]):
        G, p, m, v, x, g = _state(n, 100 + ci, real, ams)
        gh, hyper, step = G.new(16), G.new(3), G.new(1, torch.int32, fill=0)
        coef = None if coef_v is None else torch.tensor([coef_v], dtype=torch.float32, device=dev)
        cf = 1.0 if coef_v is None else f32(coef_v)
        fell = False
        for i in range(1, 6):
            gr = torch.randn(n, device=dev, generator=g) * (2.0 if i < 3 else 1e-2) * real
            gr[layout.frozen] = float("nan")                              # a frozen tile must not read its gradient into anything
            p0, m0, v0, x0 = p.clone(), m.clone(), v.clone(), x.clone()
            lr = F.lr_at(base, i, **COSINE)
            rp, rm, rv, rx = F.grouped_adam_step(p0.cpu().numpy(), gr.cpu().numpy(), m0.cpu().numpy(), v0.cpu().numpy(),
                                                 x0.cpu().numpy() if ams else None, eg, SPECS, lr, i, B1, B2, EPS_A, decoupled=dec,
                                                 coef=cf, grad_scale=gs)
            rp, rm, rv = (torch.from_numpy(a).to(dev) for a in (rp, rm, rv))
            d1 = torch.from_numpy(rx).to(dev) if ams else rv
            gclip = torch.where(live, (gr.double() * gs * cf).abs(), torch.zeros((), dtype=torch.float64, device=dev))
            bm, bv, bp = bounds(p0, gclip, m0, v0, rm, rv, d1, lr * scale_e, wd_e, dec, i, coef_v is not None)
            zero = torch.zeros_like(bm)
            bm, bv, bp = (torch.where(live, b, zero) for b in (bm, bv, bp))      # frozen: exactly the reference, which is the input
            _groups_step(L, p, gr, m, v, x if ams else None, n, layout.tiles, layout.nt, layout.groups, layout.ng, gh, hyper, step,
                         base, COSINE, gs=gs, dec=dec, coef=coef)
            G.intact()
            assert int(step.item()) == i
            gate(f"{tag}: m", m, rm, bm), gate(f"{tag}: v", v, rv, bv), gate(f"{tag}: p", p, rp, bp)
            if ams:
                gate(f"{tag}: vmax", x, d1, bv)
                fell = fell or float((v < x)[live & real].float().mean()) > 0.9
            else:
                assert bool((x == -7.0).all()), "amsgrad off must not touch vmax"
            for name, a, a0 in (("p", p, p0), ("m", m, m0), ("v", v, v0), ("vmax", x, x0)):
                assert torch.equal(a[layout.frozen].view(torch.int32), a0[layout.frozen].view(torch.int32)), f"frozen {name} changed"
                if name != "vmax" or ams:
                    assert bool((a[~real] == 0).all()), f"{name}: a padding lane is no longer zero"
            assert bool((p != p0)[live & real].float().mean() > 0.9), "the live groups were updated"
        assert fell or not ams, "the sequence must exercise v < vmax"
    # wd_g == 0 runs the expressions without a decay term: an infinite parameter of group 1 stays infinite, not NaN
    G, p, m, v, x, g = _state(n, 7, real, ams)
    gh, hyper, step = G.new(16), G.new(3), G.new(1, torch.int32, fill=0)
    o = layout.flat.offsets["p5"]
    p[o] = float("inf")
    gr = torch.randn(n, device=dev, generator=g) * real
    _groups_step(L, p, gr, m, v, x if ams else None, n, layout.tiles, layout.nt, layout.groups, layout.ng, gh, hyper, step, base,
                 COSINE, dec=dec)
    assert float(p[o]) == float("inf") and bool(torch.isfinite(p[o + 1:o + 64]).all())


# =================================================================================================================================
# 3. one group, a constant rate: the bits of sed_adam_step_ex_dev
# =================================================================================================================================
@pytest.mark.parametrize("ams", [True, False], ids=["amsgrad", "plain"])
@pytest.mark.parametrize("wdm", [0, 1, 2], ids=["wd0", "l2", "decoupled"])
def test_one_group_is_the_flat_device_step(L, layout, wdm, ams):
    lib, P, n = L.lib(), L.ptr, layout.n
    wd, dec, lr = (0.0 if wdm == 0 else WD), wdm == 2, f32(1e-3)
    tiles = layout.tiles.clone()
    tiles[:, 2] = 0
    groups = torch.tensor([[1.0, wd, 0.0, 0.0]], dtype=torch.float32, device="cuda")
    G, p, m, v, x, g = _state(n, 31 + wdm, layout.real, ams)
    G2, p2, m2, v2, x2, _ = _state(n, 31 + wdm, layout.real, ams)
    gh, hyper, step = G.new(4), G.new(3), G.new(1, torch.int32, fill=0)
    hyper2, step2 = G2.new(4), G2.new(1, torch.int32, fill=0)
    hyper2.copy_(torch.tensor([lr, float("nan"), float("nan"), float("nan")]))
    assert torch.equal(p, p2) and torch.equal(x, x2)
    for i in range(1, 6):
        gr = torch.randn(n, device="cuda", generator=g) * (2.0 if i < 3 else 1e-2)
        _groups_step(L, p, gr, m, v, x if ams else None, n, tiles, layout.nt, groups, 1, gh, hyper, step, lr, dict(kind="const"),
                     gs=0.5, dec=dec)
        L.check(lib.sed_adam_step_ex_dev(P(p2), P(gr), P(m2), P(v2), P(x2) if ams else None, n, P(hyper2), P(step2), B1, B2, EPS_A,
                                         0.5, 1.0, 0, wd, int(dec), None, _stream()), "ex_dev")
        G.intact(), G2.intact()
        for name, a, b in (("p", p, p2), ("m", m, m2), ("v", v, v2), ("vmax", x, x2)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"step {i}: {name} differs from sed_adam_step_ex_dev"
        assert int(step.item()) == int(step2.item()) == i and float(hyper[0]) == lr
        assert float(gh[0]) == float(hyper2[1]) and float(hyper[1]) == float(hyper2[2])


# =================================================================================================================================
# 4. the norm over the non-frozen groups
# =================================================================================================================================
def _norm_groups(L, layout, g, gs, max_norm):
    G = Guards()
    partial, out = G.new(layout.nt, torch.float64), G.new(2)
    L.check(L.lib().sed_grad_norm_groups(L.ptr(g), layout.n, L.ptr(layout.tiles), layout.nt, L.ptr(layout.groups), gs, max_norm,
                                         L.ptr(partial), L.ptr(out), _stream()), "grad_norm_groups")
    G.intact()
    return out.clone(), partial.clone()


@pytest.mark.parametrize("gs", [1.0, 0.5])
def test_grouped_norm(L, layout, gs):
    g = torch.randn(layout.n, device="cuda", generator=gen(5)) * 3.0
    g[layout.frozen] *= 1e3                                               # a norm that included them would be off by far
    ref = F.grouped_norm(g.cpu().numpy(), layout.elem_group, SPECS, gs)
    assert ref < 0.1 * float((g.double() * gs).norm())
    out, part = _norm_groups(L, layout, g, gs, 0.0)
    out2, part2 = _norm_groups(L, layout, g, gs, 0.0)
    assert torch.equal(out, out2) and torch.equal(part, part2), "two runs must give the same bits"
    frozen_tiles = (layout.tiles[:, 2] == 3)
    assert bool((part[frozen_tiles] == 0.0).all()) and bool((part[~frozen_tiles] > 0).all())
    r = abs(float(out[0]) - ref) / fp32_ulp(ref)
    RATIOS["grouped norm: err / fp32 ulp"] = max(RATIOS.get("grouped norm: err / fp32 ulp", 0.0), r)
    assert r <= 1.0 and float(out[1]) == 1.0, (float(out[0]), ref)
    # the same number, to the ulp, as sed_grad_norm on a buffer whose frozen slices are zero (another summation order)
    gz = torch.where(layout.frozen, torch.zeros_like(g), g)
    nparts = L.lib().sed_grad_norm_nparts(layout.n)
    pz, oz = torch.zeros(nparts, dtype=torch.float64, device="cuda"), torch.zeros(2, device="cuda")
    L.check(L.lib().sed_grad_norm(L.ptr(gz), layout.n, gs, 0.0, L.ptr(pz), nparts, L.ptr(oz), _stream()), "grad_norm")
    assert abs(float(oz[0]) - float(out[0])) <= fp32_ulp(ref)
    for max_norm in (f32(0.5 * ref), f32(2.0 * ref), f32(ref)):          # clipping, not clipping, at the edge
        o, _ = _norm_groups(L, layout, g, gs, max_norm)
        assert torch.equal(o[:1], out[:1])
        want = host_coef(o[0].item(), max_norm)
        assert np.float32(o[1].item()).tobytes() == np.float32(want).tobytes(), (gs, max_norm, o.tolist(), want)
    g2 = g.clone()
    g2[layout.frozen] = float("nan")                                      # frozen gradients are not read into the norm
    assert torch.equal(_norm_groups(L, layout, g2, gs, 0.0)[0], out)
    zero = torch.zeros_like(g)
    o, _ = _norm_groups(L, layout, zero, gs, 1.0)                         # torch: 1 / (0 + 1e-6) clamped to 1
    assert float(o[0]) == 0.0 and float(o[1]) == 1.0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_grouped_norm_nonfinite_propagates_like_torch(L, layout, bad):
    g = torch.randn(layout.n, device="cuda", generator=gen(9))
    o = layout.flat.offsets["p4"]
    g[o + 517] = bad
    out, _ = _norm_groups(L, layout, g, 1.0, 1.0)
    P = torch.nn.Parameter(torch.zeros(int((~layout.frozen).sum()), dtype=torch.float32))
    P.grad = g[~layout.frozen].cpu().clone()
    tn = torch.nn.utils.clip_grad_norm_([P], 1.0, error_if_nonfinite=False)
    tcoef = torch.clamp(1.0 / (tn + 1e-6), max=1.0)
    for got, want in ((out[0], tn), (out[1], tcoef)):
        assert (math.isnan(float(got)) and math.isnan(float(want))) or float(got) == float(want), (out.tolist(), tn, tcoef)


# =================================================================================================================================
# 5. the trainer
# =================================================================================================================================
import test_gpu_sa_model as T0                                            # noqa: E402  (its smallest model, batch and launch lists)

SCHED = dict(kind="cosine", warmup=3, total=8)
BASE_LR = 1e-3


def _fresh(sed, graph=False, **kw):
    tr = sed.train
    model = T0.make_model(sed, precision="bf16")
    groups = [{"params": ["conv_blocks"], "frozen": True}] + tr.no_decay_groups(model)
    t = sed.FusedTrainer(model, lr=BASE_LR, recall_factor=T0.W, graph=graph, weight_decay=1e-2, decoupled_weight_decay=True,
                         max_grad_norm=kw.pop("max_grad_norm", 0.05), lr_schedule=tr.LRSchedule(**SCHED), param_groups=groups, **kw)
    return model, t


def test_trainer_eager_graph_resume_and_state(sed):
    tr = sed.train
    x, y = T0.batch()
    m1, t1 = _fresh(sed)
    m2, t2 = _fresh(sed, graph=True)
    names = t1.flat.names
    frozen = [n for n in names if n.startswith("conv_blocks.")]
    assert frozen and t1.group_specs[1] == (1.0, f32(1e-2), True) and t1.group_specs[2] == (1.0, 0.0, False)
    for i, n in enumerate(names):
        want = 1 if n in frozen else (2 if t1.flat.P[n].ndim <= 1 else 0)
        assert t1.group_of[i] == want, n
    assert t1._gn_partial.numel() == t1._tiles.shape[0] and t1.lr == F.lr_at(BASE_LR, 1, **SCHED)
    p_init = t1.flat.p.clone()
    hist, snap = [], None
    for i in range(1, 7):               # eager against two eager steps, the capture, three replays
        l1 = t1.train_step(x, y).clone()
        l2 = t2.train_step(x, y).clone()
        assert torch.equal(l1, l2), (i, "the graph step's loss differs from the eager step's")
        assert torch.equal(t1.flat.p.view(torch.int32), t2.flat.p.view(torch.int32)), i
        assert torch.equal(t1.m, t2.m) and torch.equal(t1.v, t2.v) and torch.equal(t1.vmax, t2.vmax)
        assert torch.equal(t1.last_grad_norm, t2.last_grad_norm) and math.isfinite(float(t1.last_grad_norm)) and float(t1.last_grad_norm) > 0
        for t in (t1, t2):
            assert close23(t.last_lr, F.lr_at(BASE_LR, i, **SCHED)), (i, float(t.last_lr))
            assert t.lr == tr.lr_at(BASE_LR, i + 1, t.lr_schedule) == pytest.approx(F.lr_at(BASE_LR, i + 1, **SCHED), rel=1e-14)
            assert close23(t.hyper[2], F.lr_at(BASE_LR, i + 1, **SCHED)) and int(t.step_dev.item()) == i == t.step_count
        hist.append((l1, t1.flat.p.clone(), t1.m.clone(), t1.v.clone()))
        if i == 3:
            snap = ({k: v.clone() for k, v in m1.state_dict().items()}, t1.state_dict())
    assert len(t2._graphs) == 1 and not t1._graphs
    assert float((hist[-1][1] != p_init).float().mean()) > 0.1, "the live groups trained"
    for n in frozen:                    # bit-equal to their initial values, no optimizer state
        o, k = t1.flat.offsets[n], t1.flat.P[n].numel()
        for t in (t1, t2):
            assert torch.equal(t.flat.p[o:o + k].view(torch.int32), p_init[o:o + k].view(torch.int32)), n
            assert not t.m[o:o + k].any() and not t.v[o:o + k].any() and not t.vmax[o:o + k].any(), n
        assert float(t1.flat.g[o:o + k].abs().max()) > 0, "the backward of a frozen block still runs"
    t2._sync_host_scalars()
    assert t2.step_count == 6
    with pytest.raises(AttributeError):
        t1.lr = 1.0

    # state_dict: torch's multi-group layout, loadable into AdamW built with the same groups and back
    sd = t1.state_dict()
    pgs = sd["param_groups"]
    assert [g["frozen"] for g in pgs] == [False, True, False] and sorted(i for g in pgs for i in g["params"]) == list(range(len(names)))
    assert [g["weight_decay"] for g in pgs] == [f32(1e-2), f32(1e-2), 0] and all(g["decoupled_weight_decay"] and g["amsgrad"] for g in pgs)
    assert all(g["lr"] == t1.lr * g["lr_scale"] and g["initial_lr"] == BASE_LR * g["lr_scale"] for g in pgs)
    assert sd["lr_schedule"] == dict(t1.lr_schedule.as_dict(), base_lr=BASE_LR)
    assert set(sd["state"]) == {i for i, n in enumerate(names) if n not in frozen}
    params = [torch.nn.Parameter(q.detach().float().cpu().clone()) for q in m1.parameters()]
    topt = torch.optim.AdamW([{"params": [params[i] for i in g["params"]], "weight_decay": g["weight_decay"]} for g in pgs],
                             lr=123.0, amsgrad=True)
    topt.load_state_dict(sd)
    assert [g["lr"] for g in topt.param_groups] == [g["lr"] for g in pgs]
    live0 = next(i for i, n in enumerate(names) if n not in frozen)
    assert int(topt.state[params[live0]]["step"]) == 6 and all(params[names.index(n)] not in topt.state for n in frozen)
    o, k = t1.flat.offsets[names[live0]], params[live0].numel()
    assert torch.equal(topt.state[params[live0]]["exp_avg"].reshape(-1), t1.m[o:o + k].cpu())

    # resume after step 3: from the trainer's own state and from torch's renumbered one; steps 4..6 bit for bit
    t_at3 = torch.optim.AdamW([{"params": [params[i] for i in g["params"]]} for g in pgs], lr=1.0, amsgrad=True)
    t_at3.load_state_dict(snap[1])
    for state in (snap[1], t_at3.state_dict()):
        m3, t3 = _fresh(sed)
        m3.load_state_dict(snap[0])
        t3.load_state_dict(state)
        assert t3.step_count == 3 and int(t3.step_dev.item()) == 3 and t3.lr == F.lr_at(BASE_LR, 4, **SCHED)
        for i in (4, 5, 6):
            l3 = t3.train_step(x, y)
            assert torch.equal(l3, hist[i - 1][0]) and torch.equal(t3.flat.p.view(torch.int32), hist[i - 1][1].view(torch.int32)), i
            assert torch.equal(t3.m, hist[i - 1][2]) and torch.equal(t3.v, hist[i - 1][3]), i
    _, other = _fresh(sed)
    bad = dict(sd, param_groups=sd["param_groups"][:2])
    with pytest.raises(ValueError, match="parameter groups"):
        other.load_state_dict(bad)
    _, plain = _fresh(sed, amsgrad=False)
    with pytest.raises(ValueError, match="amsgrad"):
        plain.load_state_dict(sd)


def test_groups_without_a_schedule_run_the_reference_decay_in_closed_form(sed):
    x, y = T0.batch()
    model = T0.make_model(sed, precision="bf16")
    t = sed.FusedTrainer(model, lr=BASE_LR, recall_factor=T0.W, param_groups=[{"params": ["event_fc"], "lr_scale": 0.5}])
    assert t.lr_schedule.as_dict() == dict(kind="step", warmup=0, total=0, every=200, gamma=0.997, floor=0.0) and t.last_grad_norm is None
    t.step_dev.fill_(199)
    t.step_count = 199
    for s in (200, 201):
        t.train_step(x, y)
        want = BASE_LR * (1.0 if s == 200 else 0.997)
        assert close23(t.last_lr, want) and int(t.step_dev.item()) == s
    assert t.lr == BASE_LR * 0.997


def test_m5_takes_the_options(sed):
    """the raw-waveform model's engine sits on the same optimizer mixin: the options run there too (eager; graph=True stays refused)"""
    tr = sed.train
    g = torch.Generator().manual_seed(4)
    x, y = (0.1 * torch.randn(8, 1, 2048, generator=g)).cuda(), (torch.rand(8, generator=g) > 0.5).float().cuda()
    torch.manual_seed(0)
    model = sed.M5(1, precision="bf16").cuda()
    first = next(n for n, _ in model.named_parameters()).split(".")[0]
    sched = dict(kind="linear", warmup=2, total=6, floor=0.5)
    t = sed.FusedTrainer(model, lr=1e-3, recall_factor=5.0, lr_schedule=tr.LRSchedule(**sched), weight_decay=1e-2,
                         decoupled_weight_decay=True, max_grad_norm=1.0,
                         param_groups=[{"params": [first], "frozen": True}] + tr.no_decay_groups(model))
    p0 = t.flat.p.clone()
    for i in (1, 2, 3):
        loss = t.train_step(x, y)
        assert math.isfinite(float(loss)) and close23(t.last_lr, F.lr_at(1e-3, i, **sched)) and math.isfinite(float(t.last_grad_norm))
    changed = 0
    for i, n in enumerate(t.flat.names):
        o, k = t.flat.offsets[n], t.flat.P[n].numel()
        same = torch.equal(t.flat.p[o:o + k].view(torch.int32), p0[o:o + k].view(torch.int32))
        if t.group_of[i] == 1:
            assert same, f"frozen {n} changed"
        elif t.flat.P[n].ndim > 1:      # (a convolution bias in front of a BatchNorm has a zero gradient and stays where it is)
            assert not same, f"{n} was not updated"
        changed += not same
    assert changed > 0 and any(g == 1 for g in t.group_of)
    with pytest.raises(RuntimeError, match="graph=True"):
        sed.FusedTrainer(sed.M5(1, precision="bf16").cuda(), lr=1e-3, graph=True, lr_schedule=tr.LRSchedule("const"))


# =================================================================================================================================
# 6. the switch
# =================================================================================================================================
def test_unchanged_default_and_the_switch(sed):
    torch.manual_seed(0)
    assert T0.step_labels(sed, sed.Cnn_AvgPooling(3, T0.CFG, precision="bf16").cuda()) == T0.PLAIN_STEP
    x, y = T0.batch()
    legacy = ("sed_adam_amsgrad_step", "sed_adam_amsgrad_step_dev", "sed_grad_norm", "sed_adam_step_ex", "sed_adam_step_ex_dev")
    new = ("sed_grad_norm_groups", "sed_adam_groups_step")

    def run(**kw):
        model = T0.make_model(sed, precision="bf16")
        t = sed.FusedTrainer(model, lr=1e-3, recall_factor=T0.W, **kw)
        t.train_step(x, y)
        model.engine.timer = sed.engine.KernelTimer()
        t.train_step(x, y)
        torch.cuda.synchronize()
        return t, [lbl.split(":")[0] for lbl, _, _ in model.engine.timer.records]

    t, seen = run()
    assert seen[-1] == "sed_adam_amsgrad_step" and not set(seen) & set(new)
    assert t.last_lr is None and not hasattr(t, "hyper") and not hasattr(t, "_tiles") and t._grouped is None
    sd = t.state_dict()
    assert set(sd) == {"state", "param_groups"} and len(sd["param_groups"]) == 1
    assert set(sd["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable",
                                          "differentiable", "fused", "decoupled_weight_decay", "params"}
    assert sd["param_groups"][0]["params"] == list(range(len(t.flat.names))) and sd["param_groups"][0]["lr"] == t.lr == 1e-3
    t.lr = 5e-4
    assert t.lr == 5e-4
    t, seen = run(lr_schedule=sed.train.LRSchedule("const"))
    assert seen[-1] == "sed_adam_groups_step" and not set(seen) & set(legacy) and "sed_grad_norm_groups" not in seen
    t, seen = run(param_groups=[], max_grad_norm=1.0)
    assert seen[-2:] == ["sed_grad_norm_groups", "sed_adam_groups_step"] and not set(seen) & set(legacy)
