"""GPU: sed_bce_sel_fwd_bwd / sed_frame_mse_fwd_bwd / sed_ema_update (csrc/sed_semi.hip) and sed_weak_bce_fwd_bwd_ex (csrc/sed_weak.hip)
through the C ABI, and the layers on top of them (CnnEngine.loss_and_grad(kind=, teacher_pre=), FusedTrainer(mean_teacher=), train()).

Reference: tests/semi_formula.py (float64; checked against torch autograd on the host in tests/test_semi_host.py).

Tolerance of a loss kernel, for loss and dpre: |got - ref| <= 2^-23 |ref| + 2^-40 s, the derived bound of tests/test_gpu_weak.py: the
kernels compute in double and round ONCE to fp32 (relative 2^-24); their double sums have at most a few thousand terms and go through
a few factors (relative 2^-40 of the scale s: the largest |ref| of the (b, k) row for dpre, the loss itself for the loss), which also
covers the cancellation in p - p_T, P - Y and 2 p_i - P.  sed_ema_update: 2^-23 |ref| (one rounding of a double result).
A sum of n terms that were accumulated in fp32 (the trainer's plan.loss / plan.dpre): the sum of the terms' bounds plus (n - 1)
fp32 additions, 2^-24 of the sum of the terms' magnitudes each.
Cells of unselected clips and of rows with c_i = 0 are compared with np.array_equal, to 0 or to the prior contents.
Every output lies in a sentinel-filled buffer between two canary regions; every input must be unmodified afterwards.

Worst error / bound seen on the MI355X (printed per check with -s): the three losses 0.499 (the fp32 rounding), the EMA 0.500, the
trainer's accumulated loss and dpre 0.457; sed_bce_sel_fwd_bwd against the fp32 kernel 0.019 (loss) and 0.168 (dpre) of that
kernel's bound.

One deviation from a literally exact zero: with a weak pooling the clip consistency term compares the student's pooled probability,
a double, with the teacher's, which sed_clip_pool_fwd has rounded to fp32; for a teacher that equals the student the term is
therefore not 0 but at most weight * 2^-48 (asserted).  The frame term is exactly 0.0, and so is the clip cell without a pooling."""
import importlib

import numpy as np
import pytest
import torch

from semi_formula import bce_sel, ema, frame_mse, weak_ex
from test_gpu_ops_exact_oracle import SAFE, TINY, U
from test_gpu_weak import K_CLASSES, W, Guards, batch, dev, frame_totals, label_slices, make_model, stream, targets, the_plan, within
from weak_formula import MODES, frame_counts

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
# (2, 125, 300): more than 256 classes, so label_slice of csrc/sed_weak.hip (the maxima of a strong target) takes a second pass over
# the classes, with 44 of its 256 threads live -- under every selection of SELS through sed_weak_bce_fwd_bwd_ex
SHAPES = [(1, 1, 1), (3, 5, 2), (3, 63, 1), (4, 65, 3), (2, 257, 14), (2, 64, 17), (2, 125, 300)]
SELS = ["null", "all", "none", "first", "alternating"]
ids = lambda s: "x".join(map(str, s))           # noqa: E731


@pytest.fixture(scope="module")
def sed():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def L(sed):
    return sed._lib


def selection(name, B):
    """None, or (B,) uint8 with nonzero values that are not all 1"""
    if name == "null":
        return None
    b = np.arange(B)
    m = {"all": b >= 0, "none": b < 0, "first": b == 0, "alternating": b % 2 == 0}[name]
    return (m * (1 + 37 * b)).astype(np.uint8)


def logits(rng, shape, saturated=False):
    if not saturated:
        return rng.normal(0.0, 3.0, shape).astype(np.float32)
    return rng.choice(np.array([40.0, -40.0, 800.0, -800.0], dtype=np.float32), size=shape)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(L, entry, pre, other, sel, ratio, Tt, weight=1.0, grad_scale=1.0, into=None, with_grad=True, mode=None, criterion=None):
    """one of the three loss entries through the C ABI into guarded buffers -> (loss float32, dpre (B, t, K) or None[, clip_prob]) as
    numpy.  into = (loss, dpre) numpy arrays: accumulate = 1 on top of them."""
    B, t, K = pre.shape
    lib = L.lib()
    g = Guards()
    d_pre, d_other = dev(pre), dev(other)
    d_sel = None if sel is None else dev(sel)
    loss = g.new(torch.float32, 1)
    dpre = g.new(torch.float32, B, t, K) if with_grad else None
    if into is not None:
        loss.copy_(torch.from_numpy(np.asarray(into[0]).reshape(1)))
        dpre.copy_(torch.from_numpy(into[1]))
    acc = 0 if into is None else 1
    clip = None
    if entry == "bce_sel":
        nws = lib.sed_bce_sel_ws_bytes(B, t, K)
        ws = g.new(torch.float64, nws // 8)
        L.check(lib.sed_bce_sel_fwd_bwd(L.ptr(d_pre), L.ptr(d_other), L.ptr(d_sel), L.ptr(loss), L.ptr(dpre), acc, B, t, K, ratio, Tt, W,
                                        weight, grad_scale, L.ptr(ws), stream()), entry)
    elif entry == "frame_mse":
        nws = lib.sed_frame_mse_ws_bytes(B, t, K)
        ws = g.new(torch.float64, nws // 8)
        L.check(lib.sed_frame_mse_fwd_bwd(L.ptr(d_pre), L.ptr(d_other), L.ptr(d_sel), L.ptr(loss), L.ptr(dpre), acc, B, t, K, ratio, Tt,
                                          weight, grad_scale, L.ptr(ws), stream()), entry)
    else:
        nws = lib.sed_weak_bce_ws_bytes(B, t, K)
        ws = g.new(torch.float64, nws // 8)
        clip = g.new(torch.float32, B, K)
        frames = other.shape[1] if other.ndim == 3 else 0
        L.check(lib.sed_weak_bce_fwd_bwd_ex(L.ptr(d_pre), L.ptr(d_other), frames, L.ptr(d_sel), criterion, L.ptr(clip), L.ptr(loss),
                                            L.ptr(dpre), acc, B, t, K, ratio, Tt, L.POOL_MODES[mode], W, weight, grad_scale, L.ptr(ws),
                                            stream()), entry)
    assert nws % 8 == 0 and nws >= 8
    g.intact()
    assert np.array_equal(bits(d_pre.cpu().numpy()), bits(pre)) and np.array_equal(bits(d_other.cpu().numpy()), bits(other)), "an input was modified"
    assert sel is None or np.array_equal(d_sel.cpu().numpy(), sel)
    out = [loss.cpu().numpy()[0], None if dpre is None else dpre.cpu().numpy()]
    if clip is not None:
        out.append(clip.cpu().numpy())
    for a in out:
        assert a is None or not np.isnan(a).any(), "an output cell was not written"
    return tuple(out)


def check_loss(got, ref, pre, sel, ratio, Tt, tag):
    """(loss, dpre) of a kernel against (loss, dpre) of the formula: the bound, and the cells that must be exactly 0"""
    within(got[0], ref[0], abs(ref[0]), (tag, "loss"))
    if got[1] is None:
        return
    within(got[1], ref[1], np.abs(ref[1]).max(axis=1, keepdims=True), (tag, "dpre"))
    zero = np.zeros(pre.shape, dtype=bool)
    _, c = frame_counts(pre.shape[1], ratio, Tt)
    zero[:, c == 0] = True
    if sel is not None:
        zero[sel == 0] = True
    assert np.array_equal(bits(got[1][zero]), np.zeros(int(zero.sum()), dtype=np.uint32)), (tag, "cells that must be exactly +0")
    if sel is not None and not sel.any():
        assert got[0] == 0.0 and not got[1].any(), (tag, "S = 0")


def check_accumulate(L, entry, alone, pre, other, sel, ratio, Tt, rng, tag, **kw):
    """accumulate = 1 on top of prior contents: prior + alone with ONE IEEE add per element; untouched cells keep the prior's bits"""
    prior = (np.float32(rng.normal()), rng.normal(0.0, 1.0, pre.shape).astype(np.float32))
    both = run(L, entry, pre, other, sel, ratio, Tt, 0.75, 0.5, into=prior, **kw)
    assert np.float32(prior[0] + alone[0]) == both[0], tag
    assert np.array_equal(bits(prior[1] + alone[1]), bits(both[1])), tag
    _, c = frame_counts(pre.shape[1], ratio, Tt)
    off = np.zeros(pre.shape, dtype=bool)
    off[:, c == 0] = True
    if sel is not None:
        off[sel == 0] = True
    assert np.array_equal(bits(both[1][off]), bits(prior[1][off])), (tag, "cells that must keep the prior's bits")
    if sel is not None and not sel.any():
        assert both[0] == prior[0] and np.array_equal(bits(both[1]), bits(prior[1])), (tag, "S = 0 leaves everything as it was")


def same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_shapes_reach_the_second_class_pass():
    """the last of SHAPES: two passes over the classes in label_slice, the second with 44 live classes, in 5 to 37 slices"""
    B, t, K = SHAPES[-1]
    cuts = [label_slices(min(t * r, Tt), K) for r in (1, 8) for Tt in frame_totals(t, r) if Tt >= r]
    assert all(c[3] == 2 for c in cuts) and K - 256 == 44 and (min(c[1] for c in cuts), max(c[1] for c in cuts)) == (5, 37)
    assert all(label_slices(min(s[1] * r, Tt), s[2])[3] == 1 for s in SHAPES[:-1] for r in (1, 8) for Tt in frame_totals(s[1], r))


# ---- the kernels against the formula ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [1, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_bce_sel_against_formula(L, shape, ratio):
    B, t, K = shape
    rng = np.random.default_rng(B * 100000 + t * 100 + K + ratio)
    for Tt in frame_totals(t, ratio):
        for saturated in (False, True):
            pre = logits(rng, shape, saturated)
            target = targets(rng, B, K, Tt)[1]
            for name in SELS:
                sel = selection(name, B)
                tag = ("bce_sel", shape, ratio, Tt, name, saturated)
                ref = bce_sel(pre, target, sel, ratio, Tt, W, 0.75, 0.5)
                got = run(L, "bce_sel", pre, target, sel, ratio, Tt, 0.75, 0.5)
                check_loss(got, ref, pre, sel, ratio, Tt, tag)
                if not saturated:
                    assert same_bits(got, run(L, "bce_sel", pre, target, sel, ratio, Tt, 0.75, 0.5)), (tag, "two runs")
                    check_accumulate(L, "bce_sel", got, pre, target, sel, ratio, Tt, rng, tag)
                    bare = run(L, "bce_sel", pre, target, sel, ratio, Tt, 0.75, 0.5, with_grad=False)
                    assert bare[1] is None and bare[0] == got[0]


@pytest.mark.parametrize("ratio", [1, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_frame_mse_against_formula(L, shape, ratio):
    B, t, K = shape
    rng = np.random.default_rng(B * 100000 + t * 100 + K + ratio + 1)
    for Tt in frame_totals(t, ratio):
        for saturated in (False, True):
            pre, pre_t = logits(rng, shape, saturated), logits(rng, shape, saturated)
            for name in SELS:
                sel = selection(name, B)
                tag = ("frame_mse", shape, ratio, Tt, name, saturated)
                ref = frame_mse(pre, pre_t, sel, ratio, Tt, 0.75, 0.5)
                got = run(L, "frame_mse", pre, pre_t, sel, ratio, Tt, 0.75, 0.5)
                check_loss(got, ref, pre, sel, ratio, Tt, tag)
                if not saturated:
                    assert same_bits(got, run(L, "frame_mse", pre, pre_t, sel, ratio, Tt, 0.75, 0.5)), (tag, "two runs")
                    check_accumulate(L, "frame_mse", got, pre, pre_t, sel, ratio, Tt, rng, tag)
        same = run(L, "frame_mse", pre, pre, None, ratio, Tt)             # a teacher that agrees: exactly nothing
        assert same[0] == 0.0 and not same[1].any()


@pytest.mark.parametrize("criterion", ["bce", "mse"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ratio", [1, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_weak_ex_against_formula(L, shape, ratio, mode, criterion):
    B, t, K = shape
    rng = np.random.default_rng(B * 100000 + t * 100 + K + ratio + 2)
    crit = {"bce": L.CRIT_BCE, "mse": L.CRIT_MSE}[criterion]
    kw = {"mode": mode, "criterion": crit}
    for Tt in frame_totals(t, ratio):
        for saturated in (False, True):
            pre = logits(rng, shape, saturated)
            clip_t, strong_t = targets(rng, B, K, Tt)
            target = strong_t if (Tt + saturated) % 2 else clip_t           # both kinds of target, alternating
            for name in SELS:
                sel = selection(name, B)
                tag = ("weak_ex", criterion, mode, shape, ratio, Tt, name, saturated, target.ndim)
                P, lref, dref = weak_ex(pre, target, sel, criterion, ratio, Tt, mode, W, 0.75, 0.5)
                got = run(L, "weak_ex", pre, target, sel, ratio, Tt, 0.75, 0.5, **kw)
                check_loss(got, (lref, dref), pre, sel, ratio, Tt, tag)
                within(got[2], P, np.abs(P), (tag, "clip_prob"))            # of every clip, selected or not
                if not saturated:
                    assert same_bits(got, run(L, "weak_ex", pre, target, sel, ratio, Tt, 0.75, 0.5, **kw)), (tag, "two runs")
                    check_accumulate(L, "weak_ex", got, pre, target, sel, ratio, Tt, rng, tag, **kw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_weak_ex_without_selection_is_the_weak_entry_bit_for_bit(L, shape, mode):
    """sed_weak_bce_fwd_bwd forwards to the _ex entry, so this guards the forwarding (argument order, NULL selection, criterion) and
    nothing more; that the shared kernels still give the bits of the commit before the selection was added is not something a
    test in this tree can see, and tests/test_gpu_weak.py's bounds are the standing guard."""
    B, t, K = shape
    rng = np.random.default_rng(7 + t)
    lib = L.lib()
    for ratio in (1, 8):
        for Tt in frame_totals(t, ratio):
            pre = logits(rng, shape)
            for target in targets(rng, B, K, Tt):
                ex = run(L, "weak_ex", pre, target, None, ratio, Tt, 0.75, 0.5, mode=mode, criterion=L.CRIT_BCE)
                d_pre, d_tgt = dev(pre), dev(target)
                clip, loss, dpre = torch.empty(B, K, device="cuda"), torch.empty(1, device="cuda"), torch.empty(B, t, K, device="cuda")
                ws = torch.empty(lib.sed_weak_bce_ws_bytes(B, t, K) // 8, dtype=torch.float64, device="cuda")
                L.check(lib.sed_weak_bce_fwd_bwd(L.ptr(d_pre), L.ptr(d_tgt), target.shape[1] if target.ndim == 3 else 0, L.ptr(clip),
                                                 L.ptr(loss), L.ptr(dpre), 0, B, t, K, ratio, Tt, L.POOL_MODES[mode], W, 0.75, 0.5, L.ptr(ws),
                                                 stream()), "weak_bce_fwd_bwd")
                assert same_bits(ex, (loss.cpu().numpy()[0], dpre.cpu().numpy(), clip.cpu().numpy())), (shape, mode, ratio, Tt)


@pytest.mark.parametrize("ratio", [1, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_bce_sel_with_every_clip_agrees_with_the_fp32_strong_kernel(L, shape, ratio):
    """within sed_bce_fwd_bwd's own bound (tests/test_gpu_ops_exact_oracle.py, 'bce'), taken about the float64 formula"""
    B, t, K = shape
    rng = np.random.default_rng(13 + t + ratio)
    lib = L.lib()
    for Tt in frame_totals(t, ratio):
        pre, target = logits(rng, shape), targets(rng, B, K, Tt)[1]
        lref, gref, gabs = bce_sel(pre, target, None, ratio, Tt, W, 1.0, 0.5, with_abs=True)
        numel = B * min(t * ratio, Tt) * K
        d_pre, d_tgt = dev(pre), dev(target)
        loss, dpre = torch.empty(1, device="cuda"), torch.empty(B, t, K, device="cuda")
        part = torch.empty((B * t * K + 255) // 256, device="cuda")
        L.check(lib.sed_bce_fwd_bwd(L.ptr(d_pre), L.ptr(d_tgt), L.ptr(loss), L.ptr(dpre), L.ptr(part), B, t, K, ratio, Tt, W, 0.5,
                                    stream()), "bce_fwd_bwd")
        for name in ("null", "all"):
            got = run(L, "bce_sel", pre, target, selection(name, B), ratio, Tt, 1.0, 0.5)
            bl = SAFE * (19 + ratio) * U * abs(lref) + TINY * (4 + 4 * ratio * W / numel)
            bg = SAFE * (12 + ratio) * U * gabs + (gabs > 0) * TINY * (4 + 0.5 + 4 * ratio * W * 0.5 / numel)
            el, eg = abs(float(loss.cpu()[0]) - float(got[0])), np.abs(dpre.cpu().numpy().astype(np.float64) - got[1])
            print(f"{(shape, ratio, Tt, name)}: worst error / bound loss {el / bl:.3f} dpre {float((eg / np.where(bg > 0, bg, 1)).max()):.3f}")
            assert el <= bl and (eg <= bg).all()


# ---- the EMA ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [(0, 0), (1, 1), (1, 0), (3, 2)], ids=str)
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 1027, 100003])
def test_ema_update(L, n, offset):
    """offset: floats by which the teacher's / the student's pointer is moved off its 16-byte aligned allocation"""
    rng = np.random.default_rng(n)
    lib = L.lib()
    for alpha in (0.0, 0.5, 0.999, 1.0):
        t0, s0 = rng.normal(0.0, 1.0, n).astype(np.float32), rng.normal(0.0, 1.0, n).astype(np.float32)
        g = Guards()
        tb, sb = g.new(torch.float32, n + 4), g.new(torch.float32, n + 4)
        tb.fill_(-7.0)
        sb.fill_(-9.0)
        tv, sv = tb[offset[0]:offset[0] + n], sb[offset[1]:offset[1] + n]
        if alpha in (0.0, 1.0):          # a copy and a no-op, whatever the values
            special = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0], dtype=np.float32)
            t0[:min(n, 5)], s0[-min(n, 5):] = special[:min(n, 5)], special[::-1][:min(n, 5)]
        tv.copy_(torch.from_numpy(t0))
        sv.copy_(torch.from_numpy(s0))
        assert tv.data_ptr() % 16 == 4 * offset[0] and sv.data_ptr() % 16 == 4 * offset[1]
        L.check(lib.sed_ema_update(L.ptr(tv), L.ptr(sv), n, alpha, stream()), "ema_update")
        g.intact()
        got = tv.cpu().numpy()
        if alpha not in (0.0, 1.0):
            ref = ema(t0, s0, alpha)
            err, bound = np.abs(got - ref), 2.0 ** -23 * np.abs(ref)
            print(f"ema {(n, offset, alpha)}: worst error / bound {float((err / np.where(bound > 0, bound, 1)).max()):.3f}")
            assert (err <= bound).all()
        if alpha == 0.0:
            assert np.array_equal(bits(got), bits(s0))
        if alpha == 1.0:
            assert np.array_equal(bits(got), bits(t0))
        assert np.array_equal(bits(sv.cpu().numpy()), bits(s0)), "the student buffer was modified"
        tb_h, sb_h = tb.cpu().numpy(), sb.cpu().numpy()           # the floats around the two views
        assert (np.delete(tb_h, np.s_[offset[0]:offset[0] + n]) == -7.0).all() and (np.delete(sb_h, np.s_[offset[1]:offset[1] + n]) == -9.0).all()


# ---- the layers ------------------------------------------------------------------------------------------------------------------
def within_sum(got, terms, tag):
    """got: fp32 accumulation of the terms (each (ref, s)) -- the module docstring's bound for a sum"""
    ref = sum(np.asarray(r, dtype=np.float64) for r, _ in terms)
    mag = sum(np.abs(np.asarray(r, dtype=np.float64)) for r, _ in terms)
    bound = sum(2.0 ** -23 * np.abs(np.asarray(r, dtype=np.float64)) + 2.0 ** -40 * np.asarray(s, dtype=np.float64) for r, s in terms)
    bound = bound + (len(terms) - 1) * 2.0 ** -24 * mag
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    print(f"{tag}: worst error / bound {float((err / np.where(bound > 0, bound, 1.0)).max()):.3f}")
    assert np.isfinite(np.asarray(got)).all() and (err <= bound).all(), tag


def row_scale(d):
    return np.abs(d).max(axis=1, keepdims=True)


def supervised_terms(pre, y, kind, ratio, mode, weak_weight):
    """[(loss, s)], [(dpre, s)] of the strong term over kind == 0 and the weak term over kind <= 1"""
    ls, ds = bce_sel(pre, y, None if kind is None else kind == 0, ratio, y.shape[1], W)
    _, lw, dw = weak_ex(pre, y, None if kind is None else kind <= 1, "bce", ratio, y.shape[1], mode, W, weak_weight)
    return [(ls, abs(ls)), (lw, abs(lw))], [(ds, row_scale(ds)), (dw, row_scale(dw))]


@pytest.mark.parametrize("model_kind", ["cnn", "crnn"])
def test_trainer_label_kinds(sed, model_kind):
    x, y = batch()
    yn = y.cpu().numpy()
    for kind in ([0, 1], [0, 0], [1, 2], [2, 2]):
        model = make_model(sed, model_kind)
        tr = sed.FusedTrainer(model, lr=1e-3, recall_factor=W, weak_pooling="linear", weak_weight=0.5)
        kd = torch.tensor(kind, device="cuda")
        loss = tr.forward_backward(x, y, kd).clone()
        plan = the_plan(model)
        pre = plan.pre.cpu().numpy()
        lt, dt = supervised_terms(pre, yn, np.array(kind), model.engine.ratio, "linear", 0.5)
        within_sum(loss.cpu().numpy()[0], lt, (model_kind, kind, "loss"))
        within_sum(plan.dpre.cpu().numpy(), dt, (model_kind, kind, "dpre"))
        assert bool(torch.isfinite(tr.flat.g).all())
        if kind == [0, 0]:               # every clip strongly labelled: the formula with every clip selected
            lt, dt = supervised_terms(pre, yn, None, model.engine.ratio, "linear", 0.5)
            within_sum(loss.cpu().numpy()[0], lt, (model_kind, "all", "loss"))
            within_sum(plan.dpre.cpu().numpy(), dt, (model_kind, "all", "dpre"))
        if kind == [2, 2]:
            assert float(loss) == 0.0 and not bool(plan.dpre.any())
    # without a weak pooling: the strong term alone, over the strong clips
    model = make_model(sed, model_kind)
    tr = sed.FusedTrainer(model, lr=1e-3, recall_factor=W)
    loss = tr.train_step(x, y, torch.tensor([1, 0], device="cuda")).clone()
    plan = the_plan(model)
    ls, ds = bce_sel(plan.pre.cpu().numpy(), yn, np.array([0, 1]), model.engine.ratio, 32, W)
    within(loss.cpu().numpy()[0], ls, abs(ls), (model_kind, "strong only", "loss"))
    within(plan.dpre.cpu().numpy(), ds, row_scale(ds), (model_kind, "strong only", "dpre"))
    assert not bool(plan.dpre[0].any())


@pytest.mark.parametrize("pooling", [None, "linear"])
@pytest.mark.parametrize("model_kind", ["cnn", "crnn"])
def test_mean_teacher_steps(sed, model_kind, pooling):
    train = importlib.import_module(PKG + ".train")
    x, y = batch()
    yn = y.cpu().numpy()
    kind = np.array([0, 1])
    kd = torch.tensor(kind, device="cuda")
    model = make_model(sed, model_kind)
    tr = sed.FusedTrainer(model, lr=1e-3, recall_factor=W, weak_pooling=pooling, weak_weight=0.5, mean_teacher=True, ema_decay=0.6,
                          consistency_weight=1.5, consistency_rampup=4)
    assert tr.teacher is not model and tr.teacher.engine is not model.engine and tr.teacher_flat.g is None
    assert torch.equal(tr.teacher_flat.p, tr.flat.p) and tr.teacher_flat.p.data_ptr() != tr.flat.p.data_ptr()
    ratio = model.engine.ratio
    teacher_prev = tr.teacher_flat.p.clone()
    for n in (1, 2, 3):
        loss = tr.forward_backward(x, y, kd).clone()
        plan, tplan = the_plan(model), the_plan(tr.teacher)
        pre, pre_t = plan.pre.cpu().numpy(), tplan.pre.cpu().numpy()
        cons = tr.last_consistency.cpu().numpy()
        cw = train.consistency_weight_at(n, 1.5, 4)
        if n == 1:                       # the teacher is a copy and saw the same input
            assert np.array_equal(bits(pre), bits(pre_t)) and cons[0] == 0.0
            assert cons[1] == 0.0 if pooling is None else 0.0 <= cons[1] <= cw * 2.0 ** -48
        if pooling is None:
            ls, ds = bce_sel(pre, yn, kind == 0, ratio, 32, W)
            lt, dt = [(ls, abs(ls))], [(ds, row_scale(ds))]
        else:
            lt, dt = supervised_terms(pre, yn, kind, ratio, pooling, 0.5)
        lf, df = frame_mse(pre, pre_t, None, ratio, 32, cw)
        within(cons[0], lf, abs(lf), (model_kind, pooling, n, "frame term"))
        lt.append((lf, abs(lf)))
        dt.append((df, row_scale(df)))
        if pooling is not None:
            tclip = plan.teacher_clip.cpu().numpy()
            Pt = weak_ex(pre_t, np.zeros((2, K_CLASSES)), None, "mse", ratio, 32, pooling, W)[0]
            within(tclip, Pt, np.abs(Pt), (model_kind, pooling, n, "teacher clip probabilities"))
            _, lc, dc = weak_ex(pre, tclip, None, "mse", ratio, 32, pooling, W, cw)
            if n == 3:                   # (before that the two models give the same logits and P - Y is a rounding residue)
                within(cons[1], lc, abs(lc), (model_kind, pooling, n, "clip term"))
            lt.append((lc, abs(lc)))
            dt.append((dc, row_scale(dc)))
        within_sum(loss.cpu().numpy()[0], lt, (model_kind, pooling, n, "loss"))
        within_sum(plan.dpre.cpu().numpy(), dt, (model_kind, pooling, n, "dpre"))
        tr.optimizer_step()
        assert tr.step_count == n
        student, teacher = tr.flat.p.cpu().numpy(), tr.teacher_flat.p.cpu().numpy()
        if n == 1:
            assert np.array_equal(bits(teacher), bits(student))
        ref = ema(teacher_prev.cpu().numpy(), student, train.ema_factor(n, 0.6))
        assert (np.abs(teacher - ref) <= 2.0 ** -23 * np.abs(ref)).all(), (model_kind, n, "the EMA recursion")
        teacher_prev = tr.teacher_flat.p.clone()
    assert train.ema_factor(3, 0.6) == 0.6 and not np.array_equal(teacher, student)
    # the teacher's BatchNorm buffers come from its own forwards
    tr.teacher._flush_counters()
    assert int(tr.teacher.conv_blocks[0].bn1.num_batches_tracked) == 3
    assert float(tr.teacher.conv_blocks[0].bn1.running_var.std()) > 0
    assert all(not p.requires_grad for p in tr.teacher.parameters())

    # checkpoint round trip: the teacher's bits come back; a checkpoint from before the teacher starts it as a copy of the student
    sd = tr.state_dict()
    assert set(sd) == {"state", "param_groups", "teacher"}
    kw = dict(lr=1e-3, recall_factor=W, weak_pooling=pooling, weak_weight=0.5, mean_teacher=True, ema_decay=0.6)
    model2 = make_model(sed, model_kind)
    model2.load_state_dict(model.state_dict())
    tr2 = sed.FusedTrainer(model2, **kw)
    tr2.load_state_dict(sd)
    assert tr2.step_count == 3 and torch.equal(tr2.teacher_flat.p, tr.teacher_flat.p) and torch.equal(tr2.flat.p, tr.flat.p)
    for (na, a), (nb, b) in zip(tr.teacher.state_dict().items(), tr2.teacher.state_dict().items()):
        assert na == nb and torch.equal(a, b), na
    assert tr2.teacher_flat.aliased()
    old = {k: v for k, v in sd.items() if k != "teacher"}
    tr3 = sed.FusedTrainer(make_model(sed, model_kind), **kw)
    tr3.model.load_state_dict(model.state_dict())
    tr3.load_state_dict(old)
    assert torch.equal(tr3.teacher_flat.p, tr3.flat.p) and torch.equal(tr3.flat.p, tr.flat.p)
    assert torch.equal(tr3.teacher.conv_blocks[0].bn1.running_mean, model.conv_blocks[0].bn1.running_mean)
    # a teacher_augment is applied to the teacher's input only
    seen = []
    tr2.teacher_augment = lambda t: (seen.append(t.shape), t.flip(2))[1]
    tr2.train_step(x, y)
    assert seen == [x.shape] and float(tr2.last_consistency[0]) > 0


def test_launch_lists(sed):
    x, y = batch()
    kd = torch.tensor([0, 1], device="cuda")

    def names(kind=None, **kw):
        mdl = make_model(sed, "cnn")
        tr = sed.FusedTrainer(mdl, lr=1e-3, recall_factor=W, **kw)
        step = (lambda: tr.train_step(x, y)) if kind is None else (lambda: tr.train_step(x, y, kind))
        step()                          # (first step: allocations)
        mdl.engine.timer = sed.engine.KernelTimer()
        step()
        torch.cuda.synchronize()
        return [lbl.split(":")[0] for lbl, _, _ in mdl.engine.timer.records]

    new = ("sed_bce_sel_fwd_bwd", "sed_weak_bce_fwd_bwd_ex", "sed_frame_mse_fwd_bwd", "sed_ema_update", "sed_clip_pool_fwd")
    off = dict(mean_teacher=False, ema_decay=0.5, consistency_weight=3.0, consistency_rampup=7)
    plain = names()
    assert plain.count("sed_bce_fwd_bwd") == 1 and not [n for n in plain if n in new or "weak" in n], plain
    assert names(**off) == plain
    i = plain.index("sed_bce_fwd_bwd")
    assert names(weak_pooling="mean", **off) == plain[:i + 1] + ["sed_weak_bce_fwd_bwd"] + plain[i + 1:]
    assert names(weak_pooling="mean", weak_only=True, **off) == plain[:i] + ["sed_weak_bce_fwd_bwd"] + plain[i + 1:]
    # the new options: the same step around other loss launches
    assert names(kd) == plain[:i] + ["sed_bce_sel_fwd_bwd"] + plain[i + 1:]
    assert names(kd, weak_pooling="mean") == plain[:i] + ["sed_bce_sel_fwd_bwd", "sed_weak_bce_fwd_bwd_ex"] + plain[i + 1:]
    assert names(kd, weak_pooling="mean", weak_only=True) == plain[:i] + ["sed_weak_bce_fwd_bwd_ex"] + plain[i + 1:]
    assert names(mean_teacher=True) == plain[:i + 1] + ["sed_frame_mse_fwd_bwd"] + plain[i + 1:] + ["sed_ema_update"]
    assert names(mean_teacher=True, weak_pooling="mean") == \
        plain[:i + 1] + ["sed_weak_bce_fwd_bwd", "sed_frame_mse_fwd_bwd", "sed_clip_pool_fwd", "sed_weak_bce_fwd_bwd_ex"] + plain[i + 1:] + \
        ["sed_ema_update"]


def test_refusals(sed, tmp_path, monkeypatch):
    x, y = batch()
    kd = torch.tensor([0, 1], device="cuda")
    with pytest.raises(RuntimeError, match="graph=True"):
        sed.FusedTrainer(make_model(sed, "cnn"), lr=1e-3, graph=True, mean_teacher=True)
    tr = sed.FusedTrainer(make_model(sed, "cnn"), lr=1e-3, recall_factor=W, graph=True)
    for step in (tr.train_step, tr.forward_backward):
        with pytest.raises(RuntimeError, match="graph=True"):
            step(x, y, kd)
    tr = sed.FusedTrainer(make_model(sed, "cnn"), lr=1e-3, recall_factor=W)
    for bad in (torch.tensor([0, 1]), torch.tensor([0.0, 1.0], device="cuda"), torch.tensor([0, 1, 2], device="cuda"),
                torch.tensor([True, False], device="cuda"), torch.tensor([[0, 1]], device="cuda")):
        with pytest.raises(ValueError, match="kind must be"):
            tr.forward_backward(x, y, bad)
    # a process group (a world-size-1 gloo group under the SED_DDP_FORCE hook stands in for the ranks): refused before the model is touched
    import torch.distributed as dist
    assert not dist.is_initialized()
    model = make_model(sed, "cnn")
    before = [p.data_ptr() for p in model.parameters()]
    monkeypatch.setenv("SED_DDP_FORCE", "1")
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'store'}", rank=0, world_size=1)
    try:
        with pytest.raises(RuntimeError, match="single-process"):
            sed.FusedTrainer(model, lr=1e-3, recall_factor=W, mean_teacher=True)
    finally:
        dist.destroy_process_group()
        monkeypatch.delenv("SED_DDP_FORCE")
    assert before == [p.data_ptr() for p in model.parameters()]
    sed.FusedTrainer(model, lr=1e-3, recall_factor=W, mean_teacher=True).train_step(x, y, kd)      # and is as usable as before
    m5 = sed.M5(1, precision="fp32").cuda()
    with pytest.raises(ValueError, match="no time axis"):
        sed.FusedTrainer(m5, lr=1e-3, mean_teacher=True)
    with pytest.raises(ValueError, match="label kinds"):
        sed.FusedTrainer(m5, lr=1e-3).train_step(torch.zeros(2, 1, 16000, device="cuda"), torch.zeros(2, 1, device="cuda"), kd)
    plan = the_plan(tr.model)
    with pytest.raises(ValueError, match="teacher_pre"):
        tr.engine.loss_and_grad(plan, y, W, teacher_pre=plan.pre[:, :1].contiguous(), consistency=1.0)
    with pytest.raises(ValueError, match="consistency"):
        tr.engine.loss_and_grad(plan, y, W, teacher_pre=plan.pre.clone())


def mixed_batch():
    """six clips, two of each kind; weak clips carry their clip label on every frame, unlabelled ones nothing"""
    x, y = batch()
    x = torch.cat([x, x.flip(2), x.roll(5, 2)])
    y = torch.cat([y, y.flip(1), y.roll(5, 1)])
    kind = torch.tensor([0, 1, 2, 0, 1, 2], device="cuda")
    y[kind == 1] = y[kind == 1].max(dim=1, keepdim=True).values.expand(-1, y.shape[1], -1)
    y[kind == 2] = 0.0
    return x.contiguous(), y.contiguous(), kind


def test_semi_supervised_training_lowers_the_loss(sed):
    x, y, kind = mixed_batch()
    torch.manual_seed(0)
    tr = sed.FusedTrainer(make_model(sed, "cnn"), lr=3e-3, recall_factor=W, weak_pooling="linear", mean_teacher=True, ema_decay=0.9,
                          consistency_weight=1.0, consistency_rampup=10)
    losses, cons = [], []
    for _ in range(31):
        losses.append(tr.train_step(x, y, kind).clone())
        cons.append(tr.last_consistency.clone())
    losses, cons = torch.stack(losses).cpu().numpy().reshape(-1), torch.stack(cons).cpu().numpy()
    assert np.isfinite(losses).all() and np.isfinite(cons).all() and losses[30] < losses[0], losses
    assert (cons >= 0).all() and cons[0, 0] == 0.0 and cons[5:, 0].min() > 0
    assert bool(torch.isfinite(tr.flat.p).all()) and bool(torch.isfinite(tr.teacher_flat.p).all())
    for _, b in tr.teacher.named_buffers():
        assert bool(torch.isfinite(b.float()).all())


def test_train_with_kinds_and_a_teacher(sed, tmp_path, monkeypatch):
    """train() takes (x, y, kind) batches, saves the teacher under 'teacher' beside the optimizer state, from where a trainer takes
    it back, and runs its periodic evaluation on the teacher under eval_teacher"""
    synthetic = importlib.import_module(PKG + ".dataset.synthetic")
    x, y, kind = mixed_batch()

    class Loader:
        batch_size = 6
        dataset = synthetic.SyntheticSedDataset(n_train_crops=1, crop=32, n_val=2, val_frames=64, mel_bins=64, classes=K_CLASSES)

        def __iter__(self):
            return iter([(x, y, kind.cpu()), (x, y, kind.cpu())])

    evaluated = []
    real_eval = sed.train.eval
    monkeypatch.setattr(sed.train, "eval", lambda model, *a, **kw: (evaluated.append(model), real_eval(model, *a, **kw))[1])
    torch.manual_seed(0)
    model = make_model(sed, "cnn")
    tr = sed.train.train(model, Loader(), sed.WeightedBCE(W, True), 4, 1e-3, 2, str(tmp_path), "cuda",
                         weak_pooling="linear", mean_teacher=True, ema_decay=0.5, consistency_rampup=3, eval_teacher=True)
    assert tr.step_count == 4 and tr.semi == (0.5, 2.0, 3) and tr.teacher is not None
    assert len(evaluated) == 2 and all(m is tr.teacher for m in evaluated) and tr.teacher is not model
    assert "val_loss" in open(tmp_path / "progress.jsonl").read()
    ck = torch.load(tmp_path / "checkpoints" / "iteration_4.pth", map_location="cuda")
    assert set(ck) == {"iterations", "model", "optimizer", "teacher"} and "teacher" not in ck["optimizer"]
    for k, v in tr.teacher.state_dict().items():
        assert torch.equal(ck["teacher"][k], v), k
    assert not torch.equal(ck["teacher"]["event_fc.weight"], ck["model"]["event_fc.weight"])
    # resuming from the file: the teacher comes back through load_state_dict's teacher argument
    model2 = make_model(sed, "cnn")
    model2.load_state_dict(ck["model"])
    tr2 = sed.FusedTrainer(model2, lr=1e-3, recall_factor=W, weak_pooling="linear", mean_teacher=True, ema_decay=0.5)
    tr2.load_state_dict(ck["optimizer"], teacher=ck["teacher"])
    assert tr2.step_count == 4 and torch.equal(tr2.teacher_flat.p, tr.teacher_flat.p) and not torch.equal(tr2.teacher_flat.p, tr2.flat.p)
    for k, v in tr.teacher.state_dict().items():
        assert torch.equal(tr2.teacher.state_dict()[k], v), k
    evaluated.clear()
    plain = sed.train.train(make_model(sed, "cnn"), Loader(), sed.WeightedBCE(W, True), 2, 1e-3, 2, str(tmp_path / "plain"), "cuda")
    assert plain.teacher is None and evaluated == [plain.model]
    assert set(torch.load(tmp_path / "plain" / "checkpoints" / "iteration_2.pth")) == {"iterations", "model", "optimizer"}
