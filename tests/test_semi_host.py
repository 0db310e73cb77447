"""Host side of semi-supervised training (no GPU): the tests' formulas (tests/semi_formula.py) against torch autograd in float64 on
masked inputs, the EMA and ramp-up schedules, every argument refusal of the new C-ABI entries through the built library, the option
checks, the CLI flags and the synthetic dataset's label kinds.  Every C-ABI refusal case passes NULL for a required pointer or a bad
value, so a validation bug would end in the null-pointer refusal and never in a launch."""
import ctypes as C
import importlib
import inspect
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from semi_formula import bce_sel, ema, ema_factor, frame_mse, rampup, weak_ex
from weak_formula import MODES, frame_counts

PKG = "soundeventdetection-pytorch_amd"
LIB = os.path.join(ROOT, PKG, "libsed_hip.so")
GEOMETRY = [(1, 7, 7), (1, 7, 5), (8, 5, 40), (8, 5, 37), (8, 5, 45), (8, 5, 3), (8, 1, 8)]       # ratio, t, Tt
SELECTIONS = [None, (1, 1, 1), (1, 0, 0), (0, 1, 1), (1, 0, 1)]


@pytest.fixture(scope="module")
def sed():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return importlib.import_module(PKG)


def close(got, ref, tag):
    """1e-12 relative: the loss as a number, the gradient element by element (relative to the element; an element that is exactly 0
    in the formula must be exactly 0 in autograd as well)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, tag
    assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref)), (tag, float(np.abs(got - ref).max()))


def mask_of(sel, B):
    return torch.ones(B, dtype=torch.float64) if sel is None else torch.tensor(sel, dtype=torch.float64)


def frames(x, ratio, N):
    return x.repeat_interleave(ratio, dim=1)[:, :N]


# ---- the formulas against autograd -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sel", SELECTIONS, ids=str)
@pytest.mark.parametrize("ratio,t,Tt", GEOMETRY)
def test_bce_sel_equals_autograd(ratio, t, Tt, sel):
    rng = np.random.default_rng(100 * ratio + 10 * t + Tt)
    B, K, w, weight, gs = 3, 2, 5.0, 0.75, 0.5
    pre = rng.uniform(-6.0, 6.0, (B, t, K))
    target = (rng.random((B, Tt, K)) > 0.7) * rng.uniform(0.5, 1.0, (B, Tt, K))
    loss, dpre = bce_sel(pre, target, sel, ratio, Tt, w, weight, gs)
    x = torch.tensor(pre, requires_grad=True)
    N = min(t * ratio, Tt)
    m = mask_of(sel, B)
    xf, y = frames(x, ratio, N), torch.tensor(target)[:, :N]
    l = -(w * y * torch.nn.functional.logsigmoid(xf) + (1.0 - y) * torch.nn.functional.logsigmoid(-xf))
    la = weight * (l * m[:, None, None]).sum() / (m.sum() * N * K)
    (la * gs).backward()
    close(loss, float(la.detach()), "loss")
    close(dpre, x.grad.numpy(), "dpre")
    _, c = frame_counts(t, ratio, Tt)
    assert not dpre[:, c == 0].any() and not dpre[~m.numpy().astype(bool)].any()


@pytest.mark.parametrize("sel", SELECTIONS, ids=str)
@pytest.mark.parametrize("ratio,t,Tt", GEOMETRY)
def test_frame_mse_equals_autograd(ratio, t, Tt, sel):
    rng = np.random.default_rng(100 * ratio + 10 * t + Tt + 1)
    B, K, weight, gs = 3, 2, 2.0, 0.25
    pre, pre_t = rng.uniform(-6.0, 6.0, (B, t, K)), rng.uniform(-6.0, 6.0, (B, t, K))
    loss, dpre = frame_mse(pre, pre_t, sel, ratio, Tt, weight, gs)
    x = torch.tensor(pre, requires_grad=True)
    xt = torch.tensor(pre_t, requires_grad=True)
    N = min(t * ratio, Tt)
    m = mask_of(sel, B)
    d = frames(torch.sigmoid(x), ratio, N) - frames(torch.sigmoid(xt), ratio, N).detach()
    la = weight * (d * d * m[:, None, None]).sum() / (m.sum() * N * K)
    (la * gs).backward()
    close(loss, float(la.detach()), "loss")
    close(dpre, x.grad.numpy(), "dpre")
    assert xt.grad is None                           # the teacher gets no gradient
    _, c = frame_counts(t, ratio, Tt)
    assert not dpre[:, c == 0].any() and not dpre[~m.numpy().astype(bool)].any()


def pooled(p, mode):
    if mode == "max":
        return p.max(dim=1).values
    if mode == "mean":
        return p.mean(dim=1)
    if mode == "linear":
        return (p * p).sum(dim=1) / p.sum(dim=1)
    return (p * torch.exp(p)).sum(dim=1) / torch.exp(p).sum(dim=1)


@pytest.mark.parametrize("criterion", ["bce", "mse"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sel", SELECTIONS, ids=str)
@pytest.mark.parametrize("ratio,t,Tt", GEOMETRY)
def test_weak_ex_equals_autograd(ratio, t, Tt, sel, mode, criterion):
    rng = np.random.default_rng(100 * ratio + 10 * t + Tt + MODES.index(mode))
    B, K, w, weight, gs = 3, 2, 5.0, 0.75, 0.5
    pre = rng.uniform(-6.0, 6.0, (B, t, K))
    strong = (rng.random((B, Tt, K)) > 0.7) * rng.uniform(0.5, 1.0, (B, Tt, K))
    clip = rng.random((B, K))
    if criterion == "mse":
        # a relative bound on dl/dP = 2 (P - Y) needs P - Y free of cancellation: binary frame labels (P lies in [0.0025, 0.9975]
        # for logits in [-6, 6]) and clip labels a quarter away from P, as a teacher that disagrees would give
        strong = (strong > 0).astype(np.float64)
        P0 = weak_ex(pre, clip, None, "mse", ratio, Tt, mode, w)[0]
        clip = np.where(P0 > 0.5, P0 - 0.25, P0 + 0.25)
    N = min(t * ratio, Tt)
    m = mask_of(sel, B)
    for target in (strong, clip):
        P, loss, dpre = weak_ex(pre, target, sel, criterion, ratio, Tt, mode, w, weight, gs)
        x = torch.tensor(pre, requires_grad=True)
        Pa = pooled(frames(torch.sigmoid(x), ratio, N), mode)
        y = torch.tensor(target)
        Y = y if y.dim() == 2 else y[:, :N].max(dim=1).values
        l = (Pa - Y) ** 2 if criterion == "mse" else -(w * Y * torch.log(Pa) + (1.0 - Y) * torch.log(1.0 - Pa))
        la = weight * (l * m[:, None]).sum() / (m.sum() * K)
        (la * gs).backward()
        close(P, Pa.detach().numpy(), "P")
        close(loss, float(la.detach()), "loss")
        close(dpre, x.grad.numpy(), "dpre")
        assert not dpre[~m.numpy().astype(bool)].any()


def test_nothing_selected_and_the_ema():
    rng = np.random.default_rng(3)
    pre, pre_t, target = rng.normal(0, 3, (2, 5, 3)), rng.normal(0, 3, (2, 5, 3)), rng.random((2, 37, 3))
    zero = np.zeros((2, 5, 3))
    assert bce_sel(pre, target, (0, 0), 8, 37, 5.0)[0] == 0.0 and np.array_equal(bce_sel(pre, target, (0, 0), 8, 37, 5.0)[1], zero)
    assert frame_mse(pre, pre_t, (0, 0), 8, 37)[0] == 0.0 and np.array_equal(frame_mse(pre, pre_t, (0, 0), 8, 37)[1], zero)
    for crit in ("bce", "mse"):
        P, loss, dpre = weak_ex(pre, target, (0, 0), crit, 8, 37, "linear", 5.0)
        assert loss == 0.0 and np.array_equal(dpre, zero) and P.shape == (2, 3)
    assert frame_mse(pre, pre, None, 8, 37)[0] == 0.0 and not frame_mse(pre, pre, None, 8, 37)[1].any()
    # all clips selected is the unselected loss
    assert bce_sel(pre, target, (1, 1), 8, 37, 5.0)[0] == bce_sel(pre, target, None, 8, 37, 5.0)[0]
    a, b = rng.normal(size=9), rng.normal(size=9)
    assert np.array_equal(ema(a, b, 0.0), b) and np.array_equal(ema(a, b, 1.0), a)
    assert np.array_equal(ema(a, b, 0.5), 0.5 * a + 0.5 * b)


# ---- the schedules ---------------------------------------------------------------------------------------------------------------
def test_schedules(sed):
    train = importlib.import_module(PKG + ".train")
    assert [train.ema_factor(n, 0.999) for n in (1, 2, 4, 1000)] == [0.0, 0.5, 0.75, 0.999]
    assert train.ema_factor(1001, 0.999) == 0.999 and train.ema_factor(3, 0.5) == 0.5 and train.ema_factor(10 ** 9, 0.0) == 0.0
    for n in range(1, 2100, 7):
        assert train.ema_factor(n, 0.999) == ema_factor(n, 0.999) == min(1.0 - 1.0 / n, 0.999)
    # with the factor 1 - 1/n the teacher is the plain mean of the students so far
    rng = np.random.default_rng(0)
    students = rng.normal(size=(6, 4))
    teacher = rng.normal(size=4)
    for n, s in enumerate(students, 1):
        teacher = ema(teacher, s, train.ema_factor(n, 0.999))
        np.testing.assert_allclose(teacher, students[:n].mean(axis=0), rtol=1e-14)
    assert train.consistency_weight_at(1, 2.0, 0) == 2.0 == train.consistency_weight_at(10 ** 6, 2.0, 0)
    for R in (1, 5, 100):
        ws = [train.consistency_weight_at(n, 2.0, R) for n in range(1, R + 3)]
        assert ws == [rampup(n, 2.0, R) for n in range(1, R + 3)]
        assert all(a < b for a, b in zip(ws[:R - 1], ws[1:R])) and ws[R - 1] == ws[R] == ws[R + 1] == 2.0
        assert ws[0] == 2.0 * math.exp(-5.0 * (1.0 - 1.0 / R) ** 2)


# ---- the C ABI refuses bad arguments before any launch ---------------------------------------------------------------------------
def test_argument_validation_without_gpu(sed):
    L = sed._lib
    lib = L.lib()
    assert (L.CRIT_BCE, L.CRIT_MSE) == (0, 1) and lib.sed_abi_version() == 1
    B, t, K, ratio, Tt = 2, 5, 3, 8, 37
    for fn in (lib.sed_bce_sel_ws_bytes, lib.sed_frame_mse_ws_bytes):
        assert fn(B, t, K) == 8 and fn(4, 750, 14) == 8 * ((4 * 750 * 14 + 255) // 256) and fn(0, t, K) == 0
    # host memory standing in for the device buffers: never touched, every call below is refused first
    pre, dpre, other = (C.c_float * (B * t * K))(), (C.c_float * (B * t * K))(), (C.c_float * (B * t * K))()
    target, clip, loss = (C.c_float * (B * Tt * K))(), (C.c_float * (B * K))(), (C.c_float * 1)()
    ws = (C.c_double * (B * K * 40))()
    sel = (C.c_ubyte * B)()
    A = C.addressof

    def refused(rc, word):
        assert rc != 0 and word in lib.sed_last_error(), (rc, word, lib.sed_last_error())

    def bce(pre_p=A(pre), target_p=A(target), sel_p=A(sel), loss_p=None, dpre_p=A(dpre), acc=0, B_=B, t_=t, K_=K, ratio_=ratio,
            Tt_=Tt, ws_p=A(ws)):
        return lib.sed_bce_sel_fwd_bwd(pre_p, target_p, sel_p, loss_p, dpre_p, acc, B_, t_, K_, ratio_, Tt_, 5.0, 1.0, 1.0, ws_p, None)

    def mse(pre_p=A(pre), other_p=A(other), sel_p=A(sel), loss_p=None, dpre_p=A(dpre), acc=0, B_=B, t_=t, K_=K, ratio_=ratio,
            Tt_=Tt, ws_p=A(ws)):
        return lib.sed_frame_mse_fwd_bwd(pre_p, other_p, sel_p, loss_p, dpre_p, acc, B_, t_, K_, ratio_, Tt_, 1.0, 1.0, ws_p, None)

    for call, second in ((bce, "target_p"), (mse, "other_p")):
        refused(call(), b"null")                    # everything valid but loss
        refused(call(sel_p=None, dpre_p=None), b"null")         # the optional pointers may be NULL: still stops at loss
        refused(call(pre_p=None, loss_p=A(loss)), b"null")
        refused(call(loss_p=A(loss), **{second: None}), b"null")
        refused(call(ws_p=None, loss_p=A(loss)), b"null")
        refused(call(ws_p=A(ws) + 4), b"null")
        for kw in ({"B_": 0}, {"t_": -2}, {"K_": 0}, {"ratio_": 0}, {"Tt_": 0}):
            refused(call(**kw), b"bad sizes")
        for acc in (-1, 2):
            refused(call(acc=acc), b"accumulate")
        refused(call(t_=1 << 20, ratio_=1 << 11), b"t * ratio")

    def weak(crit=0, sel_p=A(sel), loss_p=None, mode=2, acc=0, frames=Tt, pre_p=A(pre)):
        return lib.sed_weak_bce_fwd_bwd_ex(pre_p, A(target), frames, sel_p, crit, A(clip), loss_p, A(dpre), acc, B, t, K, ratio, Tt, mode,
                                           5.0, 1.0, 1.0, A(ws), None)

    for crit in (0, 1):
        refused(weak(crit), b"null")
        refused(weak(crit, sel_p=None), b"null")
        refused(weak(crit, pre_p=None, loss_p=A(loss)), b"null")
        refused(weak(crit, mode=4), b"mode")
        refused(weak(crit, acc=2), b"accumulate")
        refused(weak(crit, frames=Tt - 1), b"target_frames")
    for crit in (-1, 2, 7):
        refused(weak(crit), b"criterion")

    buf = (C.c_float * 8)()
    refused(lib.sed_ema_update(None, A(buf), 8, 0.5, None), b"needed")
    refused(lib.sed_ema_update(A(buf), None, 8, 0.5, None), b"needed")
    refused(lib.sed_ema_update(None, A(buf), 0, 0.5, None), b"needed")
    for alpha in (-0.1, 1.5, float("nan")):
        refused(lib.sed_ema_update(None, A(buf), 8, alpha, None), b"alpha")


# ---- Python-level refusals -------------------------------------------------------------------------------------------------------
def test_option_checks(sed):
    train = importlib.import_module(PKG + ".train")
    engine = importlib.import_module(PKG + ".engine")
    assert train.check_semi_options() is None
    assert train.check_semi_options(False, 7.0, -1.0, -3) is None                  # off: unused
    assert train.check_semi_options(True) == (0.999, 2.0, 0)
    assert train.check_semi_options(True, 0.0, 0, 10) == (0.0, 0.0, 10)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            train.check_semi_options(True, bad)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="consistency_weight"):
            train.check_semi_options(True, 0.999, bad)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="consistency_rampup"):
            train.check_semi_options(True, 0.999, 2.0, bad)
    m5 = sed.M5(1)
    cnn = sed.Cnn_AvgPooling(1, [(32, 2), (32, 2)])
    with pytest.raises(ValueError, match="no time axis"):
        train.check_semi_options(True, model=m5)
    with pytest.raises(ValueError, match="no time axis"):
        train.FusedTrainer(m5, 1e-3, mean_teacher=True)
    with pytest.raises(ValueError, match="no time axis"):
        train.train(m5, None, sed.WeightedBCE(5, False), 1, 1e-3, 1, "unused", "cuda", mean_teacher=True)
    assert train.check_semi_options(True, model=cnn) == (0.999, 2.0, 0)
    with pytest.raises(RuntimeError, match="graph=True"):
        train.FusedTrainer(cnn, 1e-3, graph=True, mean_teacher=True)
    with pytest.raises(ValueError, match="eval_teacher needs"):
        train.train(cnn, None, sed.WeightedBCE(5, True), 1, 1e-3, 1, "unused", "cuda", eval_teacher=True)
    with pytest.raises(ValueError, match="ema_decay"):
        train.train(cnn, None, sed.WeightedBCE(5, True), 1, 1e-3, 1, "unused", "cuda", mean_teacher=True, ema_decay=1.0)

    class Headless:
        conv_blocks = ()
        engine = type("E", (), {"head": "none"})()

    with pytest.raises(ValueError, match="classification head"):
        train.check_semi_options(True, model=Headless())

    defaults = {"mean_teacher": False, "ema_decay": 0.999, "consistency_weight": 2.0, "consistency_rampup": 0}
    for fn in (train.FusedTrainer.__init__, train.train):
        prm = inspect.signature(fn).parameters
        assert {n: prm[n].default for n in defaults} == defaults
    assert inspect.signature(train.train).parameters["eval_teacher"].default is False
    for fn in (train.FusedTrainer.train_step, train.FusedTrainer.forward_backward):
        assert inspect.signature(fn).parameters["kind"].default is None
    prm = inspect.signature(engine.CnnEngine.loss_and_grad).parameters
    assert [prm[n].default for n in ("weak", "kind", "teacher_pre", "consistency")] == [None] * 4


def test_mean_teacher_is_refused_under_a_process_group(sed, tmp_path, monkeypatch):
    """the trainer's collectives run on a group of more than one rank, or on any group under SED_DDP_FORCE=1 (the hook of
    tests/test_gpu_ddp.py): a world-size-1 gloo group stands in for the ranks.  The refusal comes before the teacher is made and
    before the model's parameters move into a flat buffer."""
    import torch.distributed as dist
    train = importlib.import_module(PKG + ".train")
    assert not dist.is_initialized()
    cnn = sed.Cnn_AvgPooling(1, [(32, 2), (32, 2)])
    before = [(n, p.data_ptr()) for n, p in cnn.named_parameters()]
    engine = cnn.engine
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'store'}", rank=0, world_size=1)
    try:
        monkeypatch.delenv("SED_DDP_FORCE", raising=False)
        assert not train.data_parallel_enabled()
        with pytest.raises(RuntimeError, match="on the GPU"):          # one rank, no hook: not data parallel; the CPU model is what stops it
            train.FusedTrainer(cnn, 1e-3, mean_teacher=True)
        monkeypatch.setenv("SED_DDP_FORCE", "1")
        assert train.data_parallel_enabled() and train.data_parallel_enabled(dist.group.WORLD)
        for kw in ({}, {"group": dist.group.WORLD}, {"weak_pooling": "linear"}):
            with pytest.raises(RuntimeError, match="single-process"):
                train.FusedTrainer(cnn, 1e-3, mean_teacher=True, **kw)
        with pytest.raises(RuntimeError, match="single-process"):
            train.train(cnn, None, sed.WeightedBCE(5, True), 1, 1e-3, 1, str(tmp_path / "out"), "cuda", mean_teacher=True)
        with pytest.raises(RuntimeError, match="on the GPU"):          # without a teacher the group is no obstacle
            train.FusedTrainer(cnn, 1e-3)
    finally:
        dist.destroy_process_group()
    assert before == [(n, p.data_ptr()) for n, p in cnn.named_parameters()] and cnn.engine is engine
    assert not train.data_parallel_enabled()
    # the command line: more than one rank in the environment
    main = importlib.import_module(PKG + ".main")
    argv = ["--train_features", "Spectogram", "--dataset_name", "synthetic", "--mean_teacher"]
    main.validate_args(main.build_full_parser().parse_args(argv))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="single-process"):
        main.validate_args(main.build_full_parser().parse_args(argv))
    main.validate_args(main.build_full_parser().parse_args(argv[:-1] + ["--label_kinds", "1:1:1"]))       # kinds alone are allowed


def test_clone_without_engines(sed):
    for model in (sed.Cnn_AvgPooling(2, [(32, 2), (32, 2)]), sed.Crnn_AvgPooling(2, [(32, 2), (32, 2)], gru_hidden=32)):
        model.conv_blocks[0]._engine()               # a block's own lazily built engine is not copied either
        twin = model.clone_without_engines()
        assert type(twin) is type(model) and twin.engine is not model.engine and type(twin.engine) is type(model.engine)
        assert twin.engine.head == model.engine.head and twin.engine._plans == {}
        assert twin.conv_blocks[0]._eng is None and model.conv_blocks[0]._eng is not None
        sa, sb = model.state_dict(), twin.state_dict()
        assert list(sa) == list(sb)
        for k in sa:
            assert torch.equal(sa[k], sb[k]) and sa[k].data_ptr() != sb[k].data_ptr(), k


# ---- CLI and the synthetic dataset -----------------------------------------------------------------------------------------------
def test_cli_flags_defaults_and_refusals(sed):
    main = importlib.import_module(PKG + ".main")
    a = main.build_full_parser().parse_args([])
    assert (a.mean_teacher, a.ema_decay, a.consistency_weight, a.consistency_rampup, a.eval_teacher, a.label_kinds) == \
        (False, 0.999, 2.0, 0, False, None)
    assert main.semi_options(a) == {} and main.semi_options(main.build_parser().parse_args([])) == {}
    assert vars(main.build_semi_parser().parse_args([])).keys() == {"mean_teacher", "ema_decay", "consistency_weight",
                                                                    "consistency_rampup", "eval_teacher", "label_kinds"}
    assert not hasattr(main.build_parser().parse_args([]), "mean_teacher")        # build_parser() keeps the reference's flags
    main.validate_args(a)
    spec = ["--train_features", "Spectogram", "--dataset_name", "synthetic"]
    a = main.build_full_parser().parse_args(spec + ["--mean_teacher", "--ema_decay", "0.99", "--consistency_weight", "1.5",
                                                    "--consistency_rampup", "50", "--eval_teacher", "--label_kinds", "1:2:5"])
    main.validate_args(a)
    assert main.semi_options(a) == {"mean_teacher": True, "ema_decay": 0.99, "consistency_weight": 1.5, "consistency_rampup": 50,
                                    "eval_teacher": True}
    assert main.parse_label_kinds(a.label_kinds) == (1.0, 2.0, 5.0)
    assert main.parse_label_kinds(None) is None and main.parse_label_kinds("0.5:0:0.5") == (0.5, 0.0, 0.5)
    for bad in ("1:2", "1:2:3:4", "a:b:c", "0:0:0", "1:-1:1", "", "1:inf:1"):
        with pytest.raises(ValueError, match="label_kinds"):
            main.parse_label_kinds(bad)
    for argv, word in ((["--train_features", "Waveform", "--mean_teacher"], "Spectogram"),
                       (["--train_features", "Waveform", "--dataset_name", "synthetic", "--label_kinds", "1:1:1"], "Spectogram"),
                       (["--train_features", "Spectogram", "--dataset_name", "TAU", "--label_kinds", "1:1:1"], "synthetic only"),
                       (spec + ["--eval_teacher"], "needs --mean_teacher"),
                       (spec + ["--mean_teacher", "--ema_decay", "1"], "ema_decay"),
                       (spec + ["--mean_teacher", "--consistency_weight", "-2"], "consistency_weight"),
                       (spec + ["--mean_teacher", "--consistency_rampup", "-2"], "consistency_rampup"),
                       (spec + ["--label_kinds", "1:1"], "label_kinds"),
                       (spec + ["--label_kinds", "1:1:1", "--spec_augment", "--mixup_prob", "0.5"], "mixup")):
        with pytest.raises(ValueError, match=word):
            main.validate_args(main.build_full_parser().parse_args(argv))
    main.validate_args(main.build_full_parser().parse_args(spec + ["--ema_decay", "7"]))           # off: unused
    main.validate_args(main.build_full_parser().parse_args(spec + ["--label_kinds", "1:1:1", "--spec_augment"]))       # no mixup: fine
    main.validate_args(main.build_full_parser().parse_args(spec + ["--mean_teacher", "--spec_augment", "--mixup_prob", "0.5"]))
    for argv in (["--ema_decay", "much"], ["--consistency_rampup", "1.5"]):
        with pytest.raises(SystemExit):
            main.build_full_parser().parse_args(argv)

    infer = importlib.import_module(PKG + ".infer")
    assert infer.build_parser().parse_args(["x.wav", "--ckpt", "c.pth"]).teacher is False
    assert infer.build_parser().parse_args(["x.wav", "--ckpt", "c.pth", "--teacher"]).teacher is True
    assert inspect.signature(infer.infer_file).parameters["teacher"].default is False


def test_synthetic_dataset_label_kinds(sed):
    synthetic = importlib.import_module(PKG + ".dataset.synthetic")
    kw = dict(n_train_crops=64, crop=40, n_val=1, val_frames=40, classes=2, seed=5)
    plain = synthetic.SyntheticSedDataset(**kw)
    ds = synthetic.SyntheticSedDataset(label_kinds=(1, 2, 5), **kw)
    again = synthetic.SyntheticSedDataset(label_kinds=(1, 2, 5), **kw)
    assert plain.kinds is None and len(plain[0]) == 2 and len(ds[0]) == 3
    assert np.array_equal(ds.kinds, again.kinds) and set(ds.kinds.tolist()) == {0, 1, 2}
    counts = np.bincount(ds.kinds, minlength=3)
    assert counts[2] > counts[1] > counts[0] > 0
    for i in range(len(ds)):
        f, y, kind = ds[i]
        f0, y0 = plain[i]
        assert int(kind) == ds.kinds[i] and kind.dtype == torch.int64 and torch.equal(f, f0) and y.shape == y0.shape
        if int(kind) == 0:
            assert torch.equal(y, y0)
        elif int(kind) == 1:                         # the clip label on every frame
            assert torch.equal(y, y0.max(dim=0, keepdim=True).values.expand_as(y0))
        else:
            assert not y.any()
    only_weak = synthetic.SyntheticSedDataset(label_kinds=(0, 1, 0), **kw)
    assert set(only_weak.kinds.tolist()) == {1}
    for bad in ((1, 2), (0, 0, 0), (1, -1, 1), (1, float("nan"), 1)):
        with pytest.raises(ValueError, match="label_kinds"):
            synthetic.SyntheticSedDataset(label_kinds=bad, **kw)
    # a DataLoader collates the kinds into a (B,) integer tensor
    from torch.utils.data import DataLoader
    f, y, kind = next(iter(DataLoader(ds, batch_size=8)))
    assert kind.shape == (8,) and kind.dtype == torch.int64 and f.shape == (8, 1, 40, 64) and y.shape == (8, 40, 2)
    val = list(ds.get_validation_sampler())
    assert len(val) == 1 and len(val[0]) == 3
