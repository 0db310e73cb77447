"""Host side of the weak-label (clip-level) loss (no GPU): the tests' formula (tests/weak_formula.py) against torch autograd in
float64, its two forms against each other, every argument refusal of sed_clip_pool_fwd / sed_weak_bce_fwd_bwd through the built
library, the Python-level refusals and the CLI flags.  Every C-ABI refusal case passes NULL for a required pointer or a bad value,
so a validation bug would end in the null-pointer refusal and never in a launch."""
import ctypes as C
import importlib
import inspect
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from weak_formula import MODES, frame_counts, weak_loop, weak_vectorised

PKG = "soundeventdetection-pytorch_amd"
LIB = os.path.join(ROOT, PKG, "libsed_hip.so")


@pytest.fixture(scope="module")
def sed():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return importlib.import_module(PKG)


# ---- the formula -----------------------------------------------------------------------------------------------------------------
def autograd_reference(pre, target, ratio, Tt, mode, w, weight, grad_scale):
    """sigmoid -> repeat_interleave(ratio) -> [:N] -> pooling -> weighted BCE, composed by hand in float64"""
    x = torch.tensor(pre, dtype=torch.float64, requires_grad=True)
    B, t, K = x.shape
    N = min(t * ratio, Tt)
    p = torch.sigmoid(x).repeat_interleave(ratio, dim=1)[:, :N]
    if mode == "max":
        P = p.max(dim=1).values
    elif mode == "mean":
        P = p.mean(dim=1)
    elif mode == "linear":
        P = (p * p).sum(dim=1) / p.sum(dim=1)
    else:
        P = (p * torch.exp(p)).sum(dim=1) / torch.exp(p).sum(dim=1)
    y = torch.tensor(target, dtype=torch.float64)
    Y = y if y.dim() == 2 else y[:, :N].max(dim=1).values
    loss = weight * (-(w * Y * torch.log(P) + (1.0 - Y) * torch.log(1.0 - P))).mean()
    (loss * grad_scale).backward()
    return P.detach().numpy(), Y.numpy(), float(loss.detach()), x.grad.numpy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ratio,t,Tt", [(1, 7, 7), (1, 7, 5), (8, 5, 40), (8, 5, 37), (8, 5, 45), (8, 5, 3), (8, 1, 8)])
@pytest.mark.parametrize("strong", [False, True])
def test_formula_equals_autograd(mode, ratio, t, Tt, strong):
    rng = np.random.default_rng(1000 * ratio + 10 * t + Tt + MODES.index(mode))
    B, K = 2, 3
    pre = rng.uniform(-6.0, 6.0, (B, t, K))            # unsaturated, and distinct: the max has one winner
    if strong:
        target = (rng.random((B, Tt, K)) > 0.7).astype(np.float64) * rng.uniform(0.5, 1.0, (B, Tt, K))      # soft labels too
    else:
        target = np.where(rng.random((B, K)) > 0.5, rng.uniform(0.5, 1.0, (B, K)), 0.0)
    w, weight, gs = 5.0, 0.75, 0.5
    P, Y, loss, dpre = weak_loop(pre, target, ratio, Tt, mode, w, weight, gs)
    Pa, Ya, la, da = autograd_reference(pre, target, ratio, Tt, mode, w, weight, gs)
    np.testing.assert_allclose(P, Pa, rtol=1e-12, atol=0)
    assert np.array_equal(Y, Ya)
    np.testing.assert_allclose(loss, la, rtol=1e-12)
    np.testing.assert_allclose(dpre, da, rtol=1e-9, atol=1e-13 * np.abs(da).max())
    N, c = frame_counts(t, ratio, Tt)
    assert np.array_equal(dpre[:, c == 0], np.zeros_like(dpre[:, c == 0]))


@pytest.mark.parametrize("mode", MODES)
def test_formula_loops_equal_vectorised(mode):
    rng = np.random.default_rng(7)
    for (B, t, K), ratio, Tt in (((2, 5, 3), 8, 37), ((1, 1, 1), 1, 1), ((3, 9, 2), 8, 5), ((2, 12, 4), 1, 17), ((2, 6, 2), 4, 24)):
        pre = rng.normal(0.0, 4.0, (B, t, K))
        pre[0, 0, 0] = 60.0
        pre[-1, -1, -1] = -60.0
        if t > 2:
            pre[0, 1, 0] = pre[0, 2, 0] = pre[0].max() + 1.0          # a tie
        for target in (rng.random((B, K)), (rng.random((B, Tt, K)) > 0.6).astype(np.float64)):
            a = weak_loop(pre, target, ratio, Tt, mode, 5.0, 2.0, 0.25)
            b = weak_vectorised(pre, target, ratio, Tt, mode, 5.0, 2.0, 0.25)
            np.testing.assert_allclose(a[0], b[0], rtol=1e-14)
            assert np.array_equal(a[1], b[1])
            np.testing.assert_allclose(a[2], b[2], rtol=1e-13)
            np.testing.assert_allclose(a[3], b[3], rtol=1e-12, atol=1e-15 * np.abs(a[3]).max())
            assert np.array_equal(a[3] == 0.0, b[3] == 0.0)
    # a row of logits so low that every probability is 0: P = 0, Q = 1, loss = w * Y * 100, no gradient, nothing non-finite
    pre = np.full((1, 4, 2), -1000.0)
    for fn in (weak_loop, weak_vectorised):
        P, Y, loss, dpre = fn(pre, np.array([[1.0, 0.0]]), 8, 32, mode, 5.0)
        assert np.array_equal(P, np.zeros((1, 2))) and loss == 250.0 and np.array_equal(dpre, np.zeros_like(pre))


def test_formula_max_tie_takes_the_smaller_index():
    pre = np.array([[[0.5], [2.0], [2.0], [1.0]]])
    for fn in (weak_loop, weak_vectorised):
        dpre = fn(pre, np.array([[1.0]]), 2, 8, "max", 5.0)[3]
        assert dpre[0, 1, 0] != 0.0 and np.array_equal(dpre[0, [0, 2, 3], 0], np.zeros(3))


# ---- the C ABI refuses bad arguments before any launch ---------------------------------------------------------------------------
def test_argument_validation_without_gpu(sed):
    L = sed._lib
    lib = L.lib()
    assert (L.POOL_MAX, L.POOL_MEAN, L.POOL_LINEAR, L.POOL_EXP) == (0, 1, 2, 3)
    assert L.POOL_MODES == {"max": 0, "mean": 1, "linear": 2, "exp": 3}
    B, t, K, ratio, Tt = 2, 5, 3, 8, 37
    assert lib.sed_weak_bce_ws_bytes(B, t, K) >= B * K * 8
    assert lib.sed_weak_bce_ws_bytes(0, t, K) == 0
    # host memory standing in for the device buffers: never touched, every call below is refused first
    pre, dpre = (C.c_float * (B * t * K))(), (C.c_float * (B * t * K))()
    target, clip, loss = (C.c_float * (B * Tt * K))(), (C.c_float * (B * K))(), (C.c_float * 1)()
    ws = (C.c_double * (B * K + 1))()
    A = C.addressof

    def refused(rc, word):
        assert rc != 0 and word in lib.sed_last_error(), (rc, word, lib.sed_last_error())

    def pool(pre_p=A(pre), clip_p=None, B_=B, t_=t, K_=K, ratio_=ratio, Tt_=Tt, mode=2):
        return lib.sed_clip_pool_fwd(pre_p, clip_p, B_, t_, K_, ratio_, Tt_, mode, None)

    refused(pool(), b"null")                        # everything valid but clip_prob
    refused(pool(pre_p=None, clip_p=A(clip)), b"null")
    for kw in ({"B_": 0}, {"t_": 0}, {"K_": -1}, {"ratio_": 0}, {"Tt_": 0}):
        refused(pool(**kw), b"bad sizes")
    for mode in (-1, 4, 17):
        refused(pool(mode=mode), b"mode")
    refused(pool(B_=1 << 16, K_=1 << 15), b"too many")
    refused(pool(t_=1 << 20, ratio_=1 << 11), b"t * ratio")

    def weak(pre_p=A(pre), target_p=A(target), frames=Tt, clip_p=A(clip), loss_p=None, dpre_p=A(dpre), acc=0, B_=B, t_=t, K_=K,
             ratio_=ratio, Tt_=Tt, mode=2, ws_p=A(ws)):
        return lib.sed_weak_bce_fwd_bwd(pre_p, target_p, frames, clip_p, loss_p, dpre_p, acc, B_, t_, K_, ratio_, Tt_, mode, 5.0, 1.0,
                                        1.0, ws_p, None)

    refused(weak(), b"null")                        # everything valid but loss
    refused(weak(frames=0), b"null")
    refused(weak(clip_p=None, dpre_p=None), b"null")            # the optional pointers may be NULL: still stops at loss
    refused(weak(pre_p=None, loss_p=A(loss)), b"null")
    refused(weak(target_p=None, loss_p=A(loss)), b"null")
    refused(weak(ws_p=None, loss_p=A(loss)), b"null")
    refused(weak(ws_p=A(ws) + 4, loss_p=A(loss), pre_p=None), b"null")
    refused(weak(ws_p=A(ws) + 4, loss_p=A(loss)), b"aligned")
    for kw in ({"B_": 0}, {"t_": -2}, {"K_": 0}, {"ratio_": 0}, {"Tt_": 0, "frames": 0}):
        refused(weak(**kw), b"bad sizes")
    for mode in (-1, 4):
        refused(weak(mode=mode), b"mode")
    for frames in (-1, 1, Tt - 1, Tt + 1):
        refused(weak(frames=frames), b"target_frames")
    for acc in (-1, 2):
        refused(weak(acc=acc), b"accumulate")
    refused(weak(B_=1 << 16, K_=1 << 15), b"too many")


# ---- Python-level refusals -------------------------------------------------------------------------------------------------------
def test_python_refusals(sed):
    train = importlib.import_module(PKG + ".train")
    common = importlib.import_module(PKG + ".utils.common")
    engine = importlib.import_module(PKG + ".engine")
    assert train.check_weak_options() is None
    assert train.check_weak_options("linear", 2, True) == ("linear", 2.0, True)
    assert train.check_weak_options("max") == ("max", 1.0, False)
    for bad in ("softmax", "Linear", "", 2):
        with pytest.raises(ValueError, match="unknown pooling"):
            train.check_weak_options(bad)
        with pytest.raises(ValueError, match="unknown pooling"):
            common.WeakBCE(5, bad)
        with pytest.raises(ValueError, match="unknown pooling"):
            engine.check_pooling(bad)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="weak_weight"):
            train.check_weak_options("mean", bad)
    with pytest.raises(ValueError, match="weak_only needs"):
        train.check_weak_options(None, 1.0, True)
    with pytest.raises(ValueError, match="ratio"):
        common.WeakBCE(5, "mean", ratio=0)

    # the M5 model has no time axis in its output: refused on the host, by the trainer and by train(), before any device work
    m5 = sed.M5(1)
    cnn = sed.Cnn_AvgPooling(1, [(32, 2), (32, 2)])
    with pytest.raises(ValueError, match="no time axis"):
        train.check_weak_options("linear", 1.0, True, m5)
    with pytest.raises(ValueError, match="no time axis"):
        train.FusedTrainer(m5, 1e-3, weak_pooling="linear", weak_only=True)
    with pytest.raises(ValueError, match="no time axis"):
        train.train(m5, None, sed.WeightedBCE(5, False), 1, 1e-3, 1, "unused", "cuda", weak_pooling="max", weak_only=True)
    with pytest.raises(ValueError, match="no time axis"):
        train.train(m5, None, sed.WeakBCE(5, "max"), 1, 1e-3, 1, "unused", "cuda")
    assert train.check_weak_options("linear", 1.0, True, cnn) == ("linear", 1.0, True)
    with pytest.raises(ValueError, match="unknown pooling"):
        train.FusedTrainer(cnn, 1e-3, weak_pooling="attention")
    with pytest.raises(ValueError, match="weak_weight"):
        train.train(cnn, None, sed.WeightedBCE(5, True), 1, 1e-3, 1, "unused", "cuda", weak_pooling="exp", weak_weight=0.0)
    with pytest.raises(ValueError, match="criterion pools with"):
        train.train(cnn, None, sed.WeakBCE(5, "max"), 1, 1e-3, 1, "unused", "cuda", weak_pooling="exp")

    # wrong target rank / shapes, refused before the tensors are looked at any further
    crit = sed.WeakBCE(5, "linear", ratio=4)
    out = torch.zeros(2, 8, 3)
    for target in (torch.zeros(2), torch.zeros(2, 8, 3, 1)):
        with pytest.raises(ValueError, match="expected"):
            crit(out, target)
    with pytest.raises(ValueError, match="expected"):
        crit(torch.zeros(2, 8), torch.zeros(2, 3))
    for target in (torch.zeros(3, 3), torch.zeros(2, 4), torch.zeros(2, 8, 2)):
        with pytest.raises(ValueError, match="batch or classes"):
            crit(out, target)
    with pytest.raises(ValueError, match="multiple of ratio"):
        crit(torch.zeros(2, 9, 3), torch.zeros(2, 3))

    for fn, names in ((train.FusedTrainer.__init__, ("weak_pooling", "weak_weight", "weak_only")),
                      (train.train, ("weak_pooling", "weak_weight", "weak_only"))):
        prm = inspect.signature(fn).parameters
        assert [prm[n].default for n in names] == [None, 1.0, False]
    assert all(inspect.signature(train.train).parameters[n].kind is inspect.Parameter.KEYWORD_ONLY
               for n in ("weak_pooling", "weak_weight", "weak_only"))
    assert inspect.signature(engine.CnnEngine.loss_and_grad).parameters["weak"].default is None


# ---- CLI -------------------------------------------------------------------------------------------------------------------------
def test_cli_flags_defaults_and_refusals(sed):
    main = importlib.import_module(PKG + ".main")
    a = main.build_full_parser().parse_args([])
    assert (a.weak_labels, a.weak_pooling, a.weak_weight) == ("off", "linear", 1.0)
    assert main.weak_options(a) == {}
    assert not hasattr(main.build_parser().parse_args([]), "weak_labels")         # build_parser() keeps the reference's flags
    assert vars(a).items() >= vars(main.build_parser().parse_args([])).items()
    main.validate_args(a)
    bare = main.build_parser().parse_args([])
    main.validate_args(bare)
    assert main.weak_options(bare) == {}
    a = main.build_full_parser().parse_args(["--train_features", "Spectogram", "--dataset_name", "synthetic", "--weak_labels", "only"])
    main.validate_args(a)
    assert main.weak_options(a) == {"weak_pooling": "linear", "weak_weight": 1.0, "weak_only": True}
    a = main.build_full_parser().parse_args(["--train_features", "Spectogram", "--weak_labels", "both", "--weak_pooling", "exp",
                                             "--weak_weight", "0.5"])
    main.validate_args(a)
    assert main.weak_options(a) == {"weak_pooling": "exp", "weak_weight": 0.5, "weak_only": False}
    for argv in (["--weak_labels", "some"], ["--weak_pooling", "attention"], ["--weak_weight", "much"]):
        with pytest.raises(SystemExit):
            main.build_full_parser().parse_args(argv)
    for w in ("0", "-1", "nan", "inf"):
        with pytest.raises(ValueError, match="weak_weight"):
            main.validate_args(main.build_full_parser().parse_args(["--train_features", "Spectogram", "--weak_labels", "both",
                                                                    "--weak_weight", w]))
    main.validate_args(main.build_full_parser().parse_args(["--train_features", "Spectogram", "--weak_weight", "-1"]))     # off: unused
    with pytest.raises(ValueError, match="Spectogram"):
        main.validate_args(main.build_full_parser().parse_args(["--train_features", "Waveform", "--weak_labels", "only"]))
    a.weak_labels = "sometimes"
    with pytest.raises(ValueError, match="weak_labels"):
        main.validate_args(a)

    infer = importlib.import_module(PKG + ".infer")
    b = infer.build_parser().parse_args(["x.wav", "--ckpt", "c.pth"])
    assert b.clip_pooling is None
    b = infer.build_parser().parse_args(["x.wav", "--ckpt", "c.pth", "--clip_pooling", "linear"])
    assert b.clip_pooling == "linear"
    with pytest.raises(SystemExit):
        infer.build_parser().parse_args(["x.wav", "--ckpt", "c.pth", "--clip_pooling", "median"])
    assert inspect.signature(infer.infer_file).parameters["clip_pooling"].default is None
    with pytest.raises(ValueError, match="unknown pooling"):
        infer.infer_file("missing.wav", "missing.pth", clip_pooling="median")
