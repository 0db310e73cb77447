"""Host side of the attention pooling head (no GPU): the tests' formula (tests/att_formula.py) against torch autograd in float64,
its two forms against each other, the properties of the definition, mutants of the reference that the gate has to reject, every
argument refusal of the sed_att_* entry points through the built library, the Python-level refusals, the CLI flags and the
state_dict.  Every C-ABI refusal case passes NULL for a required pointer or a bad value, so a validation bug would end in the
null-pointer refusal and never in a launch."""
import ctypes as C
import importlib
import inspect
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from att_formula import CRITERIA, att_loop, att_vectorised, feature_grad, gate, linear_bwd, linear_fwd
from weak_formula import frame_counts, weak_vectorised

PKG = "soundeventdetection-pytorch_amd"
LIB = os.path.join(ROOT, PKG, "libsed_hip.so")
W = 5.0


@pytest.fixture(scope="module")
def sed():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return importlib.import_module(PKG)


# ---- the formula -----------------------------------------------------------------------------------------------------------------
def autograd_reference(pre, att, target, ratio, Tt, w, weight, grad_scale, criterion, sel, class_softmax=False):
    """repeat_interleave both logit tensors, cut to N frames, softmax over time, weighted sum, the criterion: float64 autograd"""
    x = torch.tensor(pre, dtype=torch.float64, requires_grad=True)
    a = torch.tensor(att, dtype=torch.float64, requires_grad=True)
    B, t, K = x.shape
    N = min(t * ratio, Tt)
    p = torch.sigmoid(x).repeat_interleave(ratio, dim=1)[:, :N]
    wgt = torch.softmax(a.repeat_interleave(ratio, dim=1)[:, :N], dim=2 if class_softmax else 1)
    if class_softmax:
        wgt = wgt / wgt.sum(dim=1, keepdim=True)
    P = (wgt * p).sum(dim=1)
    y = torch.tensor(target, dtype=torch.float64)
    Y = y if y.dim() == 2 else y[:, :N].max(dim=1).values
    l = -(w * Y * torch.log(P) + (1.0 - Y) * torch.log(1.0 - P)) if criterion == "bce" else (P - Y) ** 2
    on = torch.ones(B, dtype=torch.bool) if sel is None else torch.tensor(np.asarray(sel) != 0)
    S = int(on.sum())
    loss = weight * l[on].sum() / (S * K) if S else 0.0 * l.sum()
    (loss * grad_scale).backward()
    return P.detach().numpy(), Y.numpy(), float(loss.detach()), x.grad.numpy(), a.grad.numpy()


def inputs(rng, B, t, K, Tt, strong):
    pre = rng.uniform(-6.0, 6.0, (B, t, K))
    att = rng.normal(0.0, 2.0, (B, t, K))
    if strong:
        target = (rng.random((B, Tt, K)) > 0.7).astype(np.float64) * rng.uniform(0.5, 1.0, (B, Tt, K))
    else:
        target = np.where(rng.random((B, K)) > 0.5, rng.uniform(0.5, 1.0, (B, K)), 0.0)
    return pre, att, target


@pytest.mark.parametrize("criterion", CRITERIA)
@pytest.mark.parametrize("ratio,t,Tt", [(1, 7, 7), (1, 7, 5), (8, 5, 40), (8, 5, 37), (8, 5, 45), (8, 5, 11), (8, 1, 8)])
@pytest.mark.parametrize("strong", [False, True])
@pytest.mark.parametrize("sel", [None, (1, 0, 1), (0, 0, 0)])
def test_formula_equals_autograd(criterion, ratio, t, Tt, strong, sel):
    rng = np.random.default_rng(1000 * ratio + 10 * t + Tt)
    B, K = 3, 2
    pre, att, target = inputs(rng, B, t, K, Tt, strong)
    w, weight, gs = W, 0.75, 0.5
    r = att_loop(pre, att, target, ratio, Tt, w, weight, gs, criterion, sel)
    Pa, Ya, la, dx, da = autograd_reference(pre, att, target, ratio, Tt, w, weight, gs, criterion, sel)
    np.testing.assert_allclose(r["P"], Pa, rtol=1e-12, atol=0)
    assert np.array_equal(r["Y"], Ya)
    np.testing.assert_allclose(r["loss"], la, rtol=1e-12, atol=0)
    np.testing.assert_allclose(r["dpre"], dx, rtol=1e-9, atol=1e-13 * r["A_dpre"].max())
    np.testing.assert_allclose(r["datt"], da, rtol=1e-9, atol=1e-13 * r["A_datt"].max())      # (p - P cancels: relative to p + P)
    _, c = frame_counts(t, ratio, Tt)
    for g in (r["dpre"], r["datt"]):
        assert np.array_equal(g[:, c == 0], np.zeros_like(g[:, c == 0]))
        if sel is not None:
            off = np.asarray(sel) == 0
            assert np.array_equal(g[off], np.zeros_like(g[off]))
    if sel == (0, 0, 0):
        assert r["loss"] == 0.0 and not r["dpre"].any() and not r["datt"].any()


@pytest.mark.parametrize("criterion", CRITERIA)
def test_formula_loops_equal_vectorised(criterion):
    rng = np.random.default_rng(7)
    for (B, t, K), ratio, Tt in (((2, 5, 3), 8, 37), ((1, 1, 1), 1, 1), ((3, 9, 2), 8, 21), ((2, 12, 4), 1, 17), ((2, 6, 2), 4, 24)):
        pre = rng.normal(0.0, 4.0, (B, t, K))
        att = rng.normal(0.0, 30.0, (B, t, K))
        pre[0, 0, 0], pre[-1, -1, -1] = 60.0, -60.0
        for target in (rng.random((B, K)), (rng.random((B, Tt, K)) > 0.6).astype(np.float64)):
            for sel in (None, [1] + [0] * (B - 1)):
                a = att_loop(pre, att, target, ratio, Tt, W, 2.0, 0.25, criterion, sel)
                b = att_vectorised(pre, att, target, ratio, Tt, W, 2.0, 0.25, criterion, sel)
                assert np.array_equal(a["Y"], b["Y"])
                for n in ("P", "loss", "dpre", "datt", "A_P", "A_loss", "A_dpre", "A_datt"):
                    np.testing.assert_allclose(a[n], b[n], rtol=1e-12, atol=1e-15 * max(np.abs(a[n]).max(), 1e-300), err_msg=n)
                for n in ("dpre", "datt"):
                    assert np.array_equal(a[n] == 0.0, b[n] == 0.0)
                    ok, _ = gate(a[n], b[n], b["A_" + n])
                    assert ok


def test_datt_sums_to_zero_over_time():
    rng = np.random.default_rng(3)
    for ratio, t, Tt in ((1, 40, 40), (8, 40, 317), (8, 1025, 8200)):
        pre, att = rng.normal(0.0, 3.0, (2, t, 3)), rng.normal(0.0, 5.0, (2, t, 3))
        target = (rng.random((2, 3)) > 0.5).astype(np.float64)
        for criterion in CRITERIA:
            d = att_vectorised(pre, att, target, ratio, Tt, W, 1.0, 1.0, criterion)["datt"]
            assert (np.abs(d.sum(axis=1)) <= 2.0 ** -40 * np.abs(d).sum(axis=1)).all()


def test_constant_attention_is_mean_pooling():
    rng = np.random.default_rng(4)
    for ratio, t, Tt in ((1, 9, 9), (8, 9, 67), (8, 9, 20)):
        pre = rng.normal(0.0, 3.0, (2, t, 3))
        target = (rng.random((2, Tt, 3)) > 0.8).astype(np.float64)
        for const in (0.0, -17.25, 900.0):
            r = att_vectorised(pre, np.full_like(pre, const), target, ratio, Tt, W, 0.5, 2.0)
            P, Y, loss, dpre = weak_vectorised(pre, target, ratio, Tt, "mean", W, 0.5, 2.0)
            np.testing.assert_allclose(r["P"], P, rtol=1e-14)
            np.testing.assert_allclose(r["loss"], loss, rtol=1e-13)
            np.testing.assert_allclose(r["dpre"], dpre, rtol=1e-12, atol=0)
            assert np.array_equal(r["Y"], Y)


def test_underflowing_weights_leave_a_finite_result():
    pre = np.array([[[2.0], [-1.0], [0.5], [3.0]]])
    att = np.array([[[0.0], [-900.0], [850.0], [-3.0]]])          # a spread above 800: all weights but one are exactly 0 in double
    for fn in (att_loop, att_vectorised):
        r = fn(pre, att, np.array([[1.0]]), 8, 30, W)
        assert r["P"][0, 0] == 1.0 / (1.0 + np.exp(-0.5)) and np.isfinite(r["loss"])
        assert np.array_equal(r["dpre"][0, [0, 1, 3], 0], np.zeros(3)) and r["dpre"][0, 2, 0] != 0.0
        assert np.array_equal(r["datt"], np.zeros((1, 4, 1)))
    # a row with c_i = 0 does not enter the maximum, however large its attention logit
    att2 = att.copy()
    att2[0, 3, 0] = 5000.0
    a, b = att_vectorised(pre, att, np.array([[1.0]]), 8, 24, W), att_vectorised(pre, att2, np.array([[1.0]]), 8, 24, W)
    assert np.array_equal(a["P"], b["P"]) and np.array_equal(a["dpre"], b["dpre"])


# ---- the gate rejects wrong formulas ---------------------------------------------------------------------------------------------
def mutant(name, pre, att, target, ratio, Tt, criterion, sel):
    """(dpre, datt, P, loss) of a wrong attention pooling: the definition written out once more, with one deliberate mistake"""
    if name == "softmax over classes":
        P, _, loss, dx, da = autograd_reference(pre, att, target, ratio, Tt, W, 0.75, 0.5, criterion, sel, class_softmax=True)
        return dx, da, P, loss
    B, t, K = pre.shape
    N, c = frame_counts(t, ratio, Tt)
    live = (c > 0).astype(np.float64)[None, :, None]
    cc = live * ratio if name == "c_i ignored" else c.astype(np.float64)[None, :, None]
    amax = att.max(axis=1, keepdims=True) if name == "a_max over all rows" else np.where(live > 0, att, -np.inf).max(axis=1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ce = cc * np.exp(np.minimum(att - amax, 0.0))
        p, q = 1.0 / (1.0 + np.exp(-pre)), 1.0 / (1.0 + np.exp(pre))
        Z = ce.sum(axis=1, keepdims=True)
        P, Q = (ce * p).sum(axis=1, keepdims=True) / Z, (ce * q).sum(axis=1, keepdims=True) / Z
        Y = (target if target.ndim == 2 else target[:, :N].max(axis=1))[:, None, :]
        if criterion == "bce":
            l = -(W * Y * np.maximum(np.log(P), -100.0) + (1.0 - Y) * np.maximum(np.log(Q), -100.0))
            dl = -W * Y / np.maximum(P, 1e-12) + (1.0 - Y) / np.maximum(Q, 1e-12)
        else:
            l, dl = (P - Y) ** 2, 2.0 * (P - Y)
        on = np.asarray(sel) != 0
        S = B if name == "selection ignored in the divisor" else int(on.sum())
        m = on[:, None, None].astype(np.float64)
        coef = 0.75 * 0.5 / (S * K)
        dpre = m * coef * dl * (ce / Z) * (p * q)
        datt = m * coef * dl * ce * (p if name == "- P dropped from datt" else p - P) / Z
    return dpre, datt, P[:, 0], 0.75 * float((m * l).sum()) / (S * K)


@pytest.mark.parametrize("criterion", CRITERIA)
@pytest.mark.parametrize("name", ["softmax over classes", "c_i ignored", "- P dropped from datt", "a_max over all rows",
                                  "selection ignored in the divisor"])
def test_gate_rejects_mutants(name, criterion):
    rng = np.random.default_rng(11)
    B, t, K, ratio, Tt = 3, 6, 3, 8, 35          # a partial row (c = 3) and a row with c_i = 0
    pre, att, target = inputs(rng, B, t, K, Tt, strong=False)
    target[:, 0] = 1.0
    att[:, 5] = 1000.0                           # a row that takes no part: it must not enter the maximum
    sel = (1, 0, 1)
    ref = att_vectorised(pre, att, target, ratio, Tt, W, 0.75, 0.5, criterion, sel)
    # the reference itself, through the other form, passes
    loop = att_loop(pre, att, target, ratio, Tt, W, 0.75, 0.5, criterion, sel)
    for n in ("dpre", "datt", "P", "loss"):
        assert gate(loop[n], ref[n], ref["A_" + n])[0], n
    dx, da, P, loss = mutant(name, pre, att, target, ratio, Tt, criterion, sel)
    verdicts = [gate(dx, ref["dpre"], ref["A_dpre"])[0], gate(da, ref["datt"], ref["A_datt"])[0], gate(P, ref["P"], ref["A_P"])[0],
                gate(loss, ref["loss"], ref["A_loss"])[0]]
    assert not all(verdicts), (name, verdicts)
    if name == "- P dropped from datt":
        assert verdicts == [True, False, True, True]
    if name == "selection ignored in the divisor":
        assert verdicts == [False, False, True, False]


def test_linear_layer_and_backward_formulas_against_autograd():
    rng = np.random.default_rng(5)
    rows, C, Cp, K, Wf = 7, 5, 8, 3, 2
    m = rng.normal(size=(rows, Cp))
    w, b, fw = rng.normal(size=(K, C)), rng.normal(size=K), rng.normal(size=(K, C))
    dpre, datt = rng.normal(size=(rows, K)), rng.normal(size=(rows, K))
    mt = torch.tensor(m[:, :C], requires_grad=True)
    wt, bt, fwt = (torch.tensor(v, requires_grad=True) for v in (w, b, fw))
    att = mt @ wt.T + bt
    pre = mt @ fwt.T
    ((att * torch.tensor(datt)).sum() + (pre * torch.tensor(dpre)).sum()).backward()
    got, scale = linear_fwd(m, w, b)
    np.testing.assert_allclose(got, att.detach().numpy(), rtol=1e-13)
    assert (scale >= np.abs(got) - 1e-12).all()
    dw, db, sw, sb = linear_bwd(datt, m, C)
    np.testing.assert_allclose(dw, wt.grad.numpy(), rtol=1e-12)
    np.testing.assert_allclose(db, bt.grad.numpy(), rtol=1e-12)
    assert (sw >= np.abs(dw) - 1e-12).all() and (sb >= np.abs(db) - 1e-12).all()
    df, sf = feature_grad(dpre, datt, fw, w, 1)
    np.testing.assert_allclose(df, mt.grad.numpy(), rtol=1e-12)
    np.testing.assert_allclose(feature_grad(dpre, datt, fw, w, Wf)[0], df / Wf, rtol=1e-15)
    assert (sf >= np.abs(df) - 1e-12).all()


# ---- the C ABI refuses bad arguments before any launch ---------------------------------------------------------------------------
def test_argument_validation_without_gpu(sed):
    L = sed._lib
    lib = L.lib()
    assert L.POOL_MODES == {"max": 0, "mean": 1, "linear": 2, "exp": 3}           # the attention pooling is not one of them
    B, t, K, ratio, Tt, Cc = 2, 5, 3, 8, 37, 8
    assert lib.sed_att_loss_ws_bytes(B, t, K) >= B * K * 32 and lib.sed_att_loss_ws_bytes(B, t, K) % 8 == 0
    assert lib.sed_att_loss_ws_bytes(0, t, K) == 0 and lib.sed_att_loss_ws_bytes(B, t, 0) == 0
    # host memory standing in for the device buffers: never touched, every call below is refused first
    n = B * t * K
    pre, att, dpre, datt = ((C.c_float * n)() for _ in range(4))
    target, clip, loss = (C.c_float * (B * Tt * K))(), (C.c_float * (B * K))(), (C.c_float * 1)()
    sel = (C.c_ubyte * B)()
    ws = (C.c_double * (B * K * 40 + 1))()
    A = C.addressof

    def refused(rc, word):
        assert rc != 0 and word in lib.sed_last_error(), (rc, word, lib.sed_last_error())

    def pool(pre_p=A(pre), att_p=A(att), clip_p=None, B_=B, t_=t, K_=K, ratio_=ratio, Tt_=Tt):
        return lib.sed_att_pool_fwd(pre_p, att_p, clip_p, B_, t_, K_, ratio_, Tt_, None)

    refused(pool(), b"null")                        # everything valid but clip_prob
    refused(pool(pre_p=None, clip_p=A(clip)), b"null")
    refused(pool(att_p=None, clip_p=A(clip)), b"null")
    for kw in ({"B_": 0}, {"t_": 0}, {"K_": -1}, {"ratio_": 0}, {"Tt_": 0}):
        refused(pool(**kw), b"bad sizes")
    refused(pool(B_=1 << 16, K_=1 << 15), b"too many")
    refused(pool(t_=1 << 20, ratio_=1 << 11), b"t * ratio")

    def lossf(pre_p=A(pre), att_p=A(att), target_p=A(target), frames=Tt, sel_p=A(sel), crit=0, clip_p=A(clip), loss_p=None,
              dpre_p=A(dpre), datt_p=A(datt), acc=0, B_=B, t_=t, K_=K, ratio_=ratio, Tt_=Tt, ws_p=A(ws)):
        return lib.sed_att_loss_fwd_bwd(pre_p, att_p, target_p, frames, sel_p, crit, clip_p, loss_p, dpre_p, datt_p, acc, B_, t_, K_,
                                        ratio_, Tt_, 5.0, 1.0, 1.0, ws_p, None)

    refused(lossf(), b"null")                       # everything valid but loss
    refused(lossf(frames=0), b"null")
    refused(lossf(clip_p=None, dpre_p=None, datt_p=None, sel_p=None, crit=1), b"null")       # the optional ones may be NULL
    for name in ("pre_p", "att_p", "target_p", "ws_p"):
        refused(lossf(loss_p=A(loss), **{name: None}), b"null")
    refused(lossf(loss_p=A(loss), dpre_p=None, pre_p=None), b"null")
    refused(lossf(loss_p=None, dpre_p=None), b"null")
    refused(lossf(loss_p=None, datt_p=None), b"null")
    refused(lossf(ws_p=A(ws) + 4, pre_p=None, loss_p=A(loss)), b"null")
    refused(lossf(ws_p=A(ws) + 4), b"null")
    for kw in ({"B_": 0}, {"t_": -2}, {"K_": 0}, {"ratio_": 0}, {"Tt_": 0, "frames": 0}):
        refused(lossf(**kw), b"bad sizes")
    for crit in (-1, 2, 7):
        refused(lossf(crit=crit), b"criterion")
    for frames in (-1, 1, Tt - 1, Tt + 1):
        refused(lossf(frames=frames), b"target_frames")
    for acc in (-1, 2):
        refused(lossf(acc=acc), b"accumulate")
    refused(lossf(B_=1 << 16, K_=1 << 15), b"too many")
    # with loss given and nothing else wrong, the checks that come after the null check are reached: each with one more fault
    # that keeps the call from launching
    refused(lossf(loss_p=A(loss), ws_p=A(ws) + 4), b"aligned")
    refused(lossf(loss_p=A(loss), dpre_p=None), b"together")
    refused(lossf(loss_p=A(loss), datt_p=None), b"together")

    m, w, b = (C.c_float * (4 * Cc))(), (C.c_float * (K * Cc))(), (C.c_float * K)()
    out = (C.c_float * (4 * K))()

    def logits(m_p=A(m), w_p=A(w), b_p=A(b), out_p=None, rows=4, C_=Cc, Cp=Cc, K_=K):
        return lib.sed_att_logits_fwd(m_p, w_p, b_p, out_p, rows, C_, Cp, K_, None)

    refused(logits(), b"null")
    for name in ("m_p", "w_p", "b_p"):
        refused(logits(out_p=A(out), **{name: None}), b"null")
    for kw in ({"rows": 0}, {"C_": 0}, {"K_": 0}, {"C_": 9}, {"rows": -3}):
        refused(logits(**kw), b"bad sizes")
    refused(logits(C_=4096, Cp=4096), b"2048")
    refused(logits(rows=1 << 27, K_=1 << 10), b"too many")

    d2, w2 = (C.c_float * (4 * 2 * K))(), (C.c_float * (2 * K * Cc))()

    def pack(dpre_p=A(dpre), datt_p=A(datt), fw_p=A(w), aw_p=A(w), d_p=A(d2), w_p=None, rows=4, C_=Cc, K_=K):
        return lib.sed_att_bwd_pack(dpre_p, datt_p, fw_p, aw_p, d_p, w_p, rows, C_, K_, None)

    refused(pack(), b"null")
    for name in ("dpre_p", "datt_p", "fw_p", "aw_p", "d_p"):
        refused(pack(w_p=A(w2), **{name: None}), b"null")
    for kw in ({"rows": 0}, {"C_": 0}, {"K_": -1}):
        refused(pack(**kw), b"bad sizes")

    def split(dw_p=A(w2), db_p=A(d2), a=A(w), b_=A(b), c=A(w), d=None, C_=Cc, K_=K):
        return lib.sed_att_bwd_split(dw_p, db_p, a, b_, c, d, C_, K_, None)

    refused(split(), b"null")
    for name in ("dw_p", "db_p", "a", "b_", "c"):
        refused(split(d=A(b), **{name: None}), b"null")
    for kw in ({"C_": 0}, {"K_": 0}):
        refused(split(**kw), b"bad sizes")


# ---- Python-level refusals, defaults and the state_dict --------------------------------------------------------------------------
CFG = [(32, 2), (32, 2)]


def test_state_dict_and_parameter_order(sed):
    for cls, kw in ((sed.Cnn_AvgPooling, {}), (sed.Crnn_AvgPooling, {"gru_hidden": 32})):
        torch.manual_seed(0)
        plain = cls(3, CFG, **kw)
        after_plain = torch.rand(1)
        torch.manual_seed(0)
        off = cls(3, CFG, attention=False, **kw)
        after_off = torch.rand(1)
        torch.manual_seed(0)
        head = cls(3, CFG, attention=True, **kw)
        assert inspect.signature(cls.__init__).parameters["attention"].default is False
        assert list(off.state_dict()) == list(plain.state_dict()) and torch.equal(after_plain, after_off)     # no random number drawn
        assert not hasattr(off, "att_fc") and off.engine.attention is False and head.engine.attention is True
        keys = list(head.state_dict())
        assert keys[:-2] == list(plain.state_dict()) and keys[-2:] == ["att_fc.weight", "att_fc.bias"]
        for k, v in plain.state_dict().items():            # the same seed: every other parameter is the same
            assert torch.equal(v, head.state_dict()[k]), k
        feat = 64 if cls is sed.Crnn_AvgPooling else 32
        assert head.att_fc.weight.shape == (3, feat) and head.att_fc.bias.shape == (3,)
        assert bool((head.att_fc.bias == 0).all()) and float(head.att_fc.weight.detach().abs().max()) > 0       # init_layer
        assert not torch.equal(head.att_fc.weight, head.event_fc.weight)
        twin = head.clone_without_engines()
        assert twin.attention and twin.engine.attention and twin.engine is not head.engine
        assert torch.equal(twin.att_fc.weight, head.att_fc.weight) and twin.att_fc.weight is not head.att_fc.weight
        plain.load_state_dict(off.state_dict())
        with pytest.raises(RuntimeError, match="att_fc"):
            plain.load_state_dict(head.state_dict())


def test_flat_params_put_the_attention_group_first(sed):
    train = importlib.import_module(PKG + ".train")
    head = sed.Cnn_AvgPooling(3, CFG, attention=True)
    flat = train.FlatParams(head, n_buckets=0)
    assert [k for k, _, _ in flat.groups] == ["att_fc", "event_fc", "conv_blocks.1", "conv_blocks.0"]
    (k, s, e) = flat.groups[0]
    assert s == flat.offsets["att_fc.weight"] and e == flat.numel and flat.offsets["att_fc.bias"] == s + 3 * 32
    plain = train.FlatParams(sed.Cnn_AvgPooling(3, CFG), n_buckets=0)
    assert [k for k, _, _ in plain.groups] == ["event_fc", "conv_blocks.1", "conv_blocks.0"]
    for n, o in plain.offsets.items():
        assert flat.offsets[n] == o


def test_python_refusals(sed):
    train = importlib.import_module(PKG + ".train")
    common = importlib.import_module(PKG + ".utils.common")
    engine = importlib.import_module(PKG + ".engine")
    plain, head, m5 = sed.Cnn_AvgPooling(3, CFG), sed.Cnn_AvgPooling(3, CFG, attention=True), sed.M5(1)
    # the names the parameter-free poolings keep
    assert "att" not in sed._lib.POOL_MODES and "attention" not in sed._lib.POOL_MODES
    for bad in ("att", "attention"):
        with pytest.raises(ValueError, match="unknown pooling"):
            engine.check_pooling(bad)
        with pytest.raises(ValueError, match="unknown pooling"):
            common.WeakBCE(5, bad)
    with pytest.raises(ValueError, match="frame logits"):
        common.WeakBCE(5, "att")
    for fn in (train.check_weak_options, train.check_ranking_options):
        with pytest.raises(ValueError, match="unknown pooling"):
            fn("attention", model=head)
    # the new check takes the model
    assert engine.check_clip_pooling("att", head) == "att" and engine.check_clip_pooling("linear", plain) == "linear"
    assert engine.check_clip_pooling("att", head.engine) == "att"
    with pytest.raises(ValueError, match="attention head"):
        engine.check_clip_pooling("att", plain)
    with pytest.raises(ValueError, match="unknown pooling"):
        engine.check_clip_pooling("median", head)
    assert train.check_weak_options("att", 2, True, head) == ("att", 2.0, True)
    assert train.check_ranking_options("att", head) == "att"
    with pytest.raises(ValueError, match="attention head"):
        train.check_weak_options("att", 1.0, True, plain)
    with pytest.raises(ValueError, match="attention head"):
        train.check_ranking_options("att", plain)
    with pytest.raises(ValueError, match="attention head"):
        train.check_weak_options("att", 1.0, True, m5)
    with pytest.raises(ValueError, match="weak_weight"):
        train.check_weak_options("att", 0.0, True, head)
    with pytest.raises(ValueError, match="attention head"):
        train.FusedTrainer(plain, 1e-3, weak_pooling="att")
    with pytest.raises(ValueError, match="attention head"):
        train.train(plain, None, sed.WeightedBCE(5, True), 1, 1e-3, 1, "unused", "cuda", weak_pooling="att", weak_only=True)
    # an engine without a head takes no attention layer
    with pytest.raises(ValueError, match="classification head"):
        engine.CnnEngine(3, CFG, head="none", attention=True)
    assert inspect.signature(engine.CnnEngine.__init__).parameters["attention"].default is False
    assert inspect.signature(engine.CnnEngine.loss_and_grad).parameters["teacher_att"].default is None
    assert engine.CnnEngine(3, CFG).attention is False


def test_cli_flags_defaults_and_refusals(sed):
    main = importlib.import_module(PKG + ".main")
    a = main.build_full_parser().parse_args([])
    assert a.attention_head is False and a.weak_pooling == "linear" and a.eval_clip_pooling is None
    assert not hasattr(main.build_parser().parse_args([]), "attention_head")
    main.validate_args(a)
    base = ["--train_features", "Spectogram", "--dataset_name", "synthetic"]
    a = main.build_full_parser().parse_args(base + ["--attention_head", "--weak_labels", "only", "--weak_pooling", "att"])
    main.validate_args(a)
    assert a.attention_head and main.weak_options(a) == {"weak_pooling": "att", "weak_weight": 1.0, "weak_only": True}
    main.validate_args(main.build_full_parser().parse_args(base + ["--attention_head"]))             # the head alone: fine
    main.validate_args(main.build_full_parser().parse_args(base + ["--attention_head", "--eval_ranking", "--eval_clip_pooling", "att"]))
    main.validate_args(main.build_full_parser().parse_args(base + ["--weak_pooling", "att"]))          # --weak_labels off: unused
    with pytest.raises(ValueError, match="--attention_head"):
        main.validate_args(main.build_full_parser().parse_args(base + ["--weak_labels", "both", "--weak_pooling", "att"]))
    with pytest.raises(ValueError, match="--attention_head"):
        main.validate_args(main.build_full_parser().parse_args(base + ["--eval_ranking", "--eval_clip_pooling", "att"]))
    with pytest.raises(ValueError, match="Spectogram"):
        main.validate_args(main.build_full_parser().parse_args(["--train_features", "Waveform", "--attention_head"]))
    for argv in (["--weak_pooling", "attention"], ["--eval_clip_pooling", "attention"]):
        with pytest.raises(SystemExit):
            main.build_full_parser().parse_args(argv)

    infer = importlib.import_module(PKG + ".infer")
    b = infer.build_parser().parse_args(["x.wav", "--ckpt", "c.pth", "--clip_pooling", "att"])
    assert b.clip_pooling == "att"
    with pytest.raises(SystemExit):
        infer.build_parser().parse_args(["x.wav", "--ckpt", "c.pth", "--clip_pooling", "attention"])
    with pytest.raises(ValueError, match="unknown pooling"):
        infer.infer_file("missing.wav", "missing.pth", clip_pooling="attention")
