"""The PCEN front-end layer without a GPU: the float64 formula file against torch autograd, the C-ABI refusals, the layer's
state-dict round trip, the models' key lists with and without a layer, and the trainer's / command line's refusals as far as
they are raised before the GPU is touched."""
import argparse
import importlib
import os

import numpy as np
import pytest
import torch

import pcen_formula as PF
from conftest import ROOT

LIB = os.path.join(ROOT, "soundeventdetection-pytorch_amd", "libsed_hip.so")
TINY_CFG = [(4, 2), (8, 2), (8, 2), (8, 1)]


@pytest.fixture(scope="module")
def sed():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return importlib.import_module("soundeventdetection-pytorch_amd")


def torch_pcen(x, theta, kind, eps, gain, mean=None, std=None):
    """a plain torch restatement (float64, differentiable): the loop over t with tensors"""
    alpha, delta, r = torch.exp(theta[0]), torch.exp(theta[1]), torch.exp(theta[2])
    s = torch.sigmoid(theta[3])
    if kind == 0:
        v = x if mean is None else x * std + mean
        E = gain * torch.pow(torch.tensor(10.0, dtype=torch.float64), v / 10.0)
    else:
        E = gain * torch.relu(x)          # (subgradient 0 at x = 0, like the kernels; clamp would pass 1)
    Ms = [E[:, 0]]
    for t in range(1, x.shape[1]):
        Ms.append((1.0 - s) * Ms[-1] + s * E[:, t])
    M = torch.stack(Ms, dim=1)
    G = E * (eps + M) ** (-alpha)
    return (G + delta) ** r - delta ** r


def draw_case(kind, with_norm, seed, B=2, T=37, F=5):
    rng = np.random.default_rng(seed)
    theta = np.stack([np.log(0.98) + 0.1 * rng.standard_normal(F), np.log(2.0) + 0.2 * rng.standard_normal(F),
                      np.log(0.5) + 0.1 * rng.standard_normal(F), np.log(0.025 / 0.975) + 0.5 * rng.standard_normal(F)])
    mean = std = None
    if kind == 0:
        x = -30.0 + 10.0 * rng.standard_normal((B, T, F))
        if with_norm:
            mean, std = -30.0 + rng.standard_normal(F), 10.0 + rng.standard_normal(F)
            x = (x - mean) / std
    else:
        x = np.maximum(rng.standard_normal((B, T, F)), -0.2) * 1e-3       # negatives and, below, exact zeros
        x[rng.random((B, T, F)) < 0.1] = 0.0
    g = rng.standard_normal((B, T, F))
    return x, theta, mean, std, g


@pytest.mark.parametrize("kind,with_norm", [(0, False), (0, True), (1, False)])
def test_formula_matches_torch_autograd(kind, with_norm):
    """Every output of the formula file against autograd of the torch restatement, both in float64: per element the relative
    difference stays within 2^-40 A / |ref|, i.e. the difference within 2^-40 A."""
    eps, gain = 1e-6, 1.5
    x, theta, mean, std, g = draw_case(kind, with_norm, seed=3 + kind)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
    mt = None if mean is None else torch.tensor(mean, dtype=torch.float64)
    st = None if std is None else torch.tensor(std, dtype=torch.float64)
    yt = torch_pcen(xt, tt, kind, eps, gain, mt, st)
    yt.backward(torch.tensor(g, dtype=torch.float64))
    y, A_y = PF.forward(x, theta, kind, eps, gain, mean, std)
    bw = PF.backward(x, theta, kind, eps, gain, g, mean, std)
    for name, got, ref, A in (("y", y, yt.detach().numpy(), A_y), ("dx", bw["dx"], xt.grad.numpy(), bw["A_dx"]),
                              ("dtheta", bw["dtheta"], tt.grad.numpy(), bw["A_dtheta"])):
        err, lim = np.abs(got - ref), 2.0 ** -40 * A
        print(f"kind {kind} norm {with_norm} {name}: worst |diff| / (2^-40 A) = {float((err / np.where(lim > 0, lim, 1)).max()):.3e}")
        assert np.all(err <= lim), name
    if kind == 1:
        assert np.all(bw["dx"][x <= 0] == 0.0) and np.any(x == 0.0) and np.any(x < 0.0)


def test_formula_single_frame():
    """T = 1: M_0 = E_0, lambda_0 = m_0, no smoothing-coefficient gradient"""
    x, theta, _, _, g = draw_case(0, False, seed=9, T=1)
    bw = PF.backward(x, theta, 0, 1e-6, 1.0, g)
    assert np.all(bw["dtheta"][3] == 0.0) and np.all(np.isfinite(bw["dx"]))


def test_c_abi_refusals_without_gpu(sed):
    """Every refusal of sed_pcen_fwd / sed_pcen_bwd fires on the host before any launch (the pointers are never dereferenced)."""
    lib = sed._lib.lib()
    assert lib.sed_pcen_chunk() >= 2
    assert lib.sed_pcen_ws_bytes(2, 100, 64) > 0 and lib.sed_pcen_ws_bytes(2, 100, 257) == 0 and lib.sed_pcen_ws_bytes(0, 1, 1) == 0
    X, TH, Y, WS, GY, DX, DT, MEAN, STD = (1 << 20) * np.arange(1, 10)
    X, TH, Y, WS, GY, DX, DT, MEAN, STD = (int(v) for v in (X, TH, Y, WS, GY, DX, DT, MEAN, STD))
    B, T, F = 2, 40, 64

    def fwd(x=X, mean=None, std=None, theta=TH, kind=0, eps=1e-6, gain=1.0, y=Y, ws=WS, B=B, T=T, F=F):
        return lib.sed_pcen_fwd(x, mean, std, theta, kind, eps, gain, y, ws, B, T, F, None)

    def bwd(x=X, mean=None, std=None, theta=TH, kind=0, eps=1e-6, gain=1.0, gy=GY, dx=DX, dtheta=DT, ws=WS, B=B, T=T, F=F):
        return lib.sed_pcen_bwd(x, mean, std, theta, kind, eps, gain, gy, dx, dtheta, ws, B, T, F, None)

    nan = float("nan")
    cases = [dict(B=0), dict(T=0), dict(F=0), dict(B=-1), dict(F=257), dict(eps=0.0), dict(eps=-1.0), dict(eps=nan), dict(gain=0.0),
             dict(gain=nan), dict(kind=2), dict(kind=-1), dict(mean=MEAN), dict(std=STD), dict(kind=1, mean=MEAN, std=STD),
             dict(x=None), dict(theta=None), dict(ws=None)]
    for kw in cases:
        for name, fn in (("sed_pcen_fwd", fwd), ("sed_pcen_bwd", bwd)):
            rc = fn(**kw)
            assert rc != 0, (name, kw)
            assert name.encode() in lib.sed_last_error(), (name, kw, lib.sed_last_error())
    assert fwd(y=None) != 0 and b"null" in lib.sed_last_error()
    assert bwd(gy=None) != 0 and b"null" in lib.sed_last_error()
    assert bwd(dx=None, dtheta=None) != 0 and b"both NULL" in lib.sed_last_error()
    nbytes = B * T * F * 4
    for y in (X, X + 4, X + nbytes - 4, X - nbytes + 4):
        assert fwd(y=y) != 0 and b"overlap" in lib.sed_last_error()
        assert bwd(dx=y) != 0 and b"overlap" in lib.sed_last_error()
    with pytest.raises(RuntimeError, match="overlap"):
        sed._lib.check(fwd(y=X), "sed_pcen_fwd")


def test_layer_state_dict_round_trip(sed):
    F = 7
    mean, std = np.linspace(-40, -20, F), np.linspace(8, 12, F)
    a = sed.PCEN(F, input="db", mean=mean, std=std, alpha=0.9, delta=1.5, r=0.25, s=0.04, eps=1e-5, gain=2.0)
    assert [n for n, _ in a.named_parameters()] == ["log_alpha", "log_delta", "log_r", "logit_s"]
    with torch.no_grad():
        a.log_r += torch.linspace(-0.1, 0.1, F)
    sd = a.state_dict()
    assert list(sd) == ["log_alpha", "log_delta", "log_r", "logit_s", "feat_mean", "feat_std", "pcen_config"]
    assert sd["pcen_config"].dtype == torch.float64 and all(sd[k].shape == (F,) for k in list(sd)[:6])
    b = sed.PCEN.from_state_dict(sd)
    assert b.mel_bins == F and b._config == (0, 1e-5, 2.0) and b.trainable
    for k in sd:
        assert torch.equal(sd[k], b.state_dict()[k]), k
    # a prefix, the power input, a fixed layer: buffers of the same names, no parameter
    c = sed.PCEN(F, input="power", trainable=False)
    assert list(c.parameters()) == [] and [n for n, _ in c.named_buffers()][:4] == ["log_alpha", "log_delta", "log_r", "logit_s"]
    sdc = {"frontend." + k: v for k, v in c.state_dict().items()}
    sdc["event_fc.bias"] = torch.zeros(1)
    d = sed.PCEN.from_state_dict(sdc, prefix="frontend.", trainable=False)
    assert d._config == (1, 1e-6, 1.0) and d.feat_mean is None and list(d.state_dict()) == list(c.state_dict())
    assert np.allclose(torch.exp(c.log_alpha).numpy(), 0.98) and np.allclose(torch.sigmoid(c.logit_s).numpy(), 0.025)
    # load_state_dict carries the configuration over
    e = sed.PCEN(F, input="db", mean=np.zeros(F), std=np.ones(F))
    e.load_state_dict(sd)
    assert e._config == (0, 1e-5, 2.0)


def test_layer_constructor_refusals(sed):
    for kw in (dict(mel_bins=0), dict(mel_bins=257), dict(mel_bins=8, input="log"), dict(mel_bins=8, mean=np.zeros(8)),
               dict(mel_bins=8, input="power", mean=np.zeros(8), std=np.ones(8)), dict(mel_bins=8, s=1.0), dict(mel_bins=8, eps=0.0),
               dict(mel_bins=8, alpha=-1.0), dict(mel_bins=8, mean=np.zeros(7), std=np.ones(7))):
        with pytest.raises(ValueError):
            sed.PCEN(**kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sed.PCEN(8)(torch.zeros(1, 1, 4, 8))


@pytest.mark.parametrize("cls", ["Cnn_AvgPooling", "Crnn_AvgPooling"])
def test_model_keys_with_and_without_a_layer(sed, cls):
    make = getattr(sed, cls)
    torch.manual_seed(0)
    plain = make(1, TINY_CFG)
    torch.manual_seed(0)
    none = make(1, TINY_CFG, frontend=None)
    torch.manual_seed(0)
    with_fe = make(1, TINY_CFG, frontend=sed.PCEN(64))
    keys, pnames = list(plain.state_dict()), [n for n, _ in plain.named_parameters()]
    assert list(none.state_dict()) == keys and not any(k.startswith("frontend") for k in keys)
    fe_keys = ["frontend." + k for k in ("log_alpha", "log_delta", "log_r", "logit_s", "pcen_config")]
    assert list(with_fe.state_dict()) == fe_keys + keys
    assert [n for n, _ in with_fe.named_parameters()] == fe_keys[:4] + pnames
    assert [n for n, _ in with_fe._core_named_parameters()] == pnames
    for k in keys:                      # the layer draws nothing from the RNG: the same initial weights
        assert torch.equal(plain.state_dict()[k], with_fe.state_dict()[k]), k
    fixed = make(1, TINY_CFG, frontend=sed.PCEN(64, trainable=False))
    assert [n for n, _ in fixed.named_parameters()] == pnames and list(fixed.state_dict()) == fe_keys + keys
    twin = with_fe.clone_without_engines()
    assert twin.frontend is not with_fe.frontend and torch.equal(twin.frontend.log_alpha, with_fe.frontend.log_alpha)
    with pytest.raises(ValueError, match="mel bins"):
        make(1, TINY_CFG, frontend=sed.PCEN(40))
    make(1, TINY_CFG, mel_bins=40, frontend=sed.PCEN(40))
    with pytest.raises(TypeError):
        make(1, TINY_CFG, frontend=torch.nn.Identity())
    with pytest.raises(ValueError, match="front-end"):
        sed.M5(1, frontend=sed.PCEN(64))


def test_flat_params_put_the_layer_last(sed):
    """frontend.* is first in parameter order, so the last group in backward-completion order and the last bucket"""
    m = sed.Cnn_AvgPooling(1, TINY_CFG, frontend=sed.PCEN(64))
    flat = sed.train.FlatParams(m, n_buckets=0)
    assert flat.names[:4] == ["frontend.log_alpha", "frontend.log_delta", "frontend.log_r", "frontend.logit_s"]
    assert [k for k, _, _ in flat.groups] == ["event_fc", "conv_blocks.3", "conv_blocks.2", "conv_blocks.1", "conv_blocks.0", "frontend"]
    assert flat.buckets[-1][0] == ("frontend",) and flat.buckets[-1][1] == 0


def test_trainer_refusals_before_the_gpu(sed):
    T = sed.train
    m = sed.Cnn_AvgPooling(1, TINY_CFG, frontend=sed.PCEN(64))
    assert T.check_frontend_options(sed.Cnn_AvgPooling(1, TINY_CFG)) is None
    assert T.check_frontend_options(m) is m.frontend
    with pytest.raises(RuntimeError, match="graph"):
        T.check_frontend_options(m, graph=True)
    with pytest.raises(RuntimeError, match="mean_teacher"):
        T.check_frontend_options(m, mean_teacher=True)
    before = [p.data_ptr() for p in m.parameters()]
    for kw in (dict(graph=True), dict(mean_teacher=True)):
        with pytest.raises(RuntimeError, match="front-end"):
            sed.FusedTrainer(m, lr=1e-3, **kw)
    assert [p.data_ptr() for p in m.parameters()] == before
    with pytest.raises(RuntimeError, match="front-end"):
        T.train(m, [], sed.WeightedBCE(5, True), 1, 1e-3, 1, "unused", "cuda", mean_teacher=True)


def test_command_line(sed):
    main = importlib.import_module("soundeventdetection-pytorch_amd.main")
    parse = main.build_full_parser().parse_args
    base = ["--train_features", "Spectogram", "--dataset_name", "synthetic"]
    args = parse(base)
    assert main.pcen_options(args) is None and main.build_pcen(args, 64) is None
    main.validate_args(args)
    args = parse(base + ["--pcen", "--pcen_alpha", "0.8", "--pcen_delta", "1", "--pcen_r", "0.25", "--pcen_s", "0.1", "--pcen_eps", "1e-5",
                         "--pcen_gain", "3"])
    main.validate_args(args)
    layer = main.build_pcen(args, 40, mean=-30.0, std=np.full(40, 9.0))
    assert layer.trainable and layer.mel_bins == 40 and layer._config == (0, 1e-5, 3.0)
    assert np.allclose(layer.feat_mean.numpy(), -30.0) and np.allclose(layer.feat_std.numpy(), 9.0)
    assert np.allclose(torch.exp(layer.log_alpha.detach()).numpy(), 0.8) and np.allclose(torch.sigmoid(layer.logit_s.detach()).numpy(), 0.1)
    fixed = main.build_pcen(parse(base + ["--pcen_fixed"]), 64)
    assert fixed is not None and not fixed.trainable and fixed.feat_mean is None
    for extra, match in ((["--pcen", "--mean_teacher"], "mean_teacher"), (["--pcen", "--pcen_s", "1.5"], "pcen_s"),
                         (["--pcen", "--pcen_eps", "0"], "pcen_eps"), (["--pcen_fixed", "--pcen_alpha", "-1"], "pcen_alpha")):
        with pytest.raises(ValueError, match=match):
            main.validate_args(parse(base + extra))
    with pytest.raises(ValueError, match="Spectogram"):
        main.validate_args(parse(["--train_features", "Waveform", "--dataset_name", "synthetic", "--pcen"]))
    assert main.pcen_options(argparse.Namespace()) is None
