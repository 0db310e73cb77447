"""Host (no GPU): the local attention window's definition and gates (tests/window_formula.py) against torch in float64, the tile count
formula of sed_mhsa_win_tiles against the brute-force count, and Csa_AvgPooling(sa_window=)'s keys, draws, refusals and flags.

Mutants.  Inputs N(0, 1.5) for q and k (scores of standard deviation about 2, so that a key more or less moves a row's softmax by far
more than a rounding), t = 70 (three query tiles, so that the tile-start mutant differs), window (5, 2).  Margin seen: the worst output
of every mutant is at least 1.5e5 gates out (no_renorm and lse_all, on lse; the others further), and the test asks for 100 (-s prints
every mutant's figure per output)."""
import importlib

import numpy as np
import pytest
import torch

import ffn_formula as FF
import dropout_formula as DF
import mhsa_formula as MF
import window_formula as WF

PKG = "soundeventdetection-pytorch_amd"
CFG = [(32, 2), (64, 2), (128, 2), (128, 1)]
WINDOWS = [(3, 3), (5, 2), (4, 0), (0, 0), (None, 0), (2, None), (None, None), (100, 100)]
NAMES = ("ctx", "lse", "dq", "dk", "dv")


@pytest.fixture(scope="module")
def sed():
    return importlib.import_module(PKG)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1.0))       # (absolute below 1: a window of (0, 0) has dq = dk = 0 exactly)


def attn_case(B=2, t=37, H=2, dh=32, seed=0, sigma=1.0):
    rng = np.random.default_rng(seed)
    return tuple(rng.normal(0.0, s, (B, t, H, dh)) for s in (sigma, sigma, 1.0, 1.0))


# ---- the definition against torch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", WINDOWS, ids=str)
def test_core_against_multihead_attention_with_attn_mask(window):
    """identity projections: torch.nn.MultiheadAttention's core alone, float64, autograd"""
    q, k, v, d = attn_case()
    B, t, H, dh = q.shape
    C = H * dh
    mha = torch.nn.MultiheadAttention(C, H, batch_first=True, bias=False).double()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(C).repeat(3, 1))
        mha.out_proj.weight.copy_(torch.eye(C))
    tq, tk, tv = (torch.from_numpy(a.reshape(B, t, C)).requires_grad_(True) for a in (q, k, v))
    mask = torch.from_numpy(WF.torch_mask(t, *window))
    out, _ = mha(tq, tk, tv, attn_mask=mask, need_weights=False)
    out.backward(torch.from_numpy(d.reshape(B, t, C)))
    r = WF.core(q, k, v, *window, d)
    assert rel(r["ctx"].reshape(B, t, C), out.detach().numpy()) < 1e-12
    for n, g in (("dq", tq.grad), ("dk", tk.grad), ("dv", tv.grad)):
        assert rel(r[n].reshape(B, t, C), g.numpy()) < 1e-12, n
    # lse is the log-sum over the in-window keys
    s = np.einsum("bihc,bjhc->bhij", q, k) / np.sqrt(dh)
    w = WF.in_window(t, *window)
    assert rel(r["lse"], np.log(np.where(w, np.exp(s), 0.0).sum(axis=3))) < 1e-12
    assert not r["p"][..., ~w].any() and np.allclose(r["p"].sum(axis=3), 1.0, atol=1e-14)


def test_an_unbounded_window_is_the_plain_core():
    q, k, v, d = attn_case()
    t = q.shape[1]
    ref = MF.core(q, k, v, d)
    for window in ((None, None), (t - 1, t - 1), (1000, None)):
        r = WF.core(q, k, v, *window, d)
        for n in NAMES:
            assert np.array_equal(r[n], ref[n]), (window, n)
    keep, s = DF.keep_attn([1, 2, 3, 0], 0, 2, 2, t, 0.5), DF.thr_scale(0.5)[1]
    refd, rd = DF.core(q, k, v, keep, s, d), WF.core(q, k, v, None, None, d, keep=keep, s=s)
    for n in NAMES:
        assert np.array_equal(rd[n], refd[n]), n


def encoder_weights(rng, C, D, layers):
    W = {}
    for l in range(layers):
        an, nn_, fn, fnn = FF.layer_names(l)
        W.update({an + ".in_proj_weight": rng.normal(0, 0.2, (3 * C, C)), an + ".in_proj_bias": rng.normal(0, 0.1, 3 * C),
                  an + ".out_proj.weight": rng.normal(0, 0.2, (C, C)), an + ".out_proj.bias": rng.normal(0, 0.1, C),
                  nn_ + ".weight": rng.normal(1, 0.2, C), nn_ + ".bias": rng.normal(0, 0.1, C),
                  fn + ".linear1.weight": rng.normal(0, 0.2, (D, C)), fn + ".linear1.bias": rng.normal(0, 0.1, D),
                  fn + ".linear2.weight": rng.normal(0, 0.2, (C, D)), fn + ".linear2.bias": rng.normal(0, 0.1, C),
                  fnn + ".weight": rng.normal(1, 0.2, C), fnn + ".bias": rng.normal(0, 0.1, C)})
    return W


@pytest.mark.parametrize("window", [(3, 3), (5, 2), (4, 0), (None, None)], ids=str)
def test_encoder_against_transformer_encoder_layer_with_src_mask(window):
    rng = np.random.default_rng(5)
    B, t, C, H, D, layers = 2, 12, 64, 2, 96, 2
    W = encoder_weights(rng, C, D, layers)
    x, dh = rng.normal(0, 1, (B * t, C)), rng.normal(0, 1, (B * t, C))
    got = WF.encoder(x, W, B, t, H, *window, layers=layers, ffn_width=D, act="gelu", pos_encoding=False, dh_out=dh)
    mask = torch.from_numpy(WF.torch_mask(t, *window))
    h = torch.from_numpy(x.reshape(B, t, C)).requires_grad_(True)
    cur, mods = h, []
    for l in range(layers):
        an, nn_, fn, fnn = FF.layer_names(l)
        e = torch.nn.TransformerEncoderLayer(C, H, D, dropout=0.0, activation="gelu", batch_first=True, norm_first=False).double()
        names = {"self_attn": an, "norm1": nn_, "linear1": fn + ".linear1", "linear2": fn + ".linear2", "norm2": fnn}
        e.load_state_dict({n: torch.from_numpy(W[names[n.split(".", 1)[0]] + "." + n.split(".", 1)[1]]) for n in e.state_dict()})
        cur = e(cur, src_mask=mask)
        mods.append((e, names))
    cur.backward(torch.from_numpy(dh.reshape(B, t, C)))
    assert rel(got["h"], cur.detach().numpy().reshape(B * t, C)) < 1e-12
    assert rel(got["dx"], h.grad.numpy().reshape(B * t, C)) < 1e-12
    for e, names in mods:
        for n, p in e.named_parameters():
            top, rest = n.split(".", 1)
            assert rel(got["d_" + names[top] + "." + rest], p.grad.numpy()) < 1e-11, n
    if window == (None, None):
        ref = FF.encoder(x, W, B, t, H, layers=layers, ffn_width=D, act="gelu", pos_encoding=False, dh_out=dh)
        for n in ref:
            assert rel(got[n], ref[n]) < 1e-12, n


# ---- the gates: a plain fp32 implementation passes, mutants fail --------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("window", [(3, 0), (5, 2), (40, 7), (0, 0), (None, 0)], ids=str)
def test_plain_fp32_passes_every_gate(window, p, mode):
    bf = mode == "bf16"
    rb = MF.round_bf16 if bf else (lambda a: np.asarray(a, dtype=np.float32))
    q, k, v, d = (rb(a) for a in attn_case(t=70, sigma=1.5))
    B, t, H, dh = q.shape
    keep, s = (DF.keep_attn([1, 2, 3, 0], 0, B, H, t, p), DF.thr_scale(p)[1]) if p else (None, 1.0)
    ref = WF.core(q, k, v, *window, d, keep=keep, s=s)
    g = WF.core_gates(q, k, v, *window, d, keep=keep, s=s, mode=mode)
    got = WF.core(q, k, v, *window, d, keep=keep, s=s, dtype=np.float32, bf16_operands=bf)
    for n in NAMES:
        assert WF.check(got[n], ref[n], g[n], (window, mode, p, n))[0], n


def test_mutants_fail_the_fp32_gates():
    q, k, v, d = (a.astype(np.float32) for a in attn_case(t=70, sigma=1.5))
    window = (5, 2)
    ref, g = WF.core(q, k, v, *window, d), WF.core_gates(q, k, v, *window, d)
    closest = None
    for mutant in ("swapped", "left_off_by_one", "right_off_by_one", "no_renorm", "tile_start", "bwd_unmasked", "lse_all"):
        with np.errstate(over="ignore", invalid="ignore"):
            got = WF.core(q, k, v, *window, d, dtype=np.float32, mutant=mutant)
        out = {}
        for n in NAMES:
            err = np.abs(got[n].astype(np.float64) - ref[n])
            out[n] = float(np.nanmax(np.where(np.isfinite(err), err / g[n], np.inf)))
        worst = max(out.values())
        print(f"{mutant}: worst error / gate by output {out}")
        assert worst > 100.0, f"the mutant {mutant} is not 100 gates out anywhere"
        closest = worst if closest is None else min(closest, worst)
        if mutant == "bwd_unmasked":
            assert out["ctx"] <= 1.0 and out["lse"] <= 1.0 and min(out["dq"], out["dk"], out["dv"]) > 100.0
        if mutant == "lse_all":
            assert out["ctx"] <= 1.0 and out["lse"] > 100.0
    print(f"the closest mutant is {closest:.3g} gates out")


# ---- the tile count -------------------------------------------------------------------------------------------------------------------
def win_tiles(t, left, right, which):
    """sed_mhsa_win_tiles' formula: a wave that owns rows [a0, a0 + 31] walks the tiles that meet [a0 - before, a0 + 31 + after]"""
    if t <= 0 or left < 0 or right < 0 or which not in (0, 1, 2):
        return -1
    left, right = min(left, t - 1), min(right, t - 1)
    before, after = (right, left) if which == 1 else (left, right)
    n = 0
    for a0 in range(0, t, 32):
        lo = max(a0 - before, 0) // 32 * 32
        hi = min(a0 + 31 + after, t - 1) + 1
        n += -(-(hi - lo) // 32)
    return n


@pytest.mark.parametrize("t", [1, 33, 130, 257])
def test_tile_count_formula_is_the_brute_force_count(t):
    sides_ = [0, 1, 3, 31, 32, 33, 40, 63, 64, 65, 127, 128, 129, t - 2, t - 1, t, 10 ** 6, 0x7FFFFFFF]
    for left in sides_:
        for right in sides_:
            if left < 0 or right < 0:
                continue
            for which in (0, 1, 2):
                assert win_tiles(t, left, right, which) == WF.tiles_brute(t, left, right, which), (t, left, right, which)
    full = (-(-t // 32)) ** 2
    assert win_tiles(t, t, t, 0) == full and win_tiles(t, 0, 0, 1) == -(-t // 32)
    assert win_tiles(0, 1, 1, 0) == win_tiles(5, -1, 0, 0) == win_tiles(5, 0, 0, 3) == -1


def test_the_library_counts_tiles_without_a_gpu(sed):
    lib = sed._lib.lib()
    for t in (1, 33, 130, 257, 750):
        for left, right in ((0, 0), (3, 0), (32, 32), (64, 0), (40, 7), (0x7FFFFFFF, 0), (t - 2, t - 2), (0x7FFFFFFF, 0x7FFFFFFF)):
            if min(left, right) < 0:
                continue
            for which in (0, 1, 2):
                assert lib.sed_mhsa_win_tiles(t, left, right, which) == win_tiles(t, left, right, which), (t, left, right, which)
    assert lib.sed_mhsa_win_tiles(0, 0, 0, 0) == -1 and lib.sed_mhsa_win_tiles(5, 0, 0, 3) == -1 and lib.sed_mhsa_win_tiles(5, -1, 0, 0) == -1


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def test_model_refusals_keys_and_draws(sed):
    for bad in (-1, (3, -1), (-2, 0), 1.5, (1.0, 2), "3", (1, 2, 3), (1,), True, (None, True)):
        rng_state = torch.random.get_rng_state()
        with pytest.raises(ValueError, match="sa_window"):
            sed.Csa_AvgPooling(3, CFG, sa_heads=2, sa_window=bad)
        assert torch.equal(rng_state, torch.random.get_rng_state()), "a refused model drew random numbers"
    with pytest.raises(ValueError, match="sa_window"):
        sed.CnnEngine(3, CFG, head="sa", sa_heads=2, sa_window=-1)
    with pytest.raises(ValueError, match="sa_window"):
        sed.CnnEngine(3, CFG, head="fc", sa_window=3)
    for cls in (sed.Cnn_AvgPooling, sed.Crnn_AvgPooling):
        with pytest.raises(TypeError):
            cls(3, CFG, sa_window=3)
    torch.manual_seed(11)
    plain = sed.Csa_AvgPooling(3, CFG, precision="fp32", sa_heads=2, sa_layers=2, sa_ffn=96, sa_conv_kernel=7)
    after_plain = torch.random.get_rng_state()
    torch.manual_seed(11)
    none = sed.Csa_AvgPooling(3, CFG, precision="fp32", sa_heads=2, sa_layers=2, sa_ffn=96, sa_conv_kernel=7, sa_window=None)
    torch.manual_seed(11)
    win = sed.Csa_AvgPooling(3, CFG, precision="fp32", sa_heads=2, sa_layers=2, sa_ffn=96, sa_conv_kernel=7, sa_window=(64, None))
    assert torch.equal(after_plain, torch.random.get_rng_state()), "sa_window must not draw a random number"
    # without a window: the old keys and values, no buffer, no window in the engine
    assert list(none.state_dict()) == list(plain.state_dict()) and "window_config" not in none.state_dict()
    assert none.engine.sa_window is None and sed.Csa_AvgPooling.window_config_from_state_dict(none.state_dict()) is None
    # with one: the same draws, one more buffer
    keys = list(win.state_dict())
    assert [k for k in keys if k != "window_config"] == list(plain.state_dict())
    for n, v in plain.state_dict().items():
        assert torch.equal(v, win.state_dict()[n]), n
    cfg = win.state_dict()["window_config"]
    assert cfg.dtype == torch.float64 and cfg.tolist() == [64.0, -1.0]
    assert sed.Csa_AvgPooling.window_config_from_state_dict(win.state_dict()) == (64, None) == win.engine.sa_window
    # round trips: every form of the option, through the buffer and into a rebuilt model; a clone keeps it
    for given, pair in ((5, (5, 5)), ((3, 0), (3, 0)), ([0, 7], (0, 7)), ((None, 0), (None, 0)), ((None, None), (None, None)), (0, (0, 0))):
        m = sed.Csa_AvgPooling(3, CFG, sa_heads=2, sa_window=given)
        back = sed.Csa_AvgPooling.window_config_from_state_dict(m.state_dict())
        assert back == pair == m.sa_window == m.engine.sa_window
        again = sed.Csa_AvgPooling(3, CFG, sa_heads=2, sa_window=back)
        again.load_state_dict(m.state_dict())
        assert m.clone_without_engines().engine.sa_window == pair
    # a checkpoint with a window does not load into a model without one (and the other way round): the architecture differs
    with pytest.raises(RuntimeError):
        plain.load_state_dict(win.state_dict())


def test_command_line_flags(sed):
    main = importlib.import_module(PKG + ".main")
    full = main.build_full_parser()
    base = ["--train_features", "Spectogram", "--dataset_name", "synthetic"]
    for text, pair in (("32", (32, 32)), ("64:0", (64, 0)), ("inf:0", (None, 0)), ("0:inf", (0, None)), ("inf", (None, None)), ("8:3", (8, 3))):
        args = full.parse_args(base + ["--self_attention", "--sa_window", text])
        main.validate_args(args)
        assert main.parse_sa_window(args.sa_window) == pair
    assert full.parse_args(base).sa_window is None and main.parse_sa_window(None) is None
    main.validate_args(full.parse_args(base))
    for bad in ("-1", "3:-2", "1:2:3", "x", "1.5", ""):
        with pytest.raises(ValueError, match="sa_window"):
            main.validate_args(full.parse_args(base + ["--self_attention", "--sa_window=" + bad]))
    with pytest.raises(ValueError, match="--self_attention"):
        main.validate_args(full.parse_args(base + ["--sa_window", "32"]))
