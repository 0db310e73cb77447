"""Host (no GPU): the learned relative-position bias' definition and gates (tests/relpos_formula.py) against torch in float64, the bucket
maps' properties, and Csa_AvgPooling(sa_rel_pos=)'s keys, draws, refusals and flags.

Mutants.  Inputs N(0, 1.5) for q and k (scores of standard deviation about 2), table entries N(0, 1), t = 70 (three query tiles), window
(40, 7), L = 3.  The fp32 gate must reject each mutant by a wide margin: the test asks for 100 gates on its worst output (-s prints every
mutant's figure per output)."""
import importlib

import numpy as np
import pytest
import torch

import ffn_formula as FF
import dropout_formula as DF
import mhsa_formula as MF
import relpos_formula as RF
import window_formula as WF

PKG = "soundeventdetection-pytorch_amd"
CFG = [(32, 2), (64, 2), (128, 2), (128, 1)]
WINDOWS = [(None, None), (3, 0), (5, 2), (40, 7)]
BUCKETS = [1, 3, 40, (8, 16), (32, 128), (4, 2)]
NAMES = ("ctx", "lse", "dq", "dk", "dv", "drel", "dw")


@pytest.fixture(scope="module")
def sed():
    return importlib.import_module(PKG)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1.0))


def attn_case(B=2, t=37, H=2, dh=32, seed=0, sigma=1.0):
    rng = np.random.default_rng(seed)
    return tuple(rng.normal(0.0, s, (B, t, H, dh)) for s in (sigma, sigma, 1.0, 1.0))


def float_mask(w, cfg, t, window):
    """torch's additive float attn_mask (H, t, t) built THROUGH a gather of the weights, so autograd reaches w"""
    idx = torch.from_numpy(RF.bucket_map(cfg, t).astype(np.int64)[RF.dist_index(t)])
    bias = w[:, idx]
    return bias.masked_fill(torch.from_numpy(WF.torch_mask(t, *window))[None], float("-inf"))


# ---- the definition against torch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [3, 40, (8, 16), (32, 128)], ids=str)
@pytest.mark.parametrize("window", WINDOWS, ids=str)
def test_core_against_multihead_attention_with_a_float_attn_mask(window, cfg):
    q, k, v, d = attn_case()
    B, t, H, dh = q.shape
    C = H * dh
    rng = np.random.default_rng(3)
    wt = rng.normal(0.0, 1.0, (H, RF.num_buckets(cfg)))
    mha = torch.nn.MultiheadAttention(C, H, batch_first=True, bias=False).double()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(C).repeat(3, 1))
        mha.out_proj.weight.copy_(torch.eye(C))
    tq, tk, tv = (torch.from_numpy(a.reshape(B, t, C)).requires_grad_(True) for a in (q, k, v))
    tw = torch.from_numpy(wt).requires_grad_(True)
    mask = float_mask(tw, cfg, t, window).repeat(B, 1, 1)          # (B H, t, t), clip-major like torch's heads
    out, _ = mha(tq, tk, tv, attn_mask=mask, need_weights=False)
    out.backward(torch.from_numpy(d.reshape(B, t, C)))
    r = RF.core(q, k, v, RF.expand(wt, cfg, t), *window, d, cfg=cfg)
    assert rel(r["ctx"].reshape(B, t, C), out.detach().numpy()) < 1e-12
    for n, g in (("dq", tq.grad), ("dk", tk.grad), ("dv", tv.grad)):
        assert rel(r[n].reshape(B, t, C), g.numpy()) < 1e-12, n
    assert rel(r["dw"], tw.grad.numpy()) < 1e-12
    # drel folds to dw, and a bucket no distance of the clip maps to has gradient 0
    used = np.zeros(RF.num_buckets(cfg), dtype=bool)
    used[RF.bucket_map(cfg, t)] = True
    assert not r["dw"][:, ~used].any() and not tw.grad.numpy()[:, ~used].any()


def test_a_zero_table_is_the_windowed_core_bit_for_bit():
    q, k, v, d = attn_case()
    B, t, H, dh = q.shape
    keep, s = DF.keep_attn([1, 2, 3, 0], 0, B, H, t, 0.5), DF.thr_scale(0.5)[1]
    for window in WINDOWS:
        for kw in (dict(), dict(keep=keep, s=s)):
            ref = WF.core(q, k, v, *window, d, **kw)
            r = RF.core(q, k, v, np.zeros((H, 2 * t - 1)), *window, d, **kw)
            for n in ("ctx", "lse", "dq", "dk", "dv"):
                assert np.array_equal(r[n], ref[n]), (window, n)


def encoder_weights(rng, C, D, layers, H, cfg):
    W = {}
    for l in range(layers):
        an, nn_, fn, fnn = FF.layer_names(l)
        W.update({an + ".in_proj_weight": rng.normal(0, 0.2, (3 * C, C)), an + ".in_proj_bias": rng.normal(0, 0.1, 3 * C),
                  an + ".out_proj.weight": rng.normal(0, 0.2, (C, C)), an + ".out_proj.bias": rng.normal(0, 0.1, C),
                  nn_ + ".weight": rng.normal(1, 0.2, C), nn_ + ".bias": rng.normal(0, 0.1, C),
                  fn + ".linear1.weight": rng.normal(0, 0.2, (D, C)), fn + ".linear1.bias": rng.normal(0, 0.1, D),
                  fn + ".linear2.weight": rng.normal(0, 0.2, (C, D)), fn + ".linear2.bias": rng.normal(0, 0.1, C),
                  fnn + ".weight": rng.normal(1, 0.2, C), fnn + ".bias": rng.normal(0, 0.1, C),
                  RF.rel_name(l) + ".weight": rng.normal(0, 1.0, (H, RF.num_buckets(cfg)))})
    return W


@pytest.mark.parametrize("cfg", [3, (8, 16)], ids=str)
@pytest.mark.parametrize("window", [(None, None), (4, 2)], ids=str)
def test_encoder_against_transformer_encoder_layer_with_a_float_src_mask(window, cfg):
    rng = np.random.default_rng(5)
    B, t, C, H, D, layers = 2, 12, 64, 2, 96, 2
    W = encoder_weights(rng, C, D, layers, H, cfg)
    x, dh = rng.normal(0, 1, (B * t, C)), rng.normal(0, 1, (B * t, C))
    got = RF.encoder(x, W, cfg, B, t, H, *window, layers=layers, ffn_width=D, act="gelu", pos_encoding=False, dh_out=dh)
    h = torch.from_numpy(x.reshape(B, t, C)).requires_grad_(True)
    cur, mods, tables = h, [], []
    for l in range(layers):
        an, nn_, fn, fnn = FF.layer_names(l)
        e = torch.nn.TransformerEncoderLayer(C, H, D, dropout=0.0, activation="gelu", batch_first=True, norm_first=False).double()
        names = {"self_attn": an, "norm1": nn_, "linear1": fn + ".linear1", "linear2": fn + ".linear2", "norm2": fnn}
        e.load_state_dict({n: torch.from_numpy(W[names[n.split(".", 1)[0]] + "." + n.split(".", 1)[1]]) for n in e.state_dict()})
        tw = torch.from_numpy(W[RF.rel_name(l) + ".weight"]).requires_grad_(True)
        cur = e(cur, src_mask=float_mask(tw, cfg, t, window).repeat(B, 1, 1))
        mods.append((e, names))
        tables.append(tw)
    cur.backward(torch.from_numpy(dh.reshape(B, t, C)))
    assert rel(got["h"], cur.detach().numpy().reshape(B * t, C)) < 1e-12
    assert rel(got["dx"], h.grad.numpy().reshape(B * t, C)) < 1e-12
    for l, ((e, names), tw) in enumerate(zip(mods, tables)):
        for n, p in e.named_parameters():
            top, rest = n.split(".", 1)
            assert rel(got["d_" + names[top] + "." + rest], p.grad.numpy()) < 1e-11, n
        assert rel(got["d_" + RF.rel_name(l) + ".weight"], tw.grad.numpy()) < 1e-11, l


def torch_masked_stack(x, Wt, cfg, B, t, H, window, layers, k, masks):
    """The post-LN stack with the convolution module in torch, written out with autograd: scores + table bias, -inf outside the window,
    softmax, and the dropout masks as constant factors at dropout_formula's five sites (masks[l][site], already times s; the attention
    site (B, H, t, t), the others (R, N)).  Wt: leaf tensors by name.  -> h (B, t, C)"""
    TF = torch.nn.functional
    C = x.shape[-1]
    dh = C // H
    idx = torch.from_numpy(RF.bucket_map(cfg, t).astype(np.int64)[RF.dist_index(t)])
    blocked = torch.from_numpy(WF.torch_mask(t, *window))
    ln = lambda v, name: TF.layer_norm(v, (C,), Wt[name + ".weight"], Wt[name + ".bias"], MF.EPS)
    rows = lambda m: m.reshape(B, t, -1)
    h = x
    for l in range(layers):
        an, nn_, fn, fnn = FF.layer_names(l)
        cm, cn = RF.V.conv_names(l)
        ms = masks[l]
        q, kk, v = (TF.linear(h, Wt[an + ".in_proj_weight"], Wt[an + ".in_proj_bias"]).view(B, t, 3, H, dh)[:, :, i].transpose(1, 2) for i in range(3))
        sc = q @ kk.transpose(2, 3) / np.sqrt(dh) + Wt[RF.rel_name(l) + ".weight"][:, idx][None]
        p = torch.softmax(sc.masked_fill(blocked[None, None], float("-inf")), dim=3) * ms[DF.SITE_ATTN]
        a = TF.linear((p @ v).transpose(1, 2).reshape(B, t, C), Wt[an + ".out_proj.weight"], Wt[an + ".out_proj.bias"])
        h = ln(h + a * rows(ms[DF.SITE_ATTN_OUT]), nn_)
        g = TF.glu(TF.conv1d(h.transpose(1, 2), Wt[cm + ".pointwise1.weight"], Wt[cm + ".pointwise1.bias"]), dim=1)
        z = TF.conv1d(g, Wt[cm + ".depthwise.weight"], Wt[cm + ".depthwise.bias"], padding=(k - 1) // 2, groups=C)
        z = TF.batch_norm(z, None, None, Wt[cm + ".bn.weight"], Wt[cm + ".bn.bias"], training=True, eps=RF.V.EPS)
        o = TF.conv1d(TF.silu(z), Wt[cm + ".pointwise2.weight"], Wt[cm + ".pointwise2.bias"]).transpose(1, 2)
        h = ln(h + o * rows(ms[DF.SITE_CONV_OUT]), cn)
        u = TF.gelu(TF.linear(h, Wt[fn + ".linear1.weight"], Wt[fn + ".linear1.bias"])) * rows(ms[DF.SITE_FFN_HIDDEN])
        h = ln(h + TF.linear(u, Wt[fn + ".linear2.weight"], Wt[fn + ".linear2.bias"]) * rows(ms[DF.SITE_FFN_OUT]), fnn)
    return h


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("H,window,cfg", [(2, (3, 0), 5), (4, (3, 0), 5), (4, (4, 2), (8, 16))], ids=str)
def test_encoder_with_the_module_heads_window_table_and_dropout_against_torch_autograd(H, window, cfg, p):
    """every option of the post-LN stack at once (what tests/test_gpu_sa_block_at_size.py's configuration AR rests on): H heads, a window,
    per-layer tables, the convolution module and, with p > 0, the masks of all five sites as constant factors in a torch graph"""
    rng = np.random.default_rng(11 + H)
    B, t, C, D, layers, k = 2, 12, 64, 96, 2, 7
    R = B * t
    W = encoder_weights(rng, C, D, layers, H, cfg)
    for l in range(layers):
        cm, cn = RF.V.conv_names(l)
        W.update({cm + ".pointwise1.weight": rng.normal(0, 0.2, (2 * C, C, 1)), cm + ".pointwise1.bias": rng.normal(0, 0.1, 2 * C),
                  cm + ".depthwise.weight": rng.normal(0, 0.3, (C, 1, k)), cm + ".depthwise.bias": rng.normal(0, 0.1, C),
                  cm + ".bn.weight": rng.normal(1, 0.2, C), cm + ".bn.bias": rng.normal(0, 0.1, C),
                  cm + ".bn.running_mean": rng.normal(0, 0.2, C), cm + ".bn.running_var": rng.uniform(0.5, 1.5, C),
                  cm + ".pointwise2.weight": rng.normal(0, 0.2, (C, C, 1)), cm + ".pointwise2.bias": rng.normal(0, 0.1, C),
                  cn + ".weight": rng.normal(1, 0.2, C), cn + ".bias": rng.normal(0, 0.1, C)})
    x, dh = rng.normal(0, 1, (R, C)), rng.normal(0, 1, (R, C))
    state = [0x5EDD0001, 0x00C0FFEE, 3, 0]
    got = RF.encoder(x, W, cfg, B, t, H, *window, state=state, p=p, layers=layers, ffn_width=D, act="gelu", pos_encoding=False, conv=True, dh_out=dh)
    s = float(DF.thr_scale(p)[1]) if p else 1.0
    masks = []
    for l in range(layers):
        if p:
            ms = {site: DF.keep_rows(state, DF.stream_id(l, site), R, D if site == DF.SITE_FFN_HIDDEN else C, p) for site in (1, 2, 3, 4)}
            ms[DF.SITE_ATTN] = DF.keep_attn(state, DF.stream_id(l, DF.SITE_ATTN), B, H, t, p)
            assert all(0 < int(m.sum()) < m.size for m in ms.values())
            masks.append({site: torch.from_numpy(m.astype(np.float64) * s) for site, m in ms.items()})
        else:
            shapes = {0: (B, H, t, t), 1: (R, C), 2: (R, C), 3: (R, D), 4: (R, C)}
            masks.append({site: torch.ones(shape, dtype=torch.float64) for site, shape in shapes.items()})
    Wt = {n: torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_(".running_" not in n) for n, a in W.items()}
    xt = torch.from_numpy(x.reshape(B, t, C)).requires_grad_(True)
    h = torch_masked_stack(xt, Wt, cfg, B, t, H, window, layers, k, masks)
    h.backward(torch.from_numpy(dh.reshape(B, t, C)))
    assert rel(got["h"], h.detach().numpy().reshape(R, C)) < 1e-11
    assert rel(got["dx"], xt.grad.numpy().reshape(R, C)) < 1e-11
    want = {n for n in W if ".running_" not in n}
    assert {n[2:] for n in got if n.startswith("d_")} == want
    for n in sorted(want):
        if n.endswith("depthwise.bias"):          # zero in exact arithmetic in front of a training BatchNorm: rounding noise on both sides
            scale = np.abs(got["d_" + n.replace(".bias", ".weight")]).max()
            assert np.abs(got["d_" + n]).max() < 1e-11 * scale and float(Wt[n].grad.abs().max()) < 1e-11 * scale
            continue
        assert rel(got["d_" + n].reshape(W[n].shape), Wt[n].grad.numpy()) < 1e-10, n


@pytest.mark.parametrize("window", [(3, 0), (40, 7), (None, None)], ids=str)
def test_raw_dctx_gate_holds_where_a_key_has_one_query(window):
    """bf16 with a dctx that is not bf16-representable (what the engine's GEMM hands the core): dV = P~^T dctx with both operands rounded
    to nearest even and the sum exact, against float64 on the raw dctx.  Window (3, 0) leaves the last key of a clip one query: its dv
    moves by the whole p~ eps, up to 2^-8 p~ |dctx| -- the figure the shift is capped at (a cap of 2^-9 is missed at 1.24 gates here)."""
    rng = np.random.default_rng(0)
    B, t, H, dh = 4, 130, 4, 32
    rb = lambda a: MF.round_bf16(a).astype(np.float64)
    q, k, v = (rb(rng.normal(0, 1, (B, t, H, dh)).astype(np.float32)) for _ in range(3))
    d = rng.normal(0, 1e-3, (B, t, H, dh)).astype(np.float32).astype(np.float64)
    assert not np.array_equal(rb(d), d)
    w = rng.normal(0, 1, (H, 2 * t - 1)).astype(np.float32)
    for name, ref, gates, tight in (("biased", RF.core(q, k, v, w, *window, d), RF.core_gates(q, k, v, w, *window, d, mode="bf16", raw_dctx=True),
                                     RF.core_gates(q, k, v, w, *window, d, mode="bf16")),
                                    ("unbiased", WF.core(q, k, v, *window, d), WF.core_gates(q, k, v, *window, d, mode="bf16", raw_dctx=True),
                                     WF.core_gates(q, k, v, *window, d, mode="bf16"))):
        got = np.einsum("bhij,bihc->bjhc", rb(ref["pt_bwd"]), rb(d))
        ratio = np.abs(got - ref["dv"]) / gates["dv"]
        print(f"window {window}, {name}: worst dv error / gate {ratio.max():.3f}")
        assert ratio.max() <= 1.0
        # without the raw-dctx terms the short sums are outside: they are what holds them
        assert window != (3, 0) or (np.abs(got - ref["dv"]) / tight["dv"]).max() > 1.0


# ---- the gates: a plain fp32 implementation passes, mutants fail --------------------------------------------------------------------
def gate_case(mode, t=70):
    bf = mode == "bf16"
    rb = MF.round_bf16 if bf else (lambda a: np.asarray(a, dtype=np.float32))
    return tuple(rb(a) for a in attn_case(t=t, sigma=1.5))


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("cfg", [1, 40, (8, 16), (32, 128)], ids=str)
@pytest.mark.parametrize("window", [(None, None), (3, 0), (33, 31), (40, 7)], ids=str)
def test_plain_fp32_passes_every_gate(window, cfg, p, mode):
    q, k, v, d = gate_case(mode)
    B, t, H, dh = q.shape
    wt = np.random.default_rng(7).normal(0.0, 1.0, (H, RF.num_buckets(cfg))).astype(np.float32)
    table = RF.expand(wt, cfg, t)
    keep, s = (DF.keep_attn([1, 2, 3, 0], 0, B, H, t, p), DF.thr_scale(p)[1]) if p else (None, 1.0)
    ref = RF.core(q, k, v, table, *window, d, keep=keep, s=s, cfg=cfg)
    g = RF.core_gates(q, k, v, table, *window, d, keep=keep, s=s, mode=mode, cfg=cfg)
    got = RF.core(q, k, v, table, *window, d, keep=keep, s=s, dtype=np.float32, bf16_operands=mode == "bf16", cfg=cfg)
    for n in NAMES:
        assert RF.check(got[n], ref[n], g[n], (window, cfg, mode, p, n))[0], n


def test_mutants_fail_the_fp32_gates():
    q, k, v, d = gate_case("f32")
    B, t, H, dh = q.shape
    window, cfg = (40, 7), 3
    wt = np.random.default_rng(7).normal(0.0, 1.0, (H, RF.num_buckets(cfg))).astype(np.float32)
    table = RF.expand(wt, cfg, t)
    ref, g = RF.core(q, k, v, table, *window, d, cfg=cfg), RF.core_gates(q, k, v, table, *window, d, cfg=cfg)
    closest = None
    for mutant in ("i_minus_j", "diag_off_by_one", "bias_before_scale", "dw_scaled", "next_head", "dw_unclamped_only", "dw_out_of_window"):
        with np.errstate(over="ignore", invalid="ignore"):
            got = RF.core(q, k, v, table, *window, d, dtype=np.float32, mutant=mutant, cfg=cfg)
        out = {}
        for n in NAMES:
            err = np.abs(got[n].astype(np.float64) - ref[n])
            with np.errstate(divide="ignore", invalid="ignore"):     # (a distance without a cell has gate 0: 0 / 0 is skipped, x / 0 is out)
                out[n] = float(np.nanmax(np.where(np.isfinite(err), err / g[n], np.inf)))
        worst = max(out.values())
        print(f"{mutant}: worst error / gate by output {out}")
        assert worst > 100.0, f"the mutant {mutant} is not 100 gates out anywhere"
        closest = worst if closest is None else min(closest, worst)
        if mutant in ("dw_scaled", "dw_unclamped_only", "dw_out_of_window"):     # the forward and dqkv are right, only the table's gradient is not
            assert max(out[n] for n in ("ctx", "lse", "dq", "dk", "dv")) <= 1.0 and out["dw"] > 100.0
    print(f"the closest mutant is {closest:.3g} gates out")


# ---- the bucket maps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", BUCKETS, ids=str)
def test_bucket_map_properties(sed, cfg):
    t = 1100
    nb = RF.num_buckets(cfg)
    mp = RF.bucket_map(cfg, t)
    d = np.arange(-(t - 1), t)
    assert mp.dtype == np.int32 and mp.shape == (2 * t - 1,) and mp.min() >= 0 and mp.max() < nb
    assert np.array_equal(mp, sed.CnnEngine.rel_pos_map(sed.CnnEngine.check_sa_rel_pos(cfg), t)), "the package's map is not the definition"
    assert sed.CnnEngine.rel_pos_buckets(sed.CnnEngine.check_sa_rel_pos(cfg)) == nb
    if isinstance(cfg, int):
        assert nb == 2 * cfg + 1 and np.array_equal(mp, np.clip(d, -cfg, cfg) + cfg)
        return
    nbk, maxd = cfg
    n, m = nbk // 2, nbk // 4
    neg, pos = mp[d <= 0][::-1], mp[d > 0]                        # by |d| ascending: 0, 1, ... and 1, 2, ...
    assert np.array_equal(neg[:m], np.arange(m)) and np.array_equal(pos[:m - 1], n + np.arange(1, m)), "not exact below m"
    assert (np.diff(neg) >= 0).all() and (np.diff(pos) >= 0).all(), "not monotone in |d|"
    assert (neg[maxd:] == n - 1).all() and (pos[maxd - 1:] == nbk - 1).all(), "not saturated from max_distance on"
    assert np.array_equal(pos, neg[1:] + n), "the d > 0 half is not the other half offset by n"


def test_log_buckets_are_t5s():
    t5 = pytest.importorskip("transformers.models.t5.modeling_t5")
    d = torch.arange(-1024, 1025)
    for nb, maxd in ((8, 16), (32, 128), (4, 2), (64, 800)):
        want = t5.T5Attention._relative_position_bucket(d, bidirectional=True, num_buckets=nb, max_distance=maxd).numpy()
        got = np.array([RF.bucket((nb, maxd), int(x)) for x in d])
        assert np.array_equal(got, want), (nb, maxd)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def test_model_refusals_keys_and_draws(sed):
    for bad in (0, -1, 1.5, "3", True, (8,), (8, 16, 2), (7, 16), (2, 16), (8, 2), (8, 1.5), (8.0, 16), 2048, (4098, 2000), (None, 3)):
        rng_state = torch.random.get_rng_state()
        with pytest.raises(ValueError, match="sa_rel_pos"):
            sed.Csa_AvgPooling(3, CFG, sa_heads=2, sa_rel_pos=bad)
        assert torch.equal(rng_state, torch.random.get_rng_state()), "a refused model drew random numbers"
    with pytest.raises(ValueError, match="sa_rel_pos"):
        sed.CnnEngine(3, CFG, head="sa", sa_heads=2, sa_rel_pos=0)
    with pytest.raises(ValueError, match="sa_rel_pos"):
        sed.CnnEngine(3, CFG, head="fc", sa_rel_pos=3)
    for cls in (sed.Cnn_AvgPooling, sed.Crnn_AvgPooling):
        with pytest.raises(TypeError):
            cls(3, CFG, sa_rel_pos=3)
    kw = dict(precision="fp32", sa_heads=2, sa_layers=2, sa_ffn=96, sa_conv_kernel=7)
    torch.manual_seed(11)
    plain = sed.Csa_AvgPooling(3, CFG, **kw)
    after_plain = torch.random.get_rng_state()
    torch.manual_seed(11)
    none = sed.Csa_AvgPooling(3, CFG, sa_rel_pos=None, **kw)
    torch.manual_seed(11)
    relm = sed.Csa_AvgPooling(3, CFG, sa_rel_pos=(8, 16), **kw)
    assert torch.equal(after_plain, torch.random.get_rng_state()), "sa_rel_pos must not draw a random number"
    # without the option: the old keys and values, no buffer, nothing in the engine
    assert list(none.state_dict()) == list(plain.state_dict()) and "rel_pos_config" not in none.state_dict()
    assert [n for n, _ in none.named_parameters()] == [n for n, _ in plain.named_parameters()]
    assert none.engine.sa_rel_pos is None and sed.Csa_AvgPooling.rel_pos_config_from_state_dict(none.state_dict()) is None
    # with it: the same draws, one parameter per layer between attn* and attn_norm*, one more buffer
    new = {"rel_pos.weight", "rel_pos_l1.weight", "rel_pos_config"}
    keys = list(relm.state_dict())
    assert [k for k in keys if k not in new] == list(plain.state_dict()) and new <= set(keys)
    for n, v in plain.state_dict().items():
        assert torch.equal(v, relm.state_dict()[n]), n
    names = [n.split(".")[0] for n, _ in relm.named_parameters()]
    order = [n for i, n in enumerate(names) if i == 0 or names[i - 1] != n]
    head = [n for n in order if not n.startswith("conv_blocks")]
    assert head == ["attn", "rel_pos", "attn_norm", "convm", "conv_norm", "ffn", "ffn_norm",
                    "attn_l1", "rel_pos_l1", "attn_norm_l1", "convm_l1", "conv_norm_l1", "ffn_l1", "ffn_norm_l1", "event_fc"]
    for l in range(2):
        w = relm.state_dict()[sed.CnnEngine.sa_rel_name(l) + ".weight"]
        assert w.shape == (2, 8) and w.dtype == torch.float32 and not w.any()
    cfg = relm.state_dict()["rel_pos_config"]
    assert cfg.dtype == torch.float64 and cfg.tolist() == [1.0, 8.0, 16.0]
    assert sed.Csa_AvgPooling.rel_pos_config_from_state_dict(relm.state_dict()) == (8, 16)
    # encoder_layer_state: TransformerEncoderLayer's keys, nothing else
    want = set(torch.nn.TransformerEncoderLayer(128, 2, 96, batch_first=True).state_dict())
    for l in range(2):
        assert set(sed.Csa_AvgPooling.encoder_layer_state(relm.state_dict(), l)) == want
    # round trips through the buffer and into a rebuilt model; a clone keeps the option
    for given, back_want, buf in ((5, 5, [0.0, 5.0, 0.0]), (1, 1, [0.0, 1.0, 0.0]), ((32, 128), (32, 128), [1.0, 32.0, 128.0]), ([4, 2], (4, 2), [1.0, 4.0, 2.0])):
        m = sed.Csa_AvgPooling(3, CFG, sa_heads=2, sa_rel_pos=given)
        assert m.state_dict()["rel_pos_config"].tolist() == buf
        back = sed.Csa_AvgPooling.rel_pos_config_from_state_dict(m.state_dict())
        assert back == back_want
        again = sed.Csa_AvgPooling(3, CFG, sa_heads=2, sa_rel_pos=back)
        again.load_state_dict(m.state_dict())
        assert again.sa_rel_pos == m.sa_rel_pos == m.engine.sa_rel_pos == m.clone_without_engines().engine.sa_rel_pos
    with pytest.raises(RuntimeError):
        plain.load_state_dict(relm.state_dict())


def test_rel_pos_bias_is_the_float_mask(sed):
    torch.manual_seed(3)
    for cfg in (3, (8, 16)):
        m = sed.Csa_AvgPooling(3, CFG, sa_heads=2, sa_layers=2, sa_rel_pos=cfg)
        with torch.no_grad():
            for l in range(2):
                getattr(m, sed.CnnEngine.sa_rel_name(l)).weight.normal_()
        sd = m.state_dict()
        for l in range(2):
            t = 19
            got = sed.Csa_AvgPooling.rel_pos_bias(sd, l, t)
            w = sd[sed.CnnEngine.sa_rel_name(l) + ".weight"].numpy()
            assert got.shape == (2, t, t) and got.dtype == torch.float32
            assert np.array_equal(got.numpy(), RF.bias_matrix(RF.expand(w, cfg, t), t))
    with pytest.raises(ValueError, match="rel_pos_config"):
        sed.Csa_AvgPooling.rel_pos_bias(sed.Csa_AvgPooling(3, CFG, sa_heads=2).state_dict(), 0, 5)


def test_command_line_flags(sed):
    main = importlib.import_module(PKG + ".main")
    full = main.build_full_parser()
    base = ["--train_features", "Spectogram", "--dataset_name", "synthetic"]
    for text, want in (("32", 32), ("1", 1), ("8:16", (8, 16)), ("32:128", (32, 128))):
        args = full.parse_args(base + ["--self_attention", "--no_pos_encoding", "--sa_rel_pos", text])
        main.validate_args(args)
        assert main.parse_sa_rel_pos(args.sa_rel_pos) == want
    assert full.parse_args(base).sa_rel_pos is None and main.parse_sa_rel_pos(None) is None
    main.validate_args(full.parse_args(base))
    for bad in ("0", "-1", "7:16", "8:2", "1:2:3", "x", "1.5", "", "2:16", "5000"):
        with pytest.raises(ValueError, match="sa_rel_pos"):
            main.validate_args(full.parse_args(base + ["--self_attention", "--sa_rel_pos=" + bad]))
    with pytest.raises(ValueError, match="--self_attention"):
        main.validate_args(full.parse_args(base + ["--sa_rel_pos", "32"]))
