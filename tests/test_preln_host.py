"""Host (no GPU): tests/preln_formula.py -- the float64 definition of the pre-LN residual LayerNorm pair and of the pre-LN / macaron stack
-- against torch.nn.TransformerEncoder(TransformerEncoderLayer(norm_first=True), N, norm=LayerNorm) and a torch-module composition of
the macaron + convolution block with autograd; its gates against a plain fp32 implementation and against the mutants; and the model
plumbing of Csa_AvgPooling(sa_norm_first=, sa_macaron=): keys, block_config, registration and FlatParams order, draw order, refusals."""
import importlib

import numpy as np
import pytest
import torch

import preln_formula as PF
import window_formula as W

PKG = "soundeventdetection-pytorch_amd"
CFG = [(32, 2), (64, 2)]
C = 64
OLD_KEYS = ["attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "attn_norm.weight", "attn_norm.bias",
            "attn_config", "event_fc.weight", "event_fc.bias"]
HEAD_PREFIXES = ("attn", "ffn", "convm", "conv_norm", "rel_pos", "out_norm")


@pytest.fixture(scope="module")
def sed():
    return importlib.import_module(PKG)


def rel(a, b):
    """the largest difference relative to the reference's largest magnitude (floor 1: the depthwise bias in front of a training
    BatchNorm has a gradient of exactly zero, which both sides reach as the rounding noise of a sum of O(1) terms)"""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def randomized(sed, seed=0, heads=2, cfg=CFG, **kw):
    """a model on the CPU whose head parameters are all away from their zero / unit initial values"""
    torch.manual_seed(seed)
    m = sed.Csa_AvgPooling(3, cfg, precision="fp32", sa_heads=heads, mel_bins=8, sa_norm_first=True, **kw)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.startswith(HEAD_PREFIXES):
                p.normal_(1.0 if ("norm" in n or ".bn." in n) and n.endswith("weight") else 0.0, 0.2)
    return m


def head_weights(sd):
    return {k: v.numpy() for k, v in sd.items() if k.startswith(HEAD_PREFIXES) and "config" not in k and "num_batches" not in k}


# ---- the definition against torch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [1, 3])
@pytest.mark.parametrize("act", ["relu", "gelu"])
def test_definition_against_torch_norm_first_encoder(sed, layers, act):
    B, t, H, D = 2, 7, 2, 96
    m = randomized(sed, seed=layers, heads=H, sa_layers=layers, sa_ffn=D, sa_activation=act)
    sd = {k: v.double() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(layers)
    x, dh_out = rng.normal(0, 1, (B * t, C)), rng.normal(0, 1, (B * t, C))
    ref = PF.encoder(x, head_weights(sd), B, t, H, layers, D, act, dh_out=dh_out)
    proto = torch.nn.TransformerEncoderLayer(C, H, D, dropout=0.0, activation=act, batch_first=True, norm_first=True)
    run = torch.nn.TransformerEncoder(proto, layers, norm=torch.nn.LayerNorm(C), enable_nested_tensor=False).double()
    for l, ly in enumerate(run.layers):
        ly.load_state_dict(sed.Csa_AvgPooling.encoder_layer_state(sd, l))        # norm1 = attn_norm, norm2 = ffn_norm: strict loading
        assert sed.Csa_AvgPooling.closing_norm_state(sd, l).keys() == ({"weight", "bias"} if l == layers - 1 else set())
    run.norm.load_state_dict(sed.Csa_AvgPooling.closing_norm_state(sd, layers - 1))
    run.train()
    xt = torch.from_numpy(x).view(B, t, C).clone().requires_grad_(True)
    h = run(xt + torch.from_numpy(PF.M.positional_table(t, C)))
    h.backward(torch.from_numpy(dh_out).view(B, t, C))
    assert rel(ref["h"], h.detach().numpy().reshape(B * t, C)) < 1e-12
    assert rel(ref["dx"], xt.grad.numpy().reshape(B * t, C)) < 1e-12
    back = {"self_attn": "attn", "norm1": "attn_norm", "linear1": "ffn", "linear2": "ffn", "norm2": "ffn_norm"}
    seen = 0
    for l, ly in enumerate(run.layers):
        for n, p in ly.named_parameters():
            top, rest = n.split(".", 1)
            ours = back[top] + PF.sfx(l) + "." + (n if top.startswith("linear") else rest)
            assert rel(ref["d_" + ours], p.grad.numpy()) < 1e-12, ours
            seen += 1
    for n, p in run.norm.named_parameters():
        assert rel(ref["d_out_norm" + PF.sfx(layers - 1) + "." + n], p.grad.numpy()) < 1e-12
        seen += 1
    assert seen == 12 * layers + 2 == len([k for k in ref if k.startswith("d_")])


class TorchConformerBlock(torch.nn.Module):
    """the macaron + convolution block out of torch modules: x + 1/2 FFN(LN x), + MHSA(LN x) with a float attn_mask (window, bias),
    + ConvModule(LN x), + 1/2 FFN(LN x), LN"""

    def __init__(self, H, D, k, C=C):
        super().__init__()
        nn = torch.nn
        self.n_mac, self.n_att, self.n_conv, self.n_ffn, self.n_out = (nn.LayerNorm(C) for _ in range(5))
        self.mac1, self.mac2, self.ffn1, self.ffn2 = nn.Linear(C, D), nn.Linear(D, C), nn.Linear(C, D), nn.Linear(D, C)
        self.mha = nn.MultiheadAttention(C, H, batch_first=True)
        self.pw1, self.dw, self.bn, self.pw2 = nn.Conv1d(C, 2 * C, 1), nn.Conv1d(C, C, k, padding=(k - 1) // 2, groups=C), nn.BatchNorm1d(C), nn.Conv1d(C, C, 1)

    def forward(self, x, mask):
        F = torch.nn.functional
        x = x + 0.5 * self.mac2(F.relu(self.mac1(self.n_mac(x))))
        n = self.n_att(x)
        x = x + self.mha(n, n, n, attn_mask=mask, need_weights=False)[0]
        c = self.pw1(self.n_conv(x).transpose(1, 2))
        c = self.pw2(F.silu(self.bn(self.dw(F.glu(c, dim=1))))).transpose(1, 2)
        x = x + c
        x = x + 0.5 * self.ffn2(F.relu(self.ffn1(self.n_ffn(x))))
        return self.n_out(x)


@pytest.mark.parametrize("layers", [1, 2])
def test_definition_against_torch_conformer_block(sed, layers):
    conformer_block_against_torch(sed, layers, 2, (3, 2), 2)


@pytest.mark.parametrize("H,win,rp", [(4, (3, 0), 2), (4, (5, 2), (8, 16)), (2, (3, 0), (8, 16))], ids=str)
def test_conformer_block_with_more_heads_window_and_table_against_torch(sed, H, win, rp):
    """the heads, the window and the per-layer tables together (what tests/test_gpu_sa_block_at_size.py rests on): four heads, a causal
    window, log buckets; the tables drawn N(0, 1) so that a table read for the wrong head or layer moves the output by O(1)"""
    conformer_block_against_torch(sed, 2, H, win, rp, table_sigma=1.0)


@pytest.mark.parametrize("H", [2, 4])
@pytest.mark.parametrize("win,rp", [((3, 0), 2), ((5, 2), (8, 16))], ids=str)
def test_plain_stack_with_heads_window_and_table_against_torch_norm_first_layers(sed, H, win, rp):
    """the plain pre-LN stack (no macaron, no module) with H heads, a window and per-layer tables against
    TransformerEncoderLayer(norm_first=True) called layer by layer with its own float src_mask (the table's bias, -inf outside the
    window), then the closing LayerNorm"""
    B, t, D, layers, C = 2, 9, 96, 2, 32 * H
    m = randomized(sed, seed=20 + H, heads=H, cfg=[(32, 2), (C, 2)], sa_layers=layers, sa_ffn=D, sa_activation="gelu", sa_window=win, sa_rel_pos=rp, pos_encoding=False)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.startswith("rel_pos"):
                p.normal_(0.0, 1.0)
    sd = {k: v.double() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(H)
    x, dh_out = rng.normal(0, 1, (B * t, C)), rng.normal(0, 1, (B * t, C))
    ref = PF.encoder(x, head_weights(sd), B, t, H, layers, D, "gelu", window=win, rel_cfg=rp, pos_encoding=False, dh_out=dh_out)
    Csa = sed.Csa_AvgPooling
    window = torch.where(torch.from_numpy(W.in_window(t, *win)), 0.0, -np.inf).double()
    lys, biases = [], []
    for l in range(layers):
        ly = torch.nn.TransformerEncoderLayer(C, H, D, dropout=0.0, activation="gelu", batch_first=True, norm_first=True).double().train()
        ly.load_state_dict(Csa.encoder_layer_state(sd, l))
        lys.append(ly)
        biases.append(Csa.rel_pos_bias(sd, l, t).clone().requires_grad_(True))
    assert not torch.equal(biases[0].detach(), biases[1].detach()) and not torch.equal(biases[0][0].detach(), biases[0][1].detach())
    norm = torch.nn.LayerNorm(C).double()
    norm.load_state_dict(Csa.closing_norm_state(sd, layers - 1))
    xt = torch.from_numpy(x).view(B, t, C).clone().requires_grad_(True)
    h = xt
    for ly, bias in zip(lys, biases):
        h = ly(h, src_mask=(bias + window).repeat(B, 1, 1))
    h = norm(h)
    h.backward(torch.from_numpy(dh_out).view(B, t, C))
    assert rel(ref["h"], h.detach().numpy().reshape(B * t, C)) < 1e-12
    assert rel(ref["dx"], xt.grad.numpy().reshape(B * t, C)) < 1e-12
    back = {"self_attn": "attn", "norm1": "attn_norm", "linear1": "ffn", "linear2": "ffn", "norm2": "ffn_norm"}
    seen = set()
    for l, (ly, bias) in enumerate(zip(lys, biases)):
        for n, p in ly.named_parameters():
            top, rest = n.split(".", 1)
            key = "d_" + back[top] + PF.sfx(l) + "." + (n if top.startswith("linear") else rest)
            assert rel(ref[key], p.grad.numpy()) < 1e-12, key
            seen.add(key)
        key = "d_rel_pos" + PF.sfx(l) + ".weight"
        assert rel(ref[key], PF.RP.fold(PF.RP.diag_sums(bias.grad.numpy()), rp, t)) < 1e-12, key
        seen.add(key)
    for n, p in norm.named_parameters():
        key = "d_out_norm" + PF.sfx(layers - 1) + "." + n
        assert rel(ref[key], p.grad.numpy()) < 1e-12, key
        seen.add(key)
    assert seen == {kk for kk in ref if kk.startswith("d_")}


def conformer_block_against_torch(sed, layers, H, win, rp, table_sigma=None):
    B, t, D, k, C = 2, 9, 96, 5, 32 * H
    m = randomized(sed, seed=10 + layers, heads=H, cfg=[(32, 2), (C, 2)], sa_layers=layers, sa_ffn=D, sa_macaron=True, sa_conv_kernel=k, sa_window=win, sa_rel_pos=rp,
                   pos_encoding=False)
    if table_sigma is not None:
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.startswith("rel_pos"):
                    p.normal_(0.0, table_sigma)
    sd = {kk: v.double() for kk, v in m.state_dict().items()}
    rng = np.random.default_rng(layers)
    x, dh_out = rng.normal(0, 1, (B * t, C)), rng.normal(0, 1, (B * t, C))
    cfg = rp                                   # (relpos_formula takes the option as given)
    ref = PF.encoder(x, head_weights(sd), B, t, H, layers, D, "relu", macaron=True, conv=True, window=win, rel_cfg=cfg, pos_encoding=False,
                     dh_out=dh_out)
    Csa = sed.Csa_AvgPooling
    blocks, masks, names = [], [], []
    for l in range(layers):
        blk = TorchConformerBlock(H, D, k, C).double().train()
        enc, mac, cv, out = Csa.encoder_layer_state(sd, l), Csa.macaron_ffn_state(sd, l), Csa.conv_module_state(sd, l), Csa.closing_norm_state(sd, l)
        sfx = PF.sfx(l)
        load = {"n_mac": ("ffn_mac_norm", {kk[5:]: v for kk, v in mac.items() if kk.startswith("norm.")}),
                "mac1": ("ffn_mac", {kk[8:]: v for kk, v in mac.items() if kk.startswith("linear1.")}),
                "mac2": ("ffn_mac", {kk[8:]: v for kk, v in mac.items() if kk.startswith("linear2.")}),
                "n_att": ("attn_norm", {kk[6:]: v for kk, v in enc.items() if kk.startswith("norm1.")}),
                "mha": ("attn", {kk[10:]: v for kk, v in enc.items() if kk.startswith("self_attn.")}),
                "n_conv": ("conv_norm", {kk[10:]: v for kk, v in cv.items() if kk.startswith("conv_norm.")}),
                "pw1": ("convm", {kk[11:]: v for kk, v in cv.items() if kk.startswith("pointwise1.")}),
                "dw": ("convm", {kk[10:]: v for kk, v in cv.items() if kk.startswith("depthwise.")}),
                "bn": ("convm", {kk[3:]: v for kk, v in cv.items() if kk.startswith("bn.")}),
                "pw2": ("convm", {kk[11:]: v for kk, v in cv.items() if kk.startswith("pointwise2.")}),
                "n_ffn": ("ffn_norm", {kk[6:]: v for kk, v in enc.items() if kk.startswith("norm2.")}),
                "ffn1": ("ffn", {kk[8:]: v for kk, v in enc.items() if kk.startswith("linear1.")}),
                "ffn2": ("ffn", {kk[8:]: v for kk, v in enc.items() if kk.startswith("linear2.")}),
                "n_out": ("out_norm", out)}
        for attr, (ours, state) in load.items():
            getattr(blk, attr).load_state_dict(state)                # strict
            names.append((blk, attr, ours + sfx))
        bias = Csa.rel_pos_bias(sd, l, t).clone().requires_grad_(True)                         # (H, t, t)
        mask = torch.where(torch.from_numpy(W.in_window(t, *win)), 0.0, -np.inf).double()
        blocks.append(blk)
        masks.append((bias, mask))
    xt = torch.from_numpy(x).view(B, t, C).clone().requires_grad_(True)
    h = xt
    for blk, (bias, mask) in zip(blocks, masks):
        h = blk(h, (bias + mask).repeat(B, 1, 1))
    h.backward(torch.from_numpy(dh_out).view(B, t, C))
    assert rel(ref["h"], h.detach().numpy().reshape(B * t, C)) < 1e-12
    assert rel(ref["dx"], xt.grad.numpy().reshape(B * t, C)) < 1e-12
    seen = set()
    for blk, attr, ours in names:
        prefix = {"mac1": "linear1.", "mac2": "linear2.", "ffn1": "linear1.", "ffn2": "linear2.", "pw1": "pointwise1.", "dw": "depthwise.", "bn": "bn.",
                  "pw2": "pointwise2."}.get(attr, "")
        for n, p in getattr(blk, attr).named_parameters():
            key = f"d_{ours}.{prefix}{n}"
            assert rel(ref[key], p.grad.numpy().reshape(ref[key].shape)) < 1e-12, key
            seen.add(key)
    # the tables: the bias gradient folded over the buckets
    for l, (bias, _) in enumerate(masks):
        want = PF.RP.fold(PF.RP.diag_sums(bias.grad.numpy()), cfg, t)
        key = "d_rel_pos" + PF.sfx(l) + ".weight"
        assert rel(ref[key], want) < 1e-12, key
        seen.add(key)
    assert seen == {kk for kk in ref if kk.startswith("d_")}
    # the BatchNorm's running statistics of a training forward
    for l, blk in enumerate(blocks):
        assert rel(ref["convm" + PF.sfx(l) + ".bn.running_mean"], blk.bn.running_mean.numpy()) < 1e-12


# ---- the gates: a plain fp32 implementation passes, the mutants fail --------------------------------------------------------------------
def kernel_case(seed=0, rows=37, Cc=68, p=0.0, s=0.5, big=False):
    rng = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32)
    scale = 1e4 if big else 1.0
    x, a = f32(rng.normal(0, scale, (rows, Cc))), f32(rng.normal(0, scale, (rows, Cc)))
    x[3] = 1e4 if big else 1.0                  # a row of variance 0 (with a = 0 there)
    a[3] = 0.0
    gamma, beta = f32(rng.normal(1, 0.3, Cc)), f32(rng.normal(0, 0.3, Cc))
    dy, dres_in = f32(rng.normal(0, 1, (rows, Cc))), f32(rng.normal(0, 1, (rows, Cc)))
    if p:
        state = [7, 9, 2, 0]
        keep, sd = PF.D.keep_rows(state, PF.D.stream_id(1, 6), rows, Cc, p), float(PF.D.thr_scale(p)[1])
    else:
        keep, sd = None, 1.0
    return dict(x=x, a=a, s=s, gamma=gamma, beta=beta, keep=keep, sd=sd, dy=dy, dres_in=dres_in)


def run_pair(c, dtype, mutant=None, with_a=True, fed=None):
    """forward + backward; fed: (xsum, stats) the backward is given (the fp32 forward's own, as the kernel is fed)"""
    a = c["a"] if with_a else None
    return PF.resid_layernorm(c["x"], a, c["s"], c["gamma"], c["beta"], c["keep"], c["sd"], c["dy"], c["dres_in"],
                              xsum=None if fed is None else fed[0], stats=None if fed is None else fed[1], dtype=dtype, mutant=mutant)


@pytest.mark.parametrize("p,s,big,with_a", [(0.0, 0.5, False, True), (0.0, 1.0, True, True), (0.3, -0.75, False, True), (0.3, 0.5, True, True),
                                          (0.0, 1.0, False, False)])
def test_plain_fp32_implementation_passes_every_gate(p, s, big, with_a):
    c = kernel_case(1, p=p, s=s, big=big)
    got = run_pair(c, np.float32, with_a=with_a)
    fed = (got["xsum"], np.stack([got["mean"], got["rstd"]], axis=1))
    a = c["a"] if with_a else None
    ref = run_pair(c, np.float64, with_a=with_a, fed=fed)
    gates = PF.resid_layernorm_gates(c["x"], a, c["s"], c["gamma"], c["beta"], c["keep"], c["sd"], c["dy"], c["dres_in"], xsum=fed[0], stats=fed[1])
    for key in ("xsum", "y", "mean", "dxsum", "dgamma", "dbeta") + (("da",) if with_a else ()):
        ok, worst = PF.check(got[key], ref[key], gates[key], f"fp32 {key} p={p} s={s}")
        assert ok, (key, worst)


@pytest.mark.parametrize("mutant,key", [("drop_dres_in", "dxsum"), ("da_without_s", "da"), ("xhat_from_x", "dxsum")])
def test_kernel_mutants_fail_a_gate(mutant, key):
    c = kernel_case(2, p=0.0, s=0.5)
    good = run_pair(c, np.float32)
    fed = (good["xsum"], np.stack([good["mean"], good["rstd"]], axis=1))
    ref = run_pair(c, np.float64, fed=fed)
    gates = PF.resid_layernorm_gates(c["x"], c["a"], c["s"], c["gamma"], c["beta"], None, 1.0, c["dy"], c["dres_in"], xsum=fed[0], stats=fed[1])
    bad = run_pair(c, np.float32, mutant=mutant, fed=fed)
    ok, worst = PF.check(bad[key], ref[key], gates[key], f"mutant {mutant} {key}")
    assert not ok and worst > 100.0


STACK_MUTANTS = [("no_half_mac", True), ("no_half_ffn", True), ("post_ln", True), ("post_ln", False), ("no_closing", True), ("no_closing", False),
                 ("inner_closing", False), ("shared_ffn", True)]


@pytest.mark.parametrize("mutant,macaron", STACK_MUTANTS)
def test_stack_mutants_fail_the_fp32_gate(sed, mutant, macaron):
    B, t, H, D, layers = 2, 7, 2, 96, 2
    m = randomized(sed, seed=3, heads=H, sa_layers=layers, sa_ffn=D, sa_macaron=macaron, sa_conv_kernel=3 if macaron else 0)
    Wt = head_weights({k: v.double() for k, v in m.state_dict().items()})
    x = np.random.default_rng(4).normal(0, 1, (B * t, C))
    kw = dict(layers=layers, ffn_width=D, act="relu", macaron=macaron, conv=macaron)
    ref = PF.encoder(x, Wt, B, t, H, **kw)["h"]
    bad = PF.encoder(x, Wt, B, t, H, mutant=mutant, **kw)["h"]
    ok, worst = PF.check(bad, ref, PF.stack_gate(ref, layers, C, D, t), f"stack mutant {mutant}")
    assert not ok and worst > 10.0


# ---- model plumbing ------------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_block_config_and_orders(sed):
    torch.manual_seed(0)
    default = sed.Csa_AvgPooling(3, CFG, precision="fp32", sa_heads=2, mel_bins=8)
    assert sorted(k for k in default.state_dict() if not k.startswith("conv_blocks.")) == sorted(OLD_KEYS), "a default model's state_dict changed"
    assert sed.Csa_AvgPooling.block_config_from_state_dict(default.state_dict()) == (False, False)
    assert (default.sa_norm_first, default.sa_macaron, default.engine.sa_norm_first, default.engine.sa_macaron) == (False,) * 4
    full = sed.Csa_AvgPooling(3, CFG, precision="fp32", sa_heads=2, mel_bins=8, sa_layers=2, sa_ffn=96, sa_conv_kernel=5, sa_rel_pos=2,
                              sa_norm_first=True, sa_macaron=True, attention=True)
    sd = full.state_dict()
    assert sd["block_config"].dtype == torch.float64 and sd["block_config"].tolist() == [1.0, 1.0]
    assert sed.Csa_AvgPooling.block_config_from_state_dict(sd) == (True, True)
    order = PF.module_order(2, True, True, 96, True)
    assert order == ["ffn_mac_norm", "ffn_mac", "attn_norm", "attn", "rel_pos", "conv_norm", "convm", "ffn_norm", "ffn", "out_norm",
                     "ffn_mac_norm_l1", "ffn_mac_l1", "attn_norm_l1", "attn_l1", "rel_pos_l1", "conv_norm_l1", "convm_l1", "ffn_norm_l1", "ffn_l1",
                     "out_norm_l1"]
    assert [n for n, _ in full.named_children()] == ["conv_blocks"] + order + ["event_fc", "att_fc"]
    assert full.sa_config.module_order() == order
    keys = [k for k, _, _ in sed.train.FlatParams(full, n_buckets=0).groups]
    assert keys == ["att_fc", "event_fc"] + order[::-1] + ["conv_blocks.1", "conv_blocks.0"]
    for l in range(2):
        mac = sed.Csa_AvgPooling.macaron_ffn_state(sd, l)
        assert sorted(mac) == ["linear1.bias", "linear1.weight", "linear2.bias", "linear2.weight", "norm.bias", "norm.weight"]
        assert sorted(sed.Csa_AvgPooling.closing_norm_state(sd, l)) == ["bias", "weight"]
        assert sorted({k.split(".")[0] for k in sed.Csa_AvgPooling.encoder_layer_state(sd, l)}) == ["linear1", "linear2", "norm1", "norm2", "self_attn"]
    # no macaron: a closing norm on the last layer only
    plain = sed.Csa_AvgPooling(3, CFG, precision="fp32", sa_heads=2, sa_layers=3, sa_norm_first=True)
    assert [n for n, _ in plain.named_children()] == ["conv_blocks", "attn_norm", "attn", "attn_norm_l1", "attn_l1", "attn_norm_l2", "attn_l2",
                                                      "out_norm_l2", "event_fc"]
    assert plain.state_dict()["block_config"].tolist() == [1.0, 0.0]
    twin = sed.Csa_AvgPooling(3, CFG, precision="fp32", sa_heads=2, mel_bins=8, sa_layers=2, sa_ffn=96, sa_conv_kernel=5, sa_rel_pos=2,
                              sa_norm_first=True, sa_macaron=True, attention=True)
    twin.load_state_dict(sd)
    clone = full.clone_without_engines()
    assert (clone.engine.sa_norm_first, clone.engine.sa_macaron) == (True, True) and clone.engine is not full.engine


def replay(sed, seed, K, heads, layers, ffn, kc, macaron):
    """the documented draw order by hand: conv blocks, then per layer the macaron FFN, the attention, the convolution module, the FFN"""
    sm = sed.models.spectogram_models
    torch.manual_seed(seed)
    out = {}
    cin = 1
    for i, (c, pool) in enumerate(CFG):
        blk = sed.ConvBlock(in_channels=cin, out_channels=c, pool_size=pool)
        out.update({f"conv_blocks.{i}.{n}": p for n, p in blk.named_parameters()})
        cin = c
    for l in range(layers):
        x = PF.sfx(l)
        if macaron:
            out.update({f"ffn_mac{x}.{n}": p for n, p in sm._FfnParams(cin, ffn).named_parameters()})
        out.update({f"attn{x}.{n}": p for n, p in sm._MhaParams(cin, heads).named_parameters()})
        if kc:
            out.update({f"convm{x}.{n}": p for n, p in sm._ConvModuleParams(cin, kc).named_parameters()})
        if ffn:
            out.update({f"ffn{x}.{n}": p for n, p in sm._FfnParams(cin, ffn).named_parameters()})
    fc = sm._LinearParams(cin, K)
    sed.init_layer(fc)
    out.update({f"event_fc.{n}": p for n, p in fc.named_parameters()})
    return out


@pytest.mark.parametrize("layers,ffn,kc,macaron", [(2, 96, 0, False), (2, 96, 5, True), (1, 0, 0, False)])
def test_initial_values_follow_the_documented_draw_order(sed, layers, ffn, kc, macaron):
    torch.manual_seed(11)
    m = sed.Csa_AvgPooling(3, CFG, precision="fp32", sa_heads=2, sa_layers=layers, sa_ffn=ffn, sa_conv_kernel=kc, sa_norm_first=True,
                           sa_macaron=macaron)
    want = replay(sed, 11, 3, 2, layers, ffn, kc, macaron)
    got = dict(m.named_parameters())
    assert set(want) == {n for n in got if "norm" not in n}
    for n, p in want.items():
        assert torch.equal(p, got[n]), n
    for n, p in got.items():
        if "norm" in n:
            assert bool((p == (1.0 if n.endswith("weight") else 0.0)).all()), n


def test_a_default_model_draws_what_it_drew(sed):
    """both switches False: the same keys and, bit for bit, the same initial values as a model built without the arguments"""
    kw = dict(precision="fp32", sa_heads=2, sa_layers=2, sa_ffn=96, sa_conv_kernel=3)
    torch.manual_seed(5)
    a = sed.Csa_AvgPooling(3, CFG, **kw)
    torch.manual_seed(5)
    b = sed.Csa_AvgPooling(3, CFG, sa_norm_first=False, sa_macaron=False, **kw)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and "block_config" not in sa
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert a.sa_config.keywords() == b.sa_config.keywords() and "sa_norm_first" not in a.sa_config.keywords()


def test_refusals_before_any_draw(sed):
    for kw, pat in ((dict(sa_macaron=True, sa_ffn=96), "sa_norm_first"), (dict(sa_macaron=True, sa_norm_first=True), "sa_ffn")):
        torch.manual_seed(1)
        before = torch.get_rng_state()
        with pytest.raises(ValueError, match=pat):
            sed.Csa_AvgPooling(3, CFG, sa_heads=2, **kw)
        assert torch.equal(before, torch.get_rng_state())
        with pytest.raises(ValueError, match=pat):
            sed.CnnEngine(3, CFG, head="sa", sa_heads=2, **kw)
        with pytest.raises(ValueError, match=pat):
            sed.heads.SaConfig(64, 2, **{k[3:]: v for k, v in kw.items()})
    for kw in (dict(sa_norm_first=True), dict(sa_macaron=True)):
        for head in ("fc", "gru", "none"):
            with pytest.raises(ValueError, match="head='sa'"):
                sed.CnnEngine(3, CFG, head=head, **kw)


def test_command_line_flags(sed):
    main = importlib.import_module(PKG + ".main")
    full = main.build_full_parser()
    base = ["--train_features", "Spectogram", "--dataset_name", "synthetic"]
    args = full.parse_args(base + ["--self_attention", "--sa_ffn", "64", "--sa_norm_first", "--sa_macaron"])
    assert (args.sa_norm_first, args.sa_macaron) == (True, True)
    main.validate_args(args)
    off = full.parse_args(base)
    assert (off.sa_norm_first, off.sa_macaron) == (False, False)
    main.validate_args(off)
    for argv in (["--sa_norm_first"], ["--sa_macaron"]):
        with pytest.raises(ValueError, match="--self_attention"):
            main.validate_args(full.parse_args(base + argv))
    with pytest.raises(ValueError, match="sa_norm_first"):
        main.validate_args(full.parse_args(base + ["--self_attention", "--sa_ffn", "64", "--sa_macaron"]))
    with pytest.raises(ValueError, match="sa_ffn"):
        main.validate_args(full.parse_args(base + ["--self_attention", "--sa_norm_first", "--sa_macaron"]))
