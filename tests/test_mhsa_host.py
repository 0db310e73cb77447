"""Host (no GPU): the float64 definition of the self-attention head (tests/mhsa_formula.py) against torch.nn.MultiheadAttention +
torch.nn.LayerNorm with autograd, the gates of that file against plain fp32 / bf16-operand implementations and against mutants of
the definition, and Csa_AvgPooling's parameters, state_dict, FlatParams order and refusals.  The raw_dctx gates (a dctx that is not
bf16-representable) pass the plain implementation that rounds dctx where it is an operand and still reject the backward mutants
more than 10 gates out; the teacher-forced options (lse=, ctx=, stats=) reproduce the default path bit for bit on the definition's
own values and pass the plain implementation on values perturbed within the forward gates."""
import importlib

import numpy as np
import pytest
import torch

import mhsa_formula as F

PKG = "soundeventdetection-pytorch_amd"
CORE_OUT = ("ctx", "lse", "dq", "dk", "dv")


@pytest.fixture(scope="module")
def sed():
    return importlib.import_module(PKG)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


def head_weights(rng, C):
    return {"in_proj_weight": rng.normal(0, 0.3, (3 * C, C)), "in_proj_bias": rng.normal(0, 0.1, 3 * C),
            "out_proj.weight": rng.normal(0, 0.3, (C, C)), "out_proj.bias": rng.normal(0, 0.1, C),
            "norm.weight": rng.normal(1, 0.2, C), "norm.bias": rng.normal(0, 0.2, C)}


def torch_head(x, W, B, t, H, pos_encoding, dh_out):
    """the oracle: torch modules in float64 with autograd -> (h, dx, parameter gradients)"""
    C = x.shape[1]
    mha = torch.nn.MultiheadAttention(C, H, batch_first=True).double()
    ln = torch.nn.LayerNorm(C).double()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.from_numpy(W["in_proj_weight"]))
        mha.in_proj_bias.copy_(torch.from_numpy(W["in_proj_bias"]))
        mha.out_proj.weight.copy_(torch.from_numpy(W["out_proj.weight"]))
        mha.out_proj.bias.copy_(torch.from_numpy(W["out_proj.bias"]))
        ln.weight.copy_(torch.from_numpy(W["norm.weight"]))
        ln.bias.copy_(torch.from_numpy(W["norm.bias"]))
    xt = torch.from_numpy(x).view(B, t, C).clone().requires_grad_(True)
    xp = xt + torch.from_numpy(F.positional_table(t, C)) if pos_encoding else xt
    a, _ = mha(xp, xp, xp, need_weights=False)
    h = ln(xp + a)
    h.backward(torch.from_numpy(dh_out).view(B, t, C))
    g = {"d_in_proj_weight": mha.in_proj_weight.grad, "d_in_proj_bias": mha.in_proj_bias.grad, "d_out_proj.weight": mha.out_proj.weight.grad,
         "d_out_proj.bias": mha.out_proj.bias.grad, "d_norm.weight": ln.weight.grad, "d_norm.bias": ln.bias.grad}
    return h.detach().numpy().reshape(B * t, C), xt.grad.numpy().reshape(B * t, C), {n: v.numpy() for n, v in g.items()}


@pytest.mark.parametrize("geom", [(2, 7, 1, 32), (3, 5, 4, 32), (2, 9, 2, 64)], ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("pos", [True, False])
def test_definition_against_torch_modules(geom, pos):
    B, t, H, dh = geom
    C = H * dh
    rng = np.random.default_rng(B + 10 * t + H)
    x, dh_out, W = rng.normal(0, 1, (B * t, C)), rng.normal(0, 1, (B * t, C)), head_weights(rng, C)
    ref = F.head(x, W, B, t, H, pos, dh_out=dh_out)
    h, dx, g = torch_head(x, W, B, t, H, pos, dh_out)
    assert rel(ref["h"], h) < 1e-12 and rel(ref["dx"], dx) < 1e-12
    for n, v in g.items():
        assert rel(ref[n], v) < 1e-12, n
    # the mutant of the whole head: the residual branch missing from the gradient of x'
    assert rel(F.head(x, W, B, t, H, pos, dh_out=dh_out, mutant="no_residual")["dx"], dx) > 1e-3


def test_core_vectorised_against_loops_and_torch_sdpa():
    rng = np.random.default_rng(5)
    q, k, v, d = (rng.normal(0, 1, (2, 6, 2, 32)) for _ in range(4))
    a, b = F.core(q, k, v, d), F.core_loops(q, k, v, d)
    for n in CORE_OUT:
        assert rel(a[n], b[n]) < 1e-13, n
    tq, tk, tv = (torch.from_numpy(u).permute(0, 2, 1, 3).clone().requires_grad_(True) for u in (q, k, v))
    o = torch.nn.functional.scaled_dot_product_attention(tq, tk, tv)
    o.backward(torch.from_numpy(d).permute(0, 2, 1, 3))
    assert rel(a["ctx"], o.detach().permute(0, 2, 1, 3).numpy()) < 1e-12
    for n, u in (("dq", tq), ("dk", tk), ("dv", tv)):
        assert rel(a[n], u.grad.permute(0, 2, 1, 3).numpy()) < 1e-12, n
    pe = F.positional_table(5, 8)
    assert pe[0].tolist() == [0.0, 1.0] * 4 and pe[3, 2] == np.sin(3 / 10000 ** (2 / 8)) and pe[3, 5] == np.cos(3 / 10000 ** (4 / 8))


def cases(mode):
    rng = np.random.default_rng(11)
    out = []
    for (B, t, H, dh) in [(2, 5, 1, 32), (2, 33, 4, 32), (2, 65, 2, 64), (2, 130, 1, 32)]:
        arrs = [rng.normal(0, s, (B, t, H, dh)).astype(np.float32) for s in (1.0, 1.0, 1.0, 0.1)]
        out.append([F.round_bf16(a) if mode == "bf16" else a for a in arrs])
    return out


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_core_gates_pass_a_plain_implementation(mode):
    """a plain fp32 numpy implementation of the same formulas (bf16: with P and dS rounded to bf16 where they are operands)"""
    for q, k, v, d in cases(mode):
        ref, gates = F.core(q, k, v, d), F.core_gates(q, k, v, d, mode)
        got = F.core(q, k, v, d, dtype=np.float32, bf16_operands=mode == "bf16")
        for n in CORE_OUT:
            good, worst = F.check(got[n], ref[n], gates[n], (mode, q.shape, n))
            assert good, (mode, q.shape, n, worst)
        if mode == "bf16":          # and the bf16 gate is not so wide that it lets the fp32 one's mutants through (below), nor so
            plain = F.core(q, k, v, d, dtype=np.float32)        # narrow that it refuses fp32 arithmetic
            assert all(F.check(plain[n], ref[n], gates[n], n)[0] for n in CORE_OUT)


MUTANTS = {"no_scale": ("ctx", "lse"), "softmax_over_queries": ("ctx", "lse"), "drop_last_key": ("ctx",), "neighbour_clip": ("ctx",),
           "swap_heads_v": ("ctx",), "no_D": ("dq", "dk"), "dk_no_scale": ("dk",)}


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_core_gates_reject_mutants(mutant, mode):
    for q, k, v, d in cases(mode)[1:3]:         # H > 1, two different clips
        ref, gates = F.core(q, k, v, d), F.core_gates(q, k, v, d, mode)
        backward = MUTANTS[mutant][0] not in ("ctx", "lse")
        got = F.core(q, k, v, d if backward else None, mutant=mutant)
        for n in MUTANTS[mutant]:
            good, worst = F.check(got[n], ref[n], gates[n], (mutant, mode, n))
            assert not good and worst > 10.0, (mutant, mode, n, worst)


def raw_dctx_cases():
    """cases("bf16") with a dctx that is NOT bf16-representable (what the engine's out_proj GEMM hands the kernel)"""
    rng = np.random.default_rng(12)
    out = []
    for q, k, v, d in cases("bf16"):
        raw = rng.normal(0, 0.1, d.shape).astype(np.float32)
        assert (F.round_bf16(raw) != raw).mean() > 0.9
        out.append((q, k, v, raw))
    return out


def test_raw_dctx_gates_pass_a_plain_implementation():
    """plain fp32 arithmetic with P, dS and -- where it is an operand, not in D -- dctx rounded to bf16, against float64 on the raw dctx"""
    for q, k, v, d in raw_dctx_cases():
        ref, gates = F.core(q, k, v, d), F.core_gates(q, k, v, d, "bf16", raw_dctx=True)
        tight = F.core_gates(q, k, v, d, "bf16")
        got = F.core(q, k, v, d, dtype=np.float32, bf16_operands=True, round_dctx=True)
        for n in CORE_OUT:
            good, worst = F.check(got[n], ref[n], gates[n], ("raw dctx", q.shape, n))
            assert good, (q.shape, n, worst)
            assert (gates[n] >= tight[n]).all() and (gates[n] <= 1.5 * tight[n] + 1e-300).all(), n     # 2^-9 next to 2^-8: at most half as much again
        for n in ("ctx", "lse"):
            assert np.array_equal(gates[n], tight[n]), n
        # f32 mode has no operand rounding: the flag changes nothing there, and the default is today's gate
        f32 = F.core_gates(q, k, v, d, "f32")
        assert all(np.array_equal(F.core_gates(q, k, v, d, "f32", raw_dctx=True)[n], f32[n]) for n in CORE_OUT)
        # rounding dctx in D as well is NOT what the kernel does; the flag of core() leaves D alone
        plain = F.core(q, k, v, d, dtype=np.float32, bf16_operands=True)
        assert not np.array_equal(plain["dv"], got["dv"]) and np.array_equal(plain["ctx"], got["ctx"])


@pytest.mark.parametrize("mutant", sorted(m for m, outs in MUTANTS.items() if outs[0] not in ("ctx", "lse")))
def test_raw_dctx_gates_reject_the_backward_mutants(mutant):
    for q, k, v, d in raw_dctx_cases()[1:3]:
        ref, gates = F.core(q, k, v, d), F.core_gates(q, k, v, d, "bf16", raw_dctx=True)
        got = F.core(q, k, v, d, mutant=mutant)
        for n in MUTANTS[mutant]:
            good, worst = F.check(got[n], ref[n], gates[n], (mutant, "raw dctx", n))
            assert not good and worst > 10.0, (mutant, n, worst)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_teacher_forced_core(mode):
    """lse= / ctx=: the definition's own values reproduce the default path bit for bit; values perturbed within the forward gates
    (what a kernel's forward may hand its backward) give a reference that the plain implementation fed the same values still meets"""
    rng = np.random.default_rng(13)
    for q, k, v, d in cases(mode):
        ref, gates = F.core(q, k, v, d), F.core_gates(q, k, v, d, mode)
        same, gsame = F.core(q, k, v, d, lse=ref["lse"], ctx=ref["ctx"]), F.core_gates(q, k, v, d, mode, lse=ref["lse"], ctx=ref["ctx"])
        for n in CORE_OUT:
            assert np.array_equal(same[n], ref[n]) and np.array_equal(gsame[n], gates[n]), n
        lse = (ref["lse"] + gates["lse"] * rng.uniform(-1, 1, ref["lse"].shape)).astype(np.float32)
        ctx = (ref["ctx"] + gates["ctx"] * rng.uniform(-1, 1, ref["ctx"].shape)).astype(np.float32)
        assert not np.array_equal(lse, ref["lse"].astype(np.float32)) and not np.array_equal(ctx, ref["ctx"].astype(np.float32))
        tf, gtf = F.core(q, k, v, d, lse=lse, ctx=ctx), F.core_gates(q, k, v, d, mode, lse=lse, ctx=ctx)
        assert np.allclose(tf["p_bwd"], np.exp(tf["s"] - lse.astype(np.float64)[..., None]), rtol=1e-12, atol=0)
        assert np.array_equal(tf["ctx"], ref["ctx"]) and np.array_equal(tf["lse"], ref["lse"])          # the forward half is not forced
        got = F.core(q, k, v, d, dtype=np.float32, bf16_operands=mode == "bf16", lse=lse, ctx=ctx)
        for n in ("dq", "dk", "dv"):
            good, worst = F.check(got[n], tf[n], gtf[n], (mode, "teacher-forced", q.shape, n))
            assert good, (mode, q.shape, n, worst)
        # the forced values matter: a ctx off by far more than its gate moves dq (through D) out of the gate
        far = F.core(q, k, v, d, lse=lse, ctx=ctx + 0.05)
        assert not F.check(far["dq"], tf["dq"], gtf["dq"], (mode, "ctx far off, dq"))[0]


def ln_case(rows, C, seed=0):
    rng = np.random.default_rng(seed + rows + C)
    return (rng.normal(0.3, 1.0, (rows, C)).astype(np.float32), rng.normal(-0.1, 0.5, (rows, C)).astype(np.float32),
            rng.normal(1.0, 0.3, C).astype(np.float32), rng.normal(0.0, 0.3, C).astype(np.float32),
            rng.normal(0.0, 0.1, (rows, C)).astype(np.float32))


@pytest.mark.parametrize("C", [32, 128, 512])
def test_layernorm_gates(C):
    x, a, gamma, beta, dy = ln_case(65, C)
    ref, gates = F.add_layernorm(x, a, gamma, beta, dy), F.add_layernorm_gates(x, a, gamma, beta, dy)
    t = torch.from_numpy((x.astype(np.float64) + a)).requires_grad_(True)
    ln = torch.nn.LayerNorm(C).double()
    with torch.no_grad():
        ln.weight.copy_(torch.from_numpy(gamma.astype(np.float64)))
        ln.bias.copy_(torch.from_numpy(beta.astype(np.float64)))
    y = ln(t)
    y.backward(torch.from_numpy(dy.astype(np.float64)))
    assert rel(ref["y"], y.detach().numpy()) < 1e-12 and rel(ref["dres"], t.grad.numpy()) < 1e-12
    assert rel(ref["dgamma"], ln.weight.grad.numpy()) < 1e-12 and rel(ref["dbeta"], ln.bias.grad.numpy()) < 1e-12
    got = F.add_layernorm(x, a, gamma, beta, dy, dtype=np.float32)
    for n in ("y", "dres", "dgamma", "dbeta"):
        good, worst = F.check(got[n], ref[n], gates[n], (C, n))
        assert good, (C, n, worst)
    bad = F.add_layernorm(x, a, gamma, beta, dy, mutant="unbiased_variance")
    for n in ("y", "dres", "dgamma"):
        good, worst = F.check(bad[n], ref[n], gates[n], (C, "unbiased", n))
        assert not good and worst > 10.0, (C, n, worst)
    # the residual missing: LayerNorm of a alone (forward) / the gradient of the normalised branch without x
    alone = F.add_layernorm(np.zeros_like(x), a, gamma, beta, dy)
    assert not F.check(alone["y"], ref["y"], gates["y"], (C, "no residual"))[0]
    assert not F.check(alone["dres"], ref["dres"], gates["dres"], (C, "no residual, dres"))[0]


@pytest.mark.parametrize("C", [32, 128])
def test_teacher_forced_layernorm(C):
    """stats=: the definition's own (mean, rstd) reproduce the default path bit for bit; statistics perturbed within the forward's
    gates on them (tests/test_gpu_mhsa.py) give a reference the plain fp32 implementation fed the same statistics still meets"""
    x, a, gamma, beta, dy = ln_case(65, C, seed=1)
    ref, gates = F.add_layernorm(x, a, gamma, beta, dy), F.add_layernorm_gates(x, a, gamma, beta, dy)
    own = np.stack([ref["mean"], ref["rstd"]], axis=1)
    same, gsame = F.add_layernorm(x, a, gamma, beta, dy, stats=own), F.add_layernorm_gates(x, a, gamma, beta, dy, stats=own)
    for n in ("y", "dres", "dgamma", "dbeta"):
        assert np.array_equal(same[n], ref[n]) and np.array_equal(gsame[n], gates[n]), n
    rng = np.random.default_rng(C)
    z = ref["z"]
    M = np.abs(z).mean(axis=1)
    d = np.abs(z - ref["mean"][:, None])
    k = (C + 8) * F.U
    g_mean, g_rstd = k * M, k * ref["rstd"] * (1.0 + ref["rstd"] ** 2 * (d * (np.abs(z) + M[:, None])).mean(axis=1))
    stats = np.stack([ref["mean"] + g_mean * rng.uniform(-1, 1, M.shape), ref["rstd"] + g_rstd * rng.uniform(-1, 1, M.shape)], axis=1).astype(np.float32)
    tf, gtf = F.add_layernorm(x, a, gamma, beta, dy, stats=stats), F.add_layernorm_gates(x, a, gamma, beta, dy, stats=stats)
    assert np.array_equal(tf["y"], ref["y"]) and np.array_equal(gtf["y"], gates["y"]) and not np.array_equal(tf["dres"], ref["dres"])
    got = F.add_layernorm(x, a, gamma, beta, dy, dtype=np.float32, stats=stats)
    for n in ("dres", "dgamma", "dbeta"):
        good, worst = F.check(got[n], tf[n], gtf[n], (C, "teacher-forced", n))
        assert good, (C, n, worst)
    # the forced statistics matter: an rstd off by 1e-3 relative moves dres out of the gate
    far = F.add_layernorm(x, a, gamma, beta, dy, stats=stats * np.array([1.0, 1.001]))
    assert not F.check(far["dres"], tf["dres"], gtf["dres"], (C, "rstd far off, dres"))[0]


# ---- the model ---------------------------------------------------------------------------------------------------------------------
CFG = [(32, 2), (64, 2)]


def test_state_dict_loads_into_the_torch_modules(sed):
    torch.manual_seed(0)
    m = sed.Csa_AvgPooling(3, CFG, precision="fp32", sa_heads=2, mel_bins=8)
    sd = m.state_dict()
    C = 64
    shapes = {"attn.in_proj_weight": (3 * C, C), "attn.in_proj_bias": (3 * C,), "attn.out_proj.weight": (C, C), "attn.out_proj.bias": (C,),
              "attn_norm.weight": (C,), "attn_norm.bias": (C,), "attn_config": (2,), "event_fc.weight": (3, C), "event_fc.bias": (3,)}
    for n, shp in shapes.items():
        assert tuple(sd[n].shape) == shp, n
    assert sd["attn_config"].dtype == torch.float64 and sd["attn_config"].tolist() == [2.0, 1.0]
    assert not [n for n in sd if n.startswith("pe") or ".pe" in n], "the positional table is not part of the state_dict"
    mha, ln = torch.nn.MultiheadAttention(C, 2, batch_first=True), torch.nn.LayerNorm(C)
    mha.load_state_dict({n[len("attn."):]: v for n, v in sd.items() if n.startswith("attn.")})
    ln.load_state_dict({n[len("attn_norm."):]: v for n, v in sd.items() if n.startswith("attn_norm.")})
    # initialised like torch: zero biases, unit norm, and the same random draws in the same order as the module's constructor
    assert not sd["attn.in_proj_bias"].any() and not sd["attn.out_proj.bias"].any()
    assert bool((sd["attn_norm.weight"] == 1).all()) and not sd["attn_norm.bias"].any()
    torch.manual_seed(3)
    ours = sed.models.spectogram_models._MhaParams(C, 2)
    torch.manual_seed(3)
    theirs = torch.nn.MultiheadAttention(C, 2, batch_first=True)
    assert torch.equal(ours.in_proj_weight, theirs.in_proj_weight) and torch.equal(ours.out_proj.weight, theirs.out_proj.weight)
    # rebuildable from the state_dict alone
    assert sed.Csa_AvgPooling.config_from_state_dict(sd) == (2, True)
    twin = sed.Csa_AvgPooling(3, CFG, precision="fp32", sa_heads=2, pos_encoding=True, mel_bins=8)
    twin.load_state_dict(sd)
    assert sed.Csa_AvgPooling.config_from_state_dict(sed.Csa_AvgPooling(3, CFG, sa_heads=1, pos_encoding=False).state_dict()) == (1, False)


def test_other_models_draw_and_hold_what_they_did(sed):
    torch.manual_seed(1)
    a = sed.Cnn_AvgPooling(3, CFG, precision="fp32")
    torch.manual_seed(1)
    b = sed.Csa_AvgPooling(3, CFG, precision="fp32", sa_heads=1)
    for n, v in a.state_dict().items():
        if n.startswith("conv_blocks."):
            assert torch.equal(v, b.state_dict()[n]), n
    assert not [n for n in a.state_dict() if n.startswith("attn")]
    assert not [n for n in sed.Crnn_AvgPooling(3, CFG, precision="fp32", gru_hidden=32).state_dict() if n.startswith("attn")]
    twin = b.clone_without_engines()
    assert isinstance(twin, sed.Csa_AvgPooling) and twin.engine is not b.engine and twin.engine.head == "sa"
    assert twin.sa_heads == 1 and twin.engine.sa_heads == 1 and twin.engine.pos_encoding
    for (n, u), (_, w) in zip(b.state_dict().items(), twin.state_dict().items()):
        assert torch.equal(u, w) and (u.data_ptr() != w.data_ptr() or u.numel() == 0), n


def test_flat_params_group_order(sed):
    """backward completion order: (att_fc,) event_fc, attn_norm, attn, then the blocks from the last to the first"""
    for attention in (False, True):
        m = sed.Csa_AvgPooling(3, CFG, precision="fp32", sa_heads=2, attention=attention)
        flat = sed.train.FlatParams(m, n_buckets=0)
        keys = [k for k, _, _ in flat.groups]
        assert keys == (["att_fc"] if attention else []) + ["event_fc", "attn_norm", "attn", "conv_blocks.1", "conv_blocks.0"]
        names = [n for n, _ in m.named_parameters()]
        assert names.index("attn.in_proj_weight") > names.index("conv_blocks.1.bn2.bias") and \
            names.index("attn_norm.bias") < names.index("event_fc.weight")


def test_constructor_refusals(sed):
    with pytest.raises(ValueError, match="divide"):
        sed.Csa_AvgPooling(3, [(32, 2), (96, 2)], sa_heads=5)
    with pytest.raises(ValueError, match="head width"):
        sed.Csa_AvgPooling(3, [(32, 2), (128, 2)], sa_heads=1)           # dh = 128
    with pytest.raises(ValueError, match="head width"):
        sed.Csa_AvgPooling(3, [(32, 2), (64, 2)], sa_heads=4)            # dh = 16
    with pytest.raises(ValueError, match="multiple of 4"):
        sed.Csa_AvgPooling(3, [(32, 2), (66, 2)], sa_heads=2)
    with pytest.raises(ValueError, match="sa_heads"):
        sed.Csa_AvgPooling(3, CFG, sa_heads=0)
    with pytest.raises(ValueError):
        sed.CnnEngine(3, CFG, head="sa", sa_heads=4)
    assert sed.Csa_AvgPooling(3, [(32, 2), (128, 1)], sa_heads=4).engine.head == "sa"


def test_main_flags(sed):
    main = importlib.import_module(PKG + ".main")
    weak = main.build_weak_parser()
    args = weak.parse_args(["--self_attention", "--sa_heads", "2", "--no_pos_encoding"])
    assert args.self_attention and args.sa_heads == 2 and args.no_pos_encoding
    off = weak.parse_args([])
    assert not off.self_attention and off.sa_heads == 4 and not off.no_pos_encoding
    full = main.build_full_parser()
    assert not hasattr(main.build_parser().parse_args([]), "self_attention")
    main.validate_args(full.parse_args([]))
    base = ["--train_features", "Spectogram", "--dataset_name", "synthetic"]
    main.validate_args(full.parse_args(base + ["--self_attention"]))
    main.validate_args(full.parse_args(base + ["--self_attention", "--sa_heads", "2", "--no_pos_encoding", "--attention_head",
                                               "--weak_labels", "only", "--weak_pooling", "att"]))
    with pytest.raises(ValueError, match="Spectogram"):
        main.validate_args(full.parse_args(["--train_features", "Waveform", "--self_attention"]))
    with pytest.raises(ValueError, match="head width"):
        main.validate_args(full.parse_args(base + ["--self_attention", "--sa_heads", "8"]))
    with pytest.raises(ValueError, match="divide"):
        main.validate_args(full.parse_args(base + ["--self_attention", "--sa_heads", "3"]))
    for argv in (["--sa_heads", "2"], ["--no_pos_encoding"]):
        with pytest.raises(ValueError, match="--self_attention"):
            main.validate_args(full.parse_args(base + argv))
