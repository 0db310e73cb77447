"""GPU: Csa_AvgPooling(sa_window=) through the model, the engine, FusedTrainer and infer.py, on the tiny configuration of
tests/test_gpu_sa_model.py / test_gpu_sa_conformer.py (t = 10 frames per clip), and once at C = 128, t = 130, R = 520
(tests/test_gpu_sa_at_size.py's shape).

fp32 parity is against torch in float64 with src_mask / attn_mask = M, M[i][j] = True where j < i - left or j > i + right
(tests/test_gpu_sa_conformer.py's oracle with the mask handed to every layer's self_attn), fed by a head='none' engine on the same
parameters, whose backward takes the oracle's feature gradient.  Bounds, tests/test_gpu_crnn.py's: logits 1e-3 absolute, loss 1e-4, every
parameter gradient 3e-3 relative L2 (depthwise.bias by tests/test_gpu_sa_conformer.py's rule).  At size the two windowed launches are
checked per element against the float64 definition of tests/window_formula.py on the engine's own qkv, ctx, lse and dctx, inside that
file's gates (raw dctx terms in bf16).
Measured on the MI355X (-s): tiny fp32 logits off by at most 9.8e-7, worst gradient 1.5e-6 relative L2 (convm_l1.pointwise1.bias), the
unmasked oracle 0.27 -- 0.52 away; at size sed_mhsa_fwd_win 0.036 (fp32) / 0.49 (bf16) of its gate, sed_mhsa_bwd_win 0.043 / 0.55."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import convmod_formula as V
import ffn_formula as F
import mhsa_formula as M
import test_gpu_sa_conformer as T1
import test_gpu_sa_model as T0
import window_formula as WF

pytestmark = pytest.mark.gpu
PKG = "soundeventdetection-pytorch_amd"
CFG, MEL, W = T0.CFG, T0.MEL, T0.W
C, D = CFG[-1][0], 64
rel_l2, batch, the_plan = T0.rel_l2, T0.batch, T0.the_plan


@pytest.fixture(scope="module")
def sed():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)


def make_model(sed, window, K=3, precision="fp32", layers=2, ffn=D, k=7, **kw):
    return T1.make_model(sed, K, precision, layers=layers, ffn=ffn, k=k, sa_window=window, **kw)


def oracle(sed, sd, feat, y, window, heads, layers, ffn, k, ratio, training=True):
    """tests/test_gpu_sa_conformer.py's oracle (TransformerEncoderLayer pieces per layer, or MultiheadAttention + LayerNorm without an
    FFN; its ConvModule with k > 0) with the window as torch's boolean mask.  -> logits, loss, gradients by state_dict name"""
    Cc, t = feat.shape[-1], feat.shape[1]
    mask = None if window is None else torch.from_numpy(WF.torch_mask(t, *window))
    cpu = lambda d: {n: (v.double() if v.is_floating_point() else v).cpu() for n, v in d.items()}
    enc, conv = [], []
    for l in range(layers):
        an, nn_ = F.layer_names(l)[:2]
        if ffn:
            e = torch.nn.TransformerEncoderLayer(Cc, heads, ffn, dropout=0.0, activation="gelu", batch_first=True, norm_first=False).double()
            e.load_state_dict(cpu(sed.Csa_AvgPooling.encoder_layer_state(sd, l)), strict=False)
        else:
            e = torch.nn.Module()
            e.self_attn, e.norm1 = torch.nn.MultiheadAttention(Cc, heads, batch_first=True), torch.nn.LayerNorm(Cc)
            e.double()
            for mod, name in ((e.self_attn, an), (e.norm1, nn_)):
                mod.load_state_dict(cpu({n[len(name) + 1:]: v for n, v in sd.items() if n.startswith(name + ".")}))
        enc.append(e.train(training))
        if k:
            c = T1.ConvModule(Cc, k).double()
            c.load_state_dict(cpu(sed.Csa_AvgPooling.conv_module_state(sd, l)))
            conv.append(c.train(training))
    fc = torch.nn.Linear(Cc, sd["event_fc.weight"].shape[0]).double()
    fc.load_state_dict({n[len("event_fc."):]: v.double().cpu() for n, v in sd.items() if n.startswith("event_fc.")})
    m = feat.mean(dim=2)
    h = m + torch.from_numpy(M.positional_table(t, Cc)).float().double()      # the table as rounded to fp32
    for l, e in enumerate(enc):
        h = e.norm1(h + e.self_attn(h, h, h, attn_mask=mask, need_weights=False)[0])
        if k:
            h = conv[l](h)
        if ffn:
            h = e.norm2(h + e.linear2(TF.gelu(e.linear1(h))))
    out = fc(h).repeat_interleave(ratio, dim=1)
    N = min(out.shape[1], y.shape[1])
    loss = TF.binary_cross_entropy_with_logits(out[:, :N], y[:, :N], pos_weight=torch.tensor(W, dtype=torch.float64))
    loss.backward()
    grads = {}
    for l, e in enumerate(enc):
        an, nn_, fn, fnn = F.layer_names(l)
        back = {"self_attn": an, "norm1": nn_, "linear1": fn + ".linear1", "linear2": fn + ".linear2", "norm2": fnn}
        for n, p in e.named_parameters():
            top, rest = n.split(".", 1)
            grads[back[top] + "." + rest] = p.grad
        if k:
            cm, cn = V.conv_names(l)
            for n, p in conv[l].named_parameters():
                grads[(cn + n[len("conv_norm"):]) if n.startswith("conv_norm") else cm + "." + n] = p.grad
    grads.update({"event_fc." + n: p.grad for n, p in fc.named_parameters()})
    return out.detach(), loss.detach(), grads


def compare(sed, model, x, y, window, layers, ffn, k, training, tag):
    K = y.shape[-1]
    sd0 = {n: v.clone() for n, v in model.state_dict().items()}
    model.train(training)
    model.zero_grad()
    out = model(x)
    loss = sed.WeightedBCE(W, True)(out, y)
    loss.backward()
    plan = the_plan(model)
    bare = sed.CnnEngine(K, CFG, 1, "fp32", head="none", mel_bins=MEL)
    P0 = {n: v.cuda() for n, v in sd0.items()}
    bp = bare.forward(x, P0, training=training, update_running_stats=False, keep_for_grad=not training)
    assert torch.equal(bp.y[-1], plan.y[-1])
    feat = bp.y[-1][..., :C].double().cpu().requires_grad_(True)
    out_t, loss_t, grads = oracle(sed, sd0, feat, y.double().cpu(), window, 1, layers, ffn, k, model.engine.ratio, training)
    err = float((out.detach().cpu().double() - out_t).abs().max())
    print(f"{tag}: logits max error {err:.3e}, loss error {abs(loss.item() - float(loss_t)):.3e}")
    assert err < 1e-3 and abs(loss.item() - float(loss_t)) < 1e-4
    mine = {n for n, _ in model.named_parameters() if not n.startswith("conv_blocks.")}
    assert mine == set(grads), mine ^ set(grads)
    for n, g in grads.items():
        got = model.get_parameter(n).grad
        if training and n.endswith("depthwise.bias"):
            scale = float(grads[n.replace(".bias", ".weight")].norm())
            assert float(got.norm()) < 3e-3 * scale and float(g.norm()) < 3e-3 * scale, n
            continue
        l2 = rel_l2(got, g)
        print(f"  {n}: relative L2 {l2:.3e}")
        assert l2 < 3e-3, (n, l2)
    # the oracle's feature gradient back through the pinned conv backward
    bp.dy[-1].zero_()
    bp.dy[-1][..., :C] = feat.grad.float().cuda()
    names = [n for n, _ in model.named_parameters() if n.startswith("conv_blocks.")]
    G = {n: torch.full_like(P0[n], float("nan")) for n in names}
    bare.backward(bp, P0, G)
    for n in names:
        assert rel_l2(model.get_parameter(n).grad, G[n]) < 3e-3, n
    # the oracle without the mask is somewhere else: the bound sees the window
    plain = oracle(sed, sd0, feat.detach().clone().requires_grad_(True), y.double().cpu(), None, 1, layers, ffn, k, model.engine.ratio, training)[0]
    seen = float((out.detach().cpu().double() - plain).abs().max())
    print(f"{tag}: the unmasked oracle's logits are {seen:.3e} away")
    assert seen > 2e-3


def test_fp32_two_layer_model_matches_torch_with_src_mask(sed):
    x, y = batch()
    model = make_model(sed, (4, 2))
    assert model.engine.sa_window == (4, 2) and model.window_config.tolist() == [4.0, 2.0]
    compare(sed, model, x, y, (4, 2), 2, D, 7, True, "2 layers, gelu FFN, k = 7, window (4, 2)")


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_fp32_causal_model_matches_torch_with_src_mask(sed, training):
    x, y = batch()
    model = make_model(sed, (3, 0), layers=1, ffn=0, k=0)
    compare(sed, model, x, y, (3, 0), 1, 0, 0, training, f"1 layer, causal (3, 0), training={training}")


@pytest.mark.parametrize("precision", ["bf16", "f16x3", "bf16x3"])
def test_other_precisions_follow_fp32(sed, precision):
    """tests/test_gpu_sa_conformer.py's bounds for the same stack: the window changes which keys enter a softmax, not how many
    roundings lie between the input and a gradient"""
    x, y = batch()
    ref, model = make_model(sed, (4, 2)).train(), make_model(sed, (4, 2), precision=precision).train()
    lr = sed.WeightedBCE(W, True)(ref(x), y)
    lm = sed.WeightedBCE(W, True)(model(x), y)
    lr.backward()
    lm.backward()
    print(f"{precision}: loss difference {abs(lr.item() - lm.item()):.3e}")
    assert abs(lr.item() - lm.item()) < (6e-2 if precision == "bf16" else 6e-3)
    for (n, p), (_, q) in zip(ref.named_parameters(), model.named_parameters()):
        assert bool(torch.isfinite(q.grad).all()), n
        if n.startswith(("attn", "ffn", "event_fc", "convm", "conv_norm")) and not n.endswith("depthwise.bias"):
            assert rel_l2(q.grad, p.grad) < (0.3 if precision == "bf16" else 4e-2), (precision, n, rel_l2(q.grad, p.grad))


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_graph_steps_give_the_eager_bits(sed, p):
    x, y = batch()

    def fresh():
        return sed.FusedTrainer(make_model(sed, (4, 2), precision="bf16", sa_dropout=p, sa_dropout_seed=7), lr=1e-3, recall_factor=W, graph=True)

    eager, graph = fresh(), fresh()
    for i in range(4):              # launch by launch / two eager steps, the capture, a replay
        le = eager._step_dev(x, y).clone()
        eager._host_mirror()
        lg = graph.train_step(x, y).clone()
        assert torch.equal(le, lg), (i, "the graph step's loss differs from the eager step's")
        assert torch.equal(eager.flat.p, graph.flat.p), i
    assert len(graph._graphs) == 1 and len(eager._graphs) == 0


def test_options_take_a_step(sed):
    x, y = batch()
    tr = sed.FusedTrainer(make_model(sed, (4, 2), attention=True), lr=1e-3, recall_factor=W, weak_pooling="att", weak_only=True)
    for v in tr.flat.G.values():
        v.fill_(float("nan"))
    tr.forward_backward(x, y)
    assert all(bool(torch.isfinite(g).all()) for g in tr.flat.G.values())
    tr.forward_backward(x, y, torch.tensor([1, 2], device="cuda"))          # label kinds
    assert all(bool(torch.isfinite(g).all()) for g in tr.flat.G.values())
    mt = sed.FusedTrainer(make_model(sed, (4, None), sa_dropout=0.1, sa_dropout_seed=5), lr=1e-3, recall_factor=W, mean_teacher=True,
                          consistency_weight=2.0)
    assert mt.teacher.engine is not mt.model.engine and mt.teacher.engine.sa_window == (4, None) == mt.teacher.sa_window
    assert mt.teacher.state_dict()["window_config"].tolist() == [4.0, -1.0]
    for _ in range(2):
        loss = mt.train_step(x, y)
    assert bool(torch.isfinite(loss).all())
    opt = sed.FusedTrainer(make_model(sed, 2), lr=1e-3, recall_factor=W, weight_decay=1e-2, decoupled_weight_decay=True, max_grad_norm=0.5)
    assert bool(torch.isfinite(opt.train_step(x, y)).all())
    fe = sed.PCEN(MEL, trainable=True)
    pt = sed.FusedTrainer(make_model(sed, (0, 3), frontend=fe), lr=1e-3, recall_factor=W)
    pt.train_step(x.abs() + 0.1, y)
    assert all(bool(torch.isfinite(v).all()) for v in pt.flat.G.values())
    # need_dx in training mode and the eval-mode backward
    for training in (True, False):
        model = make_model(sed, (3, 0)).train(training)
        xg = x.clone().requires_grad_(True)
        model(xg).sum().backward()
        assert bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0, training
        assert float(model.attn.in_proj_weight.grad.abs().max()) > 0


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("window", [(9, 9), (None, 40), 1000], ids=str)
def test_a_window_that_covers_the_clip_gives_the_unwindowed_bits(sed, window, precision):
    x, y = batch()
    win, plain = make_model(sed, window, precision=precision, sa_dropout=0.1, sa_dropout_seed=3), \
        make_model(sed, None, precision=precision, sa_dropout=0.1, sa_dropout_seed=3)
    assert [n for n in win.state_dict() if n != "window_config"] == list(plain.state_dict())
    for m in (win, plain):
        m.train()
        sed.WeightedBCE(W, True)(m(x), y).backward()
    assert the_plan(win).t_out == 10
    assert torch.equal(the_plan(win).pre, the_plan(plain).pre)
    for (n, a), (_, b) in zip(win.named_parameters(), plain.named_parameters()):
        assert torch.equal(a.grad, b.grad), n
    win.eval(), plain.eval()
    with torch.no_grad():
        assert torch.equal(win(x), plain(x))


def test_launch_labels(sed):
    """sa_window=None: the list of tests/test_gpu_sa_model.py; a window: the _win entries in the core launches' places, tagged sa"""
    torch.manual_seed(0)
    sa = T0.step_labels(sed, sed.Csa_AvgPooling(3, CFG, precision="bf16", sa_heads=1, sa_window=None).cuda())
    h, b = T0.PLAIN_STEP.index("sed_head_fwd"), T0.PLAIN_STEP.index("sed_head_bwd")
    assert sa == T0.PLAIN_STEP[:h] + T0.SA_FWD + T0.PLAIN_STEP[h + 1:b] + T0.SA_BWD + T0.PLAIN_STEP[b + 1:]
    twin = {"sed_mhsa_fwd": "sed_mhsa_fwd_win", "sed_mhsa_bwd": "sed_mhsa_bwd_win"}
    win = T0.step_labels(sed, sed.Csa_AvgPooling(3, CFG, precision="bf16", sa_heads=1, sa_window=(2, 1)).cuda())
    assert win == [twin.get(l, l) for l in sa]
    drop = T0.step_labels(sed, sed.Csa_AvgPooling(3, CFG, precision="bf16", sa_heads=1, sa_window=(2, 1), sa_dropout=0.1).cuda())
    dtw = {"sed_add_layernorm_fwd": "sed_add_layernorm_fwd_drop", "sed_add_layernorm_bwd": "sed_add_layernorm_bwd_drop"}
    assert drop == [dtw.get(l, l) for l in win]
    x, y = batch()
    model = make_model(sed, (2, 1)).train()
    eng, P = model.engine, model._tensor_dict()
    eng.timer = sed.engine.KernelTimer()
    plan = eng.forward(x, P, training=True)
    eng.loss_and_grad(plan, y, W)
    eng.backward(plan, P, {n: torch.empty_like(p) for n, p in model.named_parameters()})
    torch.cuda.synchronize()
    labels = [lbl for lbl, _, _ in eng.timer.records]
    for name in twin.values():
        assert [l for l in labels if l.split(":")[0] == name] == [name + ":sa"] * 2, name
    assert not [l for l in labels if l.split(":")[0] in twin]


def test_checkpoint_round_trip_through_infer(sed, tmp_path):
    from scipy.io import wavfile
    infer = importlib.import_module(PKG + ".infer")
    sc = importlib.import_module(PKG + ".dataset.spectogram.spectogram_configs")
    rng = np.random.default_rng(4)
    wav = 0.05 * rng.standard_normal(32000 * 2)
    wav[20000:30000] += 0.4 * np.sin(2 * np.pi * 700.0 * np.arange(10000) / 32000.0)
    p = str(tmp_path / "clip.wav")
    wavfile.write(p, 32000, (wav.clip(-1, 1) * 32767).astype(np.int16))
    cfg = [(32, 2), (64, 2), (128, 2), (128, 1)]        # the model infer_file builds
    torch.manual_seed(0)
    model = sed.Csa_AvgPooling(sc.BENCH.classes_num, cfg, precision="fp32", mel_bins=sc.BENCH.mel_bins, sa_heads=2, sa_layers=2,
                               sa_ffn=256, sa_activation="gelu", sa_window=(6, None))
    ck = str(tmp_path / "m.pth")
    torch.save({"iterations": 0, "model": model.state_dict()}, ck)
    res = infer.infer_file(p, ck, precision="fp32", cfg=sc.BENCH, saliency=True)
    model = model.cuda().eval()
    with torch.no_grad():
        logits = model(torch.from_numpy(res["log_mel"]).cuda()[None, None])
        probs = torch.sigmoid(logits)[0]
    assert np.array_equal(res["probabilities"], probs.cpu().numpy()), "the rebuilt model gives other bits"
    assert np.isfinite(res["saliency"]).all()
    # and the window is in force: the same weights without it give other logits
    sd = {n: v for n, v in model.state_dict().items() if n != "window_config"}
    torch.manual_seed(0)
    plain = sed.Csa_AvgPooling(sc.BENCH.classes_num, cfg, precision="fp32", mel_bins=sc.BENCH.mel_bins, sa_heads=2, sa_layers=2,
                               sa_ffn=256, sa_activation="gelu")
    plain.load_state_dict(sd)
    plain = plain.cuda().eval()
    with torch.no_grad():
        assert not torch.equal(plain(torch.from_numpy(res["log_mel"]).cuda()[None, None]), logits)


# ---- at size: C = 128, t = 130, R = 520, window (40, 8) --------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_the_windowed_launches_at_size_against_float64(sed, precision):
    """4 heads of 32, one layer: ctx and lse of sed_mhsa_fwd_win from the engine's qkv (its thirds rounded to bf16 in bf16 mode), dq, dk,
    dv of sed_mhsa_bwd_win teacher-forced on the engine's own ctx, lse and dctx, every element"""
    import test_gpu_sa_at_size as S
    Bc, t, H, Cs, win = S.B, S.t, 4, S.C, (40, 8)
    dh = Cs // H
    torch.manual_seed(0)
    model = sed.Csa_AvgPooling(S.K, S.CFG, precision=precision, mel_bins=S.MEL, sa_heads=H, sa_window=win).cuda().train()
    x, y = S.batch()
    eng, P = model.engine, model._tensor_dict()
    G = {n: torch.full_like(p, float("nan")) for n, p in model.named_parameters()}
    plan = eng.forward(x, P, training=True)
    eng.loss_and_grad(plan, y, W)
    g = plan.sa
    assert g["R"] == S.R and plan.t_out == t
    snap = {}

    def cb(name):
        if name == "attn":
            snap.update(dctx=g["dctx"].clone(), dqkv=g["dqkv"].clone())

    eng.backward(plan, P, G, on_group_done=cb)
    torch.cuda.synchronize()
    ly = {n: S.f32(v) for n, v in g["layers"][0].items()}
    mode = "bf16" if precision == "bf16" else "f32"
    qkv = M.round_bf16(ly["qkv"]) if mode == "bf16" else ly["qkv"]
    q, k, v = M.split_qkv(qkv, Bc, t, H, dh)
    d4, ctx4 = S.f32(snap["dctx"]).reshape(Bc, t, H, dh), ly["ctx"].reshape(Bc, t, H, dh)
    ref = WF.core(q, k, v, *win, d4, lse=ly["lse"], ctx=ctx4)
    gates = WF.core_gates(q, k, v, *win, d4, mode=mode, lse=ly["lse"], ctx=ctx4, raw_dctx=mode == "bf16")
    got = dict(ctx=ctx4, lse=ly["lse"])
    got.update(zip(("dq", "dk", "dv"), M.split_qkv(S.f32(snap["dqkv"]), Bc, t, H, dh)))
    for name in ("ctx", "lse", "dq", "dk", "dv"):
        good, worst = WF.check(got[name], ref[name], gates[name], (precision, name))
        assert good, (precision, name, worst)
    # the window is seen: the unwindowed definition is far outside the gate
    far = M.core(q, k, v)["ctx"]
    assert float((np.abs(far - ctx4) / gates["ctx"]).max()) > 10
    lib = eng.lib
    assert lib.sed_mhsa_win_tiles(t, 40, 8, 0) == WF.tiles_brute(t, 40, 8, 0) < 25
