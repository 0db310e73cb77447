"""GPU: Csa_AvgPooling(sa_rel_pos=) through the model, the engine, FusedTrainer and infer.py, on the tiny configuration of
tests/test_gpu_sa_model.py / test_gpu_sa_conformer.py / test_gpu_sa_window.py (t = 10 frames per clip).

fp32 parity is against torch in float64 with a FLOAT src_mask / attn_mask per layer, mask[i][j] = rel_pos*.weight[g][bucket(j - i)]
gathered from a leaf tensor (so autograd gives the table's gradient) and -inf outside the window, fed by a head='none' engine on the
same parameters, whose backward takes the oracle's feature gradient.  Bounds, tests/test_gpu_crnn.py's: logits 1e-3 absolute, loss 1e-4,
every parameter gradient 3e-3 relative L2, rel_pos*.weight included (depthwise.bias by tests/test_gpu_sa_conformer.py's rule).  The tables
are set to N(0, 1) first; the oracle without the bias must be far outside the bound.
Measured on the MI355X (-s): fp32 logits off by at most 5e-7, worst gradient 8.4e-7 relative L2 (rel_pos.weight, eval mode), the oracle without
the bias 0.11 -- 0.73 away."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import convmod_formula as V
import ffn_formula as F
import mhsa_formula as M
import relpos_formula as RF
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


def make_model(sed, rel_pos, window=None, K=3, precision="fp32", layers=2, ffn=D, k=7, tables=True, **kw):
    m = T1.make_model(sed, K, precision, layers=layers, ffn=ffn, k=k, sa_window=window, sa_rel_pos=rel_pos, **kw)
    if rel_pos is not None and tables:
        g = torch.Generator().manual_seed(17)
        with torch.no_grad():
            for l in range(layers):
                w = m.get_parameter(sed.CnnEngine.sa_rel_name(l) + ".weight")
                w.copy_(torch.randn(w.shape, generator=g).to(w.device))
    return m


def oracle(sed, sd, feat, y, rel_pos, window, heads, layers, ffn, k, ratio, training=True):
    """tests/test_gpu_sa_window.py's oracle with the float mask of each layer's table (None: no bias) -> logits, loss, gradients by name"""
    Cc, t, Bc = feat.shape[-1], feat.shape[1], feat.shape[0]
    blocked = torch.from_numpy(WF.torch_mask(t, *(window if window is not None else (None, None))))
    cpu = lambda d: {n: (v.double() if v.is_floating_point() else v).cpu() for n, v in d.items()}
    enc, conv, tables = [], [], []
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
        if rel_pos is not None:
            tables.append(sd[sed.CnnEngine.sa_rel_name(l) + ".weight"].double().cpu().clone().requires_grad_(True))
    fc = torch.nn.Linear(Cc, sd["event_fc.weight"].shape[0]).double()
    fc.load_state_dict({n[len("event_fc."):]: v.double().cpu() for n, v in sd.items() if n.startswith("event_fc.")})
    idx = None if rel_pos is None else torch.from_numpy(RF.bucket_map(rel_pos, t).astype(np.int64)[RF.dist_index(t)])
    m = feat.mean(dim=2)
    h = m + torch.from_numpy(M.positional_table(t, Cc)).float().double()      # the table as rounded to fp32
    for l, e in enumerate(enc):
        bias = torch.zeros(heads, t, t, dtype=torch.float64) if rel_pos is None else tables[l][:, idx]
        mask = bias.masked_fill(blocked[None], float("-inf")).repeat(Bc, 1, 1)
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
        if rel_pos is not None:
            grads[sed.CnnEngine.sa_rel_name(l) + ".weight"] = tables[l].grad
    grads.update({"event_fc." + n: p.grad for n, p in fc.named_parameters()})
    return out.detach(), loss.detach(), grads


def compare(sed, model, x, y, rel_pos, window, layers, ffn, k, training, tag):
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
    out_t, loss_t, grads = oracle(sed, sd0, feat, y.double().cpu(), rel_pos, window, 1, layers, ffn, k, model.engine.ratio, training)
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
        if n.startswith("rel_pos"):
            assert float(g.norm()) > 0
    # the oracle's feature gradient back through the pinned conv backward
    bp.dy[-1].zero_()
    bp.dy[-1][..., :C] = feat.grad.float().cuda()
    names = [n for n, _ in model.named_parameters() if n.startswith("conv_blocks.")]
    G = {n: torch.full_like(P0[n], float("nan")) for n in names}
    bare.backward(bp, P0, G)
    for n in names:
        assert rel_l2(model.get_parameter(n).grad, G[n]) < 3e-3, n
    # the oracle without the bias is somewhere else: the bound sees the tables
    plain = oracle(sed, sd0, feat.detach().clone().requires_grad_(True), y.double().cpu(), None, window, 1, layers, ffn, k, model.engine.ratio,
                   training)[0]
    seen = float((out.detach().cpu().double() - plain).abs().max())
    print(f"{tag}: the oracle without the bias is {seen:.3e} away")
    assert seen > 2e-3


def test_fp32_two_layer_windowed_model_matches_torch_with_a_float_src_mask(sed):
    x, y = batch()
    model = make_model(sed, 3, (4, 2))
    assert model.engine.sa_rel_pos == ("clip", 3) and model.rel_pos_config.tolist() == [0.0, 3.0, 0.0]
    compare(sed, model, x, y, 3, (4, 2), 2, D, 7, True, "2 layers, gelu FFN, k = 7, window (4, 2), L = 3")


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_fp32_one_layer_log_bucket_model_matches_torch(sed, training):
    x, y = batch()
    model = make_model(sed, (8, 16), None, layers=1, ffn=0, k=0)
    compare(sed, model, x, y, (8, 16), None, 1, 0, 0, training, f"1 layer, unwindowed, (8, 16) buckets, training={training}")


@pytest.mark.parametrize("precision", ["bf16", "f16x3", "bf16x3"])
def test_other_precisions_follow_fp32(sed, precision):
    """tests/test_gpu_sa_conformer.py's bounds for the same stack: the bias adds one fp32 add per score in every precision"""
    x, y = batch()
    ref, model = make_model(sed, 3, (4, 2)).train(), make_model(sed, 3, (4, 2), precision=precision).train()
    lr = sed.WeightedBCE(W, True)(ref(x), y)
    lm = sed.WeightedBCE(W, True)(model(x), y)
    lr.backward()
    lm.backward()
    print(f"{precision}: loss difference {abs(lr.item() - lm.item()):.3e}")
    assert abs(lr.item() - lm.item()) < (6e-2 if precision == "bf16" else 6e-3)
    for (n, p), (_, q) in zip(ref.named_parameters(), model.named_parameters()):
        assert bool(torch.isfinite(q.grad).all()), n
        if n.startswith(("attn", "ffn", "event_fc", "convm", "conv_norm", "rel_pos")) and not n.endswith("depthwise.bias"):
            assert rel_l2(q.grad, p.grad) < (0.3 if precision == "bf16" else 4e-2), (precision, n, rel_l2(q.grad, p.grad))


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_graph_steps_give_the_eager_bits_and_train_the_table(sed, p):
    x, y = batch()

    def fresh():
        return sed.FusedTrainer(make_model(sed, (8, 16), (4, 2), precision="bf16", tables=False, sa_dropout=p, sa_dropout_seed=7), lr=1e-3,
                                recall_factor=W, graph=True)

    eager, graph = fresh(), fresh()
    assert not eager.flat.P["rel_pos.weight"].any()
    for i in range(4):              # launch by launch / two eager steps, the capture, a replay
        le = eager._step_dev(x, y).clone()
        eager._host_mirror()
        lg = graph.train_step(x, y).clone()
        assert torch.equal(le, lg), (i, "the graph step's loss differs from the eager step's")
        assert torch.equal(eager.flat.p, graph.flat.p), i
    assert len(graph._graphs) == 1 and len(eager._graphs) == 0
    for l in range(2):
        w = graph.flat.P[sed.CnnEngine.sa_rel_name(l) + ".weight"]
        assert bool(torch.isfinite(w).all()) and float(w.abs().max()) > 0, "the table did not move from zero"


def test_options_take_a_step(sed):
    x, y = batch()
    finite = lambda tr: all(bool(torch.isfinite(g).all()) for g in tr.flat.G.values())
    tr = sed.FusedTrainer(make_model(sed, 3, (4, 2), attention=True), lr=1e-3, recall_factor=W, weak_pooling="att", weak_only=True)
    for v in tr.flat.G.values():
        v.fill_(float("nan"))
    tr.forward_backward(x, y)
    assert finite(tr) and float(tr.flat.G["rel_pos.weight"].abs().max()) > 0
    tr.forward_backward(x, y, torch.tensor([1, 2], device="cuda"))          # label kinds
    assert finite(tr)
    mt = sed.FusedTrainer(make_model(sed, (8, 16), (4, None), sa_dropout=0.1, sa_dropout_seed=5), lr=1e-3, recall_factor=W, mean_teacher=True,
                          consistency_weight=2.0)
    assert mt.teacher.engine is not mt.model.engine and mt.teacher.engine.sa_rel_pos == ("log", 8, 16) == mt.teacher.sa_rel_pos
    assert mt.teacher.state_dict()["rel_pos_config"].tolist() == [1.0, 8.0, 16.0]
    before = mt.teacher_flat.P["rel_pos_l1.weight"].clone()
    for _ in range(2):
        loss = mt.train_step(x, y)
    assert bool(torch.isfinite(loss).all())
    assert not torch.equal(before, mt.teacher_flat.P["rel_pos_l1.weight"]), "the EMA does not reach the table"
    opt = sed.FusedTrainer(make_model(sed, 3), lr=1e-3, recall_factor=W, weight_decay=1e-2, decoupled_weight_decay=True, max_grad_norm=0.5)
    assert bool(torch.isfinite(opt.train_step(x, y)).all())
    fe = sed.PCEN(MEL, trainable=True)
    pt = sed.FusedTrainer(make_model(sed, 3, (0, 3), frontend=fe), lr=1e-3, recall_factor=W)
    pt.train_step(x.abs() + 0.1, y)
    assert finite(pt)
    # need_dx in training mode and the eval-mode backward, which still produces dw
    for training in (True, False):
        model = make_model(sed, 3, (3, 0)).train(training)
        xg = x.clone().requires_grad_(True)
        model(xg).sum().backward()
        assert bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0, training
        assert float(model.attn.in_proj_weight.grad.abs().max()) > 0
        for l in range(2):
            g = model.get_parameter(sed.CnnEngine.sa_rel_name(l) + ".weight").grad
            assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, (training, l)


def test_groups_complete_in_flat_order(sed):
    """on_group_done fires for rel_pos* after attn_norm* and before attn*, the reverse of the parameter order, once dw is written"""
    x, y = batch()
    model = make_model(sed, 3, (4, 2)).train()
    tr = sed.FusedTrainer(model, lr=1e-3, recall_factor=W)
    eng, P = model.engine, tr.flat.tensor_dict()
    plan = eng.forward(x, P, training=True)
    eng.loss_and_grad(plan, y, W)
    for v in tr.flat.G.values():
        v.fill_(float("nan"))
    seen, ready = [], {}

    def cb(name):
        seen.append(name)
        if name.startswith("rel_pos"):
            ready[name] = bool(torch.isfinite(tr.flat.G[name + ".weight"]).all())

    eng.backward(plan, P, tr.flat.G, on_group_done=cb)
    torch.cuda.synchronize()
    assert seen == [k for k, _, _ in tr.flat.groups], (seen, [k for k, _, _ in tr.flat.groups])
    assert ready == {"rel_pos": True, "rel_pos_l1": True}
    i = seen.index("rel_pos")
    assert seen[i - 1] == "attn_norm" and seen[i + 1] == "attn"


def test_launch_labels(sed):
    """sa_rel_pos=None: the list of tests/test_gpu_sa_model.py; with the option the two core names replaced and expand / fold added"""
    torch.manual_seed(0)
    sa = T0.step_labels(sed, sed.Csa_AvgPooling(3, CFG, precision="bf16", sa_heads=1, sa_rel_pos=None).cuda())
    h, b = T0.PLAIN_STEP.index("sed_head_fwd"), T0.PLAIN_STEP.index("sed_head_bwd")
    assert sa == T0.PLAIN_STEP[:h] + T0.SA_FWD + T0.PLAIN_STEP[h + 1:b] + T0.SA_BWD + T0.PLAIN_STEP[b + 1:]
    want = []
    for l in sa:
        want += ["sed_relpos_expand", "sed_mhsa_fwd_rel"] if l == "sed_mhsa_fwd" else ["sed_mhsa_bwd_rel", "sed_relpos_fold"] if l == "sed_mhsa_bwd" else [l]
    for kw in (dict(sa_rel_pos=3), dict(sa_rel_pos=(8, 16), sa_window=(2, 1))):
        got = T0.step_labels(sed, sed.Csa_AvgPooling(3, CFG, precision="bf16", sa_heads=1, **kw).cuda())
        assert got == want, kw
    x, y = batch()
    model = make_model(sed, 3, (2, 1)).train()
    eng, P = model.engine, model._tensor_dict()
    eng.timer = sed.engine.KernelTimer()
    plan = eng.forward(x, P, training=True)
    eng.loss_and_grad(plan, y, W)
    eng.backward(plan, P, {n: torch.empty_like(p) for n, p in model.named_parameters()})
    torch.cuda.synchronize()
    labels = [lbl for lbl, _, _ in eng.timer.records]
    for name in ("sed_relpos_expand", "sed_mhsa_fwd_rel", "sed_mhsa_bwd_rel", "sed_relpos_fold"):
        assert [l for l in labels if l.split(":")[0] == name] == [name + ":sa"] * 2, name
    assert not [l for l in labels if l.split(":")[0] in ("sed_mhsa_fwd", "sed_mhsa_bwd", "sed_mhsa_fwd_win", "sed_mhsa_bwd_win")]


def test_a_zero_table_gives_the_windowed_models_bits(sed):
    """the initial model (tables zero) computes what the model without the option computes, bit for bit, and its table gets a gradient"""
    x, y = batch()
    relm, plain = make_model(sed, (8, 16), (4, 2), tables=False), make_model(sed, None, (4, 2))
    for m in (relm, plain):
        m.train()
        sed.WeightedBCE(W, True)(m(x), y).backward()
    assert torch.equal(the_plan(relm).pre, the_plan(plain).pre)
    for n, b in plain.named_parameters():
        assert torch.equal(relm.get_parameter(n).grad, b.grad), n
    assert float(relm.rel_pos.weight.grad.abs().max()) > 0


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
    kw = dict(precision="fp32", mel_bins=sc.BENCH.mel_bins, sa_heads=2, sa_layers=2, sa_ffn=256, sa_activation="gelu", pos_encoding=False)
    torch.manual_seed(0)
    model = sed.Csa_AvgPooling(sc.BENCH.classes_num, cfg, sa_rel_pos=(32, 128), sa_window=(6, None), **kw)
    with torch.no_grad():
        model.rel_pos.weight.normal_()
        model.rel_pos_l1.weight.normal_()
    ck = str(tmp_path / "m.pth")
    torch.save({"iterations": 0, "model": model.state_dict()}, ck)
    res = infer.infer_file(p, ck, precision="fp32", cfg=sc.BENCH, saliency=True)
    model = model.cuda().eval()
    with torch.no_grad():
        logits = model(torch.from_numpy(res["log_mel"]).cuda()[None, None])
        probs = torch.sigmoid(logits)[0]
    assert np.array_equal(res["probabilities"], probs.cpu().numpy()), "the rebuilt model gives other bits"
    assert np.isfinite(res["saliency"]).all()
    # and the tables are in force: the same weights without them give other logits
    sd = {n: v for n, v in model.state_dict().items() if not n.startswith("rel_pos")}
    torch.manual_seed(0)
    plain = sed.Csa_AvgPooling(sc.BENCH.classes_num, cfg, sa_window=(6, None), **kw)
    plain.load_state_dict(sd)
    plain = plain.cuda().eval()
    with torch.no_grad():
        assert not torch.equal(plain(torch.from_numpy(res["log_mel"]).cuda()[None, None]), logits)
