"""GPU: Csa_AvgPooling with a feed-forward sub-layer and stacked layers (csrc/sed_ffn.hip) through the model, the engine, FusedTrainer
and infer.py, on the tiny configuration of tests/test_gpu_sa_model.py.

fp32 parity as in that file: the conv-stack output of a head='none' engine on the same parameters is fed to the torch CPU oracle in
float64 -- torch.nn.TransformerEncoderLayer(C, H, D, dropout=0, activation=..., batch_first=True, norm_first=False) per layer, loaded
through Csa_AvgPooling.encoder_layer_state, + the linear layer + interpolate + the weighted BCE, with autograd.  Bounds as there
(tests/test_gpu_crnn.py's): fp32 logits 1e-3 absolute, loss 1e-4, every parameter gradient 3e-3 relative L2."""
import importlib

import numpy as np
import pytest
import torch

import ffn_formula as F
import mhsa_formula as M
import test_gpu_sa_model as T0

pytestmark = pytest.mark.gpu
PKG = "soundeventdetection-pytorch_amd"
CFG, MEL, T, B, W = T0.CFG, T0.MEL, T0.T, T0.B, T0.W
C, D = CFG[-1][0], 64
rel_l2, batch, the_plan = T0.rel_l2, T0.batch, T0.the_plan


@pytest.fixture(scope="module")
def sed():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)


def make_model(sed, K=3, precision="fp32", seed=0, layers=2, ffn=D, act="gelu", **kw):
    torch.manual_seed(seed)
    kw.setdefault("sa_heads", 1)
    m = sed.Csa_AvgPooling(K, CFG, precision=precision, mel_bins=MEL, sa_layers=layers, sa_ffn=ffn, sa_activation=act, **kw)
    with torch.no_grad():       # the zero / unit initial values would hide a wrong bias or affine gradient
        for n, p in m.named_parameters():
            if n.startswith(("attn", "ffn")):
                if "norm" in n and n.endswith("weight"):
                    p.normal_(1.0, 0.2)
                elif n.endswith("bias"):
                    p.normal_(0.0, 0.1)
    return m.cuda()


def oracle(sed, sd, feat, y, heads, layers, ffn, act, pos, ratio):
    """feat (B, t, Wf, C) float64 with requires_grad -> (logits, loss, parameter gradients by state_dict name)"""
    C = feat.shape[-1]          # (tests/test_gpu_sa_at_size.py calls this at another width than this module's)
    enc =[torch.nn.TransformerEncoderLayer(C, heads, ffn, dropout=0.0, activation=act, batch_first=True, norm_first=False).double()
           for _ in range(layers)]
    for l, ly in enumerate(enc):
        ly.load_state_dict({k: v.double().cpu() for k, v in sed.Csa_AvgPooling.encoder_layer_state(sd, l).items()})
    fc = torch.nn.Linear(C, sd["event_fc.weight"].shape[0]).double()
    fc.load_state_dict({n[len("event_fc."):]: v.double().cpu() for n, v in sd.items() if n.startswith("event_fc.")})
    m = feat.mean(dim=2)
    h = m + torch.from_numpy(M.positional_table(m.shape[1], C)).float().double() if pos else m       # the table as rounded to fp32
    for ly in enc:
        h = ly(h)
    out = fc(h).repeat_interleave(ratio, dim=1)
    N = min(out.shape[1], y.shape[1])
    loss = torch.nn.functional.binary_cross_entropy_with_logits(out[:, :N], y[:, :N], pos_weight=torch.tensor(W, dtype=torch.float64))
    loss.backward()
    inv = {"self_attn": 0, "norm1": 1, "linear1": 2, "linear2": 2, "norm2": 3}
    grads = {}
    for l, ly in enumerate(enc):
        names = F.layer_names(l)
        for n, p in ly.named_parameters():
            top, rest = n.split(".", 1)
            ours = names[inv[top]]
            grads[ours + "." + (top + "." + rest if top.startswith("linear") else rest)] = p.grad
    grads.update({"event_fc." + n: p.grad for n, p in fc.named_parameters()})
    return out.detach(), loss.detach(), grads


@pytest.mark.parametrize("layers,act", [(2, "gelu"), (1, "relu")])
def test_fp32_model_matches_the_torch_encoder(sed, layers, act):
    K = 3
    x, y = batch(K)
    model = make_model(sed, K, layers=layers, act=act).train()
    out = model(x)
    loss = sed.WeightedBCE(W, True)(out, y)
    loss.backward()
    plan = the_plan(model)
    assert plan.sa is not None and len(plan.sa["layers"]) == layers
    P = model._tensor_dict()
    bare = sed.CnnEngine(K, CFG, 1, "fp32", head="none", mel_bins=MEL)
    bp = bare.forward(x, P, training=True, update_running_stats=False)
    assert torch.equal(bp.y[-1], plan.y[-1])
    feat = bp.y[-1][..., :C].double().cpu().requires_grad_(True)
    out_t, loss_t, grads = oracle(sed, model.state_dict(), feat, y.double().cpu(), 1, layers, D, act, True, model.engine.ratio)
    err = float((out.cpu().double() - out_t).abs().max())
    print(f"layers={layers} act={act}: logits max error {err:.3e}, loss error {abs(loss.item() - float(loss_t)):.3e}")
    assert err < 1e-3 and abs(loss.item() - float(loss_t)) < 1e-4
    mine = {n for n, _ in model.named_parameters() if not n.startswith("conv_blocks.")}
    assert mine == set(grads), mine ^ set(grads)
    for n, g in grads.items():
        l2 = rel_l2(model.get_parameter(n).grad, g)
        print(f"  {n}: relative L2 {l2:.3e}")
        assert l2 < 3e-3, (n, l2)
    # the oracle's feature gradient back through the pinned conv backward
    bp.dy[-1].zero_()
    bp.dy[-1][..., :C] = feat.grad.float().cuda()
    names = [n for n, _ in model.named_parameters() if n.startswith("conv_blocks.")]
    G = {n: torch.full_like(P[n], float("nan")) for n in names}
    bare.backward(bp, P, G)
    for n in names:
        assert rel_l2(model.get_parameter(n).grad, G[n]) < 3e-3, n
    # an eval forward stores no pre-activation and gives the training forward's head arithmetic on running statistics: finite;
    # under grad mode it can be differentiated, and the input gradient exists in training mode (need_dx)
    model.eval()
    with torch.no_grad():
        e = model(x)
    assert bool(torch.isfinite(e).all()) and e.shape == out.shape
    for training in (False, True):
        model.train(training)
        xg = x.clone().requires_grad_(True)
        model.zero_grad()
        model(xg).sum().backward()
        assert bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0, training
        assert float(model.get_parameter("ffn.linear1.weight").grad.abs().max()) > 0, training


@pytest.mark.parametrize("precision", ["bf16", "f16x3", "bf16x3"])
def test_other_precisions_follow_fp32(sed, precision):
    """Bounds as tests/test_gpu_sa_model.py derives them for the one-layer head; the two-layer stack with FFNs doubles the number of
    bf16 operand roundings a head gradient passes (about twenty, 8e-2), held to 0.3 relative L2, and the loss to 6e-2."""
    x, y = batch()
    ref, model = make_model(sed).train(), make_model(sed, precision=precision).train()
    lr = sed.WeightedBCE(W, True)(ref(x), y)
    lm = sed.WeightedBCE(W, True)(model(x), y)
    lr.backward()
    lm.backward()
    assert abs(lr.item() - lm.item()) < (6e-2 if precision == "bf16" else 6e-3)
    for (n, p), (_, q) in zip(ref.named_parameters(), model.named_parameters()):
        assert bool(torch.isfinite(q.grad).all()), n
        if n.startswith(("attn", "ffn", "event_fc")):
            assert rel_l2(q.grad, p.grad) < (0.3 if precision == "bf16" else 4e-2), (precision, n, rel_l2(q.grad, p.grad))


def test_graph_steps_give_the_eager_bits(sed):
    x, y = batch()

    def fresh():
        return sed.FusedTrainer(make_model(sed, precision="bf16"), lr=1e-3, recall_factor=W, graph=True)

    eager, graph = fresh(), fresh()
    for i in range(4):              # launch by launch / two eager steps, the capture, a replay
        le = eager._step_dev(x, y).clone()
        eager._host_mirror()
        lg = graph.train_step(x, y).clone()
        assert torch.equal(le, lg), (i, "the graph step's loss differs from the eager step's")
        assert torch.equal(eager.flat.p, graph.flat.p), i
    assert len(graph._graphs) == 1 and len(eager._graphs) == 0


def test_attention_pooling_and_mean_teacher(sed):
    x, y = batch()
    model = make_model(sed, attention=True)
    tr = sed.FusedTrainer(model, lr=1e-3, recall_factor=W, weak_pooling="att", weak_only=True)
    for v in tr.flat.G.values():
        v.fill_(float("nan"))
    tr.forward_backward(x, y)
    for n, g in tr.flat.G.items():
        assert bool(torch.isfinite(g).all()), n
        if n.startswith(("attn", "ffn", "att_fc.")):
            assert float(g.abs().max()) > 0, n
    mt = sed.FusedTrainer(make_model(sed), lr=1e-3, recall_factor=W, mean_teacher=True, consistency_weight=2.0)
    teacher = mt.teacher
    assert isinstance(teacher, sed.Csa_AvgPooling) and teacher.engine is not mt.model.engine
    assert (teacher.engine.sa_layers, teacher.engine.sa_ffn, teacher.engine.sa_activation) == (2, D, "gelu")
    before = mt.teacher_flat.P["ffn_l1.linear2.weight"].clone()
    for _ in range(2):
        loss = mt.train_step(x, y)
    assert bool(torch.isfinite(loss).all()) and not torch.equal(before, mt.teacher_flat.P["ffn_l1.linear2.weight"])


def test_backward_completion_order_and_launch_labels(sed):
    x, y = batch()
    model = make_model(sed).train()
    eng, P = model.engine, model._tensor_dict()
    G = {n: torch.empty_like(p) for n, p in model.named_parameters()}
    plan = eng.forward(x, P, training=True)
    eng.loss_and_grad(plan, y, W)
    done = []
    eng.timer = sed.engine.KernelTimer()
    eng.backward(plan, P, G, on_group_done=done.append)
    torch.cuda.synchronize()
    assert done == ["event_fc", "ffn_norm_l1", "ffn_l1", "attn_norm_l1", "attn_l1", "ffn_norm", "ffn", "attn_norm", "attn",
                    "conv_blocks.1", "conv_blocks.0"]
    tagged = [lbl for lbl, _, _ in eng.timer.records if lbl.split(":")[0] == "sed_ffn_act_bwd"]
    assert tagged == ["sed_ffn_act_bwd:sa"] * 2, tagged
    # a default model records exactly the launch labels tests/test_gpu_sa_model.py lists
    torch.manual_seed(0)
    sa = T0.step_labels(sed, sed.Csa_AvgPooling(3, CFG, precision="bf16", sa_heads=1).cuda())
    h, b = T0.PLAIN_STEP.index("sed_head_fwd"), T0.PLAIN_STEP.index("sed_head_bwd")
    assert sa == T0.PLAIN_STEP[:h] + T0.SA_FWD + T0.PLAIN_STEP[h + 1:b] + T0.SA_BWD + T0.PLAIN_STEP[b + 1:]
    full = T0.step_labels(sed, sed.Csa_AvgPooling(3, CFG, precision="bf16", sa_heads=1, sa_ffn=64).cuda())
    assert full.count("sed_ffn_fwd") == 1 and full.count("sed_ffn_act_bwd") == 1 and full.count("sed_add_layernorm_fwd") == 2


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
                               sa_ffn=256, sa_activation="gelu")
    ck = str(tmp_path / "m.pth")
    torch.save({"iterations": 0, "model": model.state_dict()}, ck)
    res = infer.infer_file(p, ck, precision="fp32", cfg=sc.BENCH, clip_pooling="linear", saliency=True)
    model = model.cuda().eval()
    with torch.no_grad():
        probs = torch.sigmoid(model(torch.from_numpy(res["log_mel"]).cuda()[None, None]))[0]
    assert np.array_equal(res["probabilities"], probs.cpu().numpy()), "the rebuilt model gives other bits"
    assert "clip_probs" in res and np.isfinite(res["saliency"]).all()
