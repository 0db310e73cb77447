"""GPU: Csa_AvgPooling (the self-attention temporal head, csrc/sed_mhsa.hip) through the model, the engine, FusedTrainer and infer.py.

fp32 parity is against a composition of already-pinned pieces: the conv-stack output of a head='none' engine on the same
parameters (the same bits as the model's own stack) is fed to the torch CPU oracle of the head in float64
(torch.nn.MultiheadAttention + torch.nn.LayerNorm + the linear layer + interpolate + the weighted BCE, with autograd), and the
oracle's gradient of the conv features goes back through that engine's backward.  Tolerances as tests/test_gpu_crnn.py sets them
for the recurrent head: fp32 logits 1e-3 absolute, loss 1e-4, every parameter gradient 3e-3 relative L2; bf16: the loss of a few
trainer steps tracks the fp32 model's within 0.05 (5e-3 at the first step) and falls, and the whole step is bit-reproducible."""
import importlib

import numpy as np
import pytest
import torch

import mhsa_formula as F

pytestmark = pytest.mark.gpu
PKG = "soundeventdetection-pytorch_amd"
CFG = [(32, 2), (32, 2)]
MEL, T, B = 8, 40, 2
W = 5.0


@pytest.fixture(scope="module")
def sed():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return float((a - b).norm() / max(b.norm().item(), 1e-30))


def make_model(sed, K=3, precision="fp32", seed=0, **kw):
    torch.manual_seed(seed)
    kw.setdefault("sa_heads", 1)
    m = sed.Csa_AvgPooling(K, CFG, precision=precision, mel_bins=MEL, **kw)
    with torch.no_grad():       # the zero / unit initial values would hide a wrong bias or affine gradient
        for n in ("attn.in_proj_bias", "attn.out_proj.bias", "attn_norm.bias"):
            m.get_parameter(n).normal_(0.0, 0.1)
        m.attn_norm.weight.normal_(1.0, 0.2)
    return m.cuda()


def batch(K=3):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 1, T, MEL, generator=g)
    y = (torch.rand(B, T, K, generator=g) < 0.3).float()
    return x.cuda(), y.cuda()


def the_plan(model):
    plans = list(model.engine._plans.values())
    assert len(plans) == 1
    return plans[0]


def oracle_head(sd, feat, y, heads, pos, ratio):
    """feat (B, t, Wf, C) float64 with requires_grad -> (logits, loss, parameter gradients by state_dict name)"""
    C = feat.shape[-1]
    mha = torch.nn.MultiheadAttention(C, heads, batch_first=True).double()
    ln = torch.nn.LayerNorm(C).double()
    fc = torch.nn.Linear(C, sd["event_fc.weight"].shape[0]).double()
    mha.load_state_dict({n[len("attn."):]: v.double().cpu() for n, v in sd.items() if n.startswith("attn.")})
    ln.load_state_dict({n[len("attn_norm."):]: v.double().cpu() for n, v in sd.items() if n.startswith("attn_norm.")})
    fc.load_state_dict({n[len("event_fc."):]: v.double().cpu() for n, v in sd.items() if n.startswith("event_fc.")})
    m = feat.mean(dim=2)
    xp = m + torch.from_numpy(F.positional_table(m.shape[1], C)).float().double() if pos else m      # the table as rounded to fp32
    a, _ = mha(xp, xp, xp, need_weights=False)
    out = fc(ln(xp + a)).repeat_interleave(ratio, dim=1)
    N = min(out.shape[1], y.shape[1])
    loss = torch.nn.functional.binary_cross_entropy_with_logits(out[:, :N], y[:, :N], pos_weight=torch.tensor(W, dtype=torch.float64))
    loss.backward()
    grads = {"attn." + n: p.grad for n, p in mha.named_parameters()}
    grads.update({"attn_norm." + n: p.grad for n, p in ln.named_parameters()})
    grads.update({"event_fc." + n: p.grad for n, p in fc.named_parameters()})
    return out.detach(), loss.detach(), grads


@pytest.mark.parametrize("pos", [True, False], ids=["pe", "nope"])
@pytest.mark.parametrize("K", [1, 3])
def test_fp32_model_matches_the_composition(sed, K, pos):
    x, y = batch(K)
    model = make_model(sed, K, pos_encoding=pos).train()
    C = CFG[-1][0]
    out = model(x)
    loss = sed.WeightedBCE(W, True)(out, y)
    loss.backward()
    plan = the_plan(model)
    assert plan.sa is not None and plan.gru is None and plan.pre.shape == (B, T // 4, K)
    # the conv stack of a head='none' engine on the same parameters: the same bits
    P = model._tensor_dict()
    bare = sed.CnnEngine(K, CFG, 1, "fp32", head="none", mel_bins=MEL)
    bp = bare.forward(x, P, training=True, update_running_stats=False)
    assert torch.equal(bp.y[-1], plan.y[-1])
    feat = bp.y[-1][..., :C].double().cpu().requires_grad_(True)
    out_t, loss_t, grads = oracle_head(model.state_dict(), feat, y.double().cpu(), 1, pos, model.engine.ratio)
    assert out.shape == out_t.shape
    err = float((out.cpu().double() - out_t).abs().max())
    print(f"K={K} pos={pos}: logits max error {err:.3e}, loss error {abs(loss.item() - float(loss_t)):.3e}")
    assert err < 1e-3 and abs(loss.item() - float(loss_t)) < 1e-4
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
        l2 = rel_l2(model.get_parameter(n).grad, G[n])
        assert l2 < 3e-3, (n, l2)
    # an eval forward saves nothing and gives finite logits; under grad mode it can be differentiated (running statistics)
    model.eval()
    with torch.no_grad():
        e = model(x)
    assert bool(torch.isfinite(e).all()) and e.shape == out.shape
    xg = x.clone().requires_grad_(True)
    model.zero_grad()
    model(xg).sum().backward()
    assert bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0
    assert float(model.attn.in_proj_weight.grad.abs().max()) > 0


def test_input_gradient_in_training_mode(sed):
    x, y = batch()
    model = make_model(sed).train()
    xg = x.clone().requires_grad_(True)
    sed.WeightedBCE(W, True)(model(xg), y).backward()
    assert xg.grad.shape == x.shape and bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0


@pytest.mark.parametrize("precision", ["bf16", "f16x3", "bf16x3"])
def test_other_precisions_follow_fp32(sed, precision):
    """The same weights and batch in fp32 and in another mode.  bf16 has a unit roundoff of 2^-8 = 3.9e-3: four conv layers store their
    activations in it and every product rounds its operands to it, forward and backward, so a gradient of the head carries on the
    order of ten such roundings one after another (4e-2) and is held to 0.15 relative L2, the loss (a mean of 240 terms, each off by a
    few 2^-8 of an O(1) logit) to 3e-2.  The split-operand modes keep fp32 tensors and are good to 1e-5 per product (bf16x3) or
    better: 2e-2 and 3e-3 leave the room tests/test_gpu_crnn.py leaves the fp32 mode (3e-3 on gradients) times the stack's depth."""
    x, y = batch()
    ref, model = make_model(sed).train(), make_model(sed, precision=precision).train()
    lr = sed.WeightedBCE(W, True)(ref(x), y)
    lm = sed.WeightedBCE(W, True)(model(x), y)
    lr.backward()
    lm.backward()
    tol = 3e-2 if precision == "bf16" else 3e-3
    assert abs(lr.item() - lm.item()) < tol
    for (n, p), (_, q) in zip(ref.named_parameters(), model.named_parameters()):
        assert bool(torch.isfinite(q.grad).all()), n
        if n.startswith(("attn", "event_fc")):
            assert rel_l2(q.grad, p.grad) < (0.15 if precision == "bf16" else 2e-2), (precision, n, rel_l2(q.grad, p.grad))


def test_bf16_training_tracks_fp32_and_is_reproducible(sed):
    x, y = batch()

    def run(precision):
        tr = sed.FusedTrainer(make_model(sed, precision=precision), lr=1e-3, recall_factor=W)
        return [float(tr.train_step(x, y)) for _ in range(6)]

    lf, lb, lb2 = run("fp32"), run("bf16"), run("bf16")
    print("fp32 losses", lf, "bf16 losses", lb)
    assert lb[-1] < lb[0] and abs(lb[0] - lf[0]) < 5e-3
    assert max(abs(a - b) for a, b in zip(lb, lf)) < 0.05
    assert lb == lb2, "the bf16 step is not bit-reproducible"


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


def test_attention_pooling_step_fills_every_gradient(sed):
    x, y = batch()
    model = make_model(sed, attention=True)
    tr = sed.FusedTrainer(model, lr=1e-3, recall_factor=W, weak_pooling="att", weak_only=True)
    for v in tr.flat.G.values():
        v.fill_(float("nan"))
    tr.forward_backward(x, y)
    assert the_plan(model).att_pending
    for n, g in tr.flat.G.items():
        assert bool(torch.isfinite(g).all()), n
        if n.startswith(("attn.", "attn_norm.", "att_fc.")):
            assert float(g.abs().max()) > 0, n
    # label kinds (clip 0 weak, clip 1 unlabelled) and a parameter-free pooling run on the same model
    tr.forward_backward(x, y, torch.tensor([1, 2], device="cuda"))
    lin = sed.FusedTrainer(make_model(sed, attention=True), lr=1e-3, recall_factor=W, weak_pooling="linear", weak_only=True)
    lin.train_step(x, y)
    assert all(bool(torch.isfinite(v).all()) for v in lin.flat.G.values()) and not lin.flat.G["att_fc.weight"].any()


def test_mean_teacher_optimizer_options_and_pcen(sed):
    x, y = batch()
    mt = sed.FusedTrainer(make_model(sed), lr=1e-3, recall_factor=W, mean_teacher=True, consistency_weight=2.0)
    assert isinstance(mt.teacher, sed.Csa_AvgPooling) and mt.teacher.engine.head == "sa" and mt.teacher.engine is not mt.model.engine
    before = mt.teacher_flat.P["attn.in_proj_weight"].clone()
    for _ in range(2):
        loss = mt.train_step(x, y)
    assert bool(torch.isfinite(loss).all()) and not torch.equal(before, mt.teacher_flat.P["attn.in_proj_weight"])
    opt = sed.FusedTrainer(make_model(sed), lr=1e-3, recall_factor=W, weight_decay=1e-2, decoupled_weight_decay=True, max_grad_norm=0.5)
    start = opt.flat.P["attn.in_proj_weight"].clone()
    assert bool(torch.isfinite(opt.train_step(x, y)).all()) and not torch.equal(start, opt.flat.P["attn.in_proj_weight"])
    fe = sed.PCEN(MEL, trainable=True)
    pm = make_model(sed, frontend=fe)
    pt = sed.FusedTrainer(pm, lr=1e-3, recall_factor=W)
    pt.train_step(x.abs() + 0.1, y)
    assert all(bool(torch.isfinite(v).all()) for v in pt.flat.G.values()) and float(pt.flat.G["attn.out_proj.weight"].abs().max()) > 0


def test_backward_completion_order_on_the_device(sed):
    x, y = batch()
    model = make_model(sed, attention=True).train()
    eng, P = model.engine, model._tensor_dict()
    G = {n: torch.empty_like(p) for n, p in model.named_parameters()}
    plan = eng.forward(x, P, training=True)
    eng.loss_and_grad(plan, y, W)
    done = []
    eng.backward(plan, P, G, on_group_done=done.append)
    assert done == ["att_fc", "event_fc", "attn_norm", "attn", "conv_blocks.1", "conv_blocks.0"]


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
    model = sed.Csa_AvgPooling(sc.BENCH.classes_num, cfg, precision="fp32", mel_bins=sc.BENCH.mel_bins, sa_heads=2, pos_encoding=False)
    ck = str(tmp_path / "m.pth")
    torch.save({"iterations": 0, "model": model.state_dict()}, ck)
    res = infer.infer_file(p, ck, precision="fp32", cfg=sc.BENCH, clip_pooling="linear", saliency=True)
    model = model.cuda().eval()
    with torch.no_grad():
        probs = torch.sigmoid(model(torch.from_numpy(res["log_mel"]).cuda()[None, None]))[0]
    assert np.array_equal(res["probabilities"], probs.cpu().numpy()), "the rebuilt model gives other bits"
    assert "clip_probs" in res and np.isfinite(res["saliency"]).all()
    # the heads and the positional flag came from attn_config: another setting gives other logits
    other = sed.Csa_AvgPooling(sc.BENCH.classes_num, cfg, precision="fp32", mel_bins=sc.BENCH.mel_bins, sa_heads=4, pos_encoding=False)
    sd = model.state_dict()
    other.load_state_dict(sd)
    other = other.cuda().eval()
    with torch.no_grad():
        p4 = torch.sigmoid(other(torch.from_numpy(res["log_mel"]).cuda()[None, None]))[0]
    assert not torch.equal(p4, probs)


# the launch labels of one eager bf16 train step of Cnn_AvgPooling(3, [(32, 2), (32, 2)]) as tests/test_gpu_att.py writes them out
PLAIN_STEP = ["sed_pack_conv_weights_batch", "sed_conv3x3_c1_gram", "sed_bn_train_finalize_c1", "sed_conv3x3_fwd_c1",
              "sed_bn_train_finalize", "sed_bn_relu_pool_cnt_fwd", "sed_conv3x3_fwd", "sed_bn_train_finalize", "sed_conv3x3_fwd",
              "sed_bn_train_finalize", "sed_bn_relu_pool_fwd", "sed_head_fwd", "sed_bce_fwd_bwd", "sed_head_bwd",
              "sed_pool_relu_bwd_stats", "sed_bn_bwd_finalize", "sed_conv3x3_wgrad_fused", "sed_conv3x3_fwd", "sed_bn_bwd_finalize",
              "sed_conv3x3_wgrad_fused", "sed_conv3x3_dgrad_poolstats", "sed_pool_relu_bwd_stats_if", "sed_bn_bwd_finalize",
              "sed_conv3x3_bwd_fused_c1", "sed_c1_bwd_tail", "sed_adam_amsgrad_step"]
# the recurrent head's launches between the conv stack and the loss, and between the loss and the conv backward (engine.py)
GRU_FWD = ["sed_mel_mean_fwd", "sed_gemm_nt", "sed_gemm_nt", "sed_gru_pack_weights", "sed_gru_seq_fwd", "sed_head_fwd"]
GRU_BWD = ["sed_head_bwd", "sed_gru_seq_bwd", "sed_gemm_tn_batch", "sed_transpose_shift", "sed_transpose_shift", "sed_gemm_nt",
           "sed_mel_mean_bwd"]
SA_FWD = ["sed_mel_mean_fwd", "sed_gemm_nt", "sed_mhsa_fwd", "sed_gemm_nt", "sed_add_layernorm_fwd", "sed_head_fwd"]
SA_BWD = ["sed_head_bwd", "sed_add_layernorm_bwd", "sed_gemm_tn", "sed_transpose_shift", "sed_gemm_nt", "sed_mhsa_bwd", "sed_gemm_tn",
          "sed_transpose_shift", "sed_gemm_nt", "sed_mel_mean_bwd"]


def step_labels(sed, mdl):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 1, 32, 64, generator=g).cuda()
    y = torch.zeros(2, 32, 3, device="cuda")
    y[0, 4:13, 0] = 1.0
    tr = sed.FusedTrainer(mdl, lr=1e-3, recall_factor=W)
    tr.train_step(x, y)             # (first step: allocations)
    mdl.engine.timer = sed.engine.KernelTimer()
    tr.train_step(x, y)
    torch.cuda.synchronize()
    return [lbl.split(":")[0] for lbl, _, _ in mdl.engine.timer.records]


def test_other_models_launch_what_they_did(sed):
    torch.manual_seed(0)
    plain = step_labels(sed, sed.Cnn_AvgPooling(3, CFG, precision="bf16").cuda())
    assert plain == PLAIN_STEP
    h, b = PLAIN_STEP.index("sed_head_fwd"), PLAIN_STEP.index("sed_head_bwd")
    crnn = step_labels(sed, sed.Crnn_AvgPooling(3, CFG, precision="bf16", gru_hidden=32).cuda())
    print("crnn step:", crnn)
    assert crnn == PLAIN_STEP[:h] + GRU_FWD + PLAIN_STEP[h + 1:b] + GRU_BWD + PLAIN_STEP[b + 1:]
    assert not [n for n in plain + crnn if "mhsa" in n or "layernorm" in n]
    sa = step_labels(sed, sed.Csa_AvgPooling(3, CFG, precision="bf16", sa_heads=1).cuda())
    assert sa == PLAIN_STEP[:h] + SA_FWD + PLAIN_STEP[h + 1:b] + SA_BWD + PLAIN_STEP[b + 1:]
