"""GPU: Csa_AvgPooling with the Conformer convolution module (csrc/sed_convmod.hip) through the model, the engine, FusedTrainer and
infer.py, on the tiny configuration of tests/test_gpu_sa_model.py (t = 10 frames per clip: the 31-tap filter is wider than a clip).

fp32 parity as in that file: the conv-stack output of a head='none' engine on the same parameters is fed to the torch CPU oracle in
float64 -- per layer torch.nn.TransformerEncoderLayer's attention half (and FFN half), and between them nn.Conv1d / F.glu /
nn.BatchNorm1d / F.silu / nn.LayerNorm loaded through Csa_AvgPooling.conv_module_state -- + the linear layer + interpolate + the
weighted BCE, with autograd.  Bounds as there (tests/test_gpu_crnn.py's): fp32 logits 1e-3 absolute, loss 1e-4, every parameter
gradient 3e-3 relative L2.  Two things that bound does not define are set here by reasoning, not by what the code gives:
  - in training mode the gradient of depthwise.bias is zero in exact arithmetic (batch statistics remove a per-channel constant), so
    its relative error means nothing: both the oracle's and the model's must stay below 3e-3 of the L2 norm of the depthwise.weight
    gradient, which is formed from the same dz;
  - the running statistics after a step are means over R = 20 rows of an fp32 chain of a 32-term product and a k-term filter, a
    relative error of the order of 50 u = 3e-6: held to 1e-4 relative L2 against the oracle's BatchNorm buffers.
tests/test_gpu_sa_at_size.py calls compare and oracle at its own geometry (C = 128, t = 130, R = 520), with the same bounds."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import convmod_formula as V
import ffn_formula as F
import mhsa_formula as M
import test_gpu_sa_model as T0

pytestmark = pytest.mark.gpu
PKG = "soundeventdetection-pytorch_amd"
CFG, MEL, T, B, W = T0.CFG, T0.MEL, T0.T, T0.B, T0.W
C, D = CFG[-1][0], 64
rel_l2, batch, the_plan = T0.rel_l2, T0.batch, T0.the_plan
NEW = ["sed_dwconv_glu_fwd", "sed_bn_silu_fwd", "sed_bn_silu_bwd_reduce", "sed_dwconv_glu_bwd"]


@pytest.fixture(scope="module")
def sed():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)


def make_model(sed, K=3, precision="fp32", seed=0, layers=2, ffn=D, k=7, **kw):
    torch.manual_seed(seed)
    kw.setdefault("sa_heads", 1)
    m = sed.Csa_AvgPooling(K, CFG, precision=precision, mel_bins=MEL, sa_layers=layers, sa_ffn=ffn, sa_activation="gelu", sa_conv_kernel=k, **kw)
    with torch.no_grad():       # the zero / unit initial values would hide a wrong bias, affine or running-statistics path
        for n, p in m.named_parameters():
            if n.startswith(("attn", "ffn", "convm", "conv_norm")):
                if ("norm" in n or ".bn." in n) and n.endswith("weight"):
                    p.normal_(1.0, 0.2)
                elif n.endswith("bias"):
                    p.normal_(0.0, 0.1)
        for n, b in m.named_buffers():
            if n.startswith("convm") and n.endswith("running_mean"):
                b.normal_(0.0, 0.2)
            if n.startswith("convm") and n.endswith("running_var"):
                b.uniform_(0.5, 1.5)
    return m.cuda()


class ConvModule(torch.nn.Module):
    def __init__(self, Cc, k):
        super().__init__()
        self.pointwise1 = torch.nn.Conv1d(Cc, 2 * Cc, 1)
        self.depthwise = torch.nn.Conv1d(Cc, Cc, k, padding=(k - 1) // 2, groups=Cc)
        self.bn = torch.nn.BatchNorm1d(Cc)
        self.pointwise2 = torch.nn.Conv1d(Cc, Cc, 1)
        self.conv_norm = torch.nn.LayerNorm(Cc)

    def forward(self, h):
        x = TF.glu(self.pointwise1(h.transpose(1, 2)), dim=1)
        x = self.pointwise2(TF.silu(self.bn(self.depthwise(x))))
        return self.conv_norm(h + x.transpose(1, 2))


def oracle(sed, sd, feat, y, heads, layers, ffn, k, ratio, training=True, pos=True, act="gelu", plain_attention=False):
    """feat (B, t, Wf, C) float64 with requires_grad -> (logits, loss, parameter gradients by state_dict name, BatchNorm buffers).
    pos: the positional table; act: the FFN's activation; plain_attention (no FFN): the attention half from torch.nn.MultiheadAttention
    + LayerNorm as tests/test_gpu_sa_model.py's oracle_head builds it, not from a TransformerEncoderLayer with an unused FFN."""
    Cc = feat.shape[-1]
    cpu = lambda d: {n: (v.double() if v.is_floating_point() else v).cpu() for n, v in d.items()}
    enc, conv = [], []
    for l in range(layers):
        if plain_attention:
            assert not ffn
            an, nn_ = F.layer_names(l)[:2]
            e = torch.nn.Module()
            e.self_attn, e.norm1 = torch.nn.MultiheadAttention(Cc, heads, batch_first=True), torch.nn.LayerNorm(Cc)
            e.double()
            for mod, name in ((e.self_attn, an), (e.norm1, nn_)):
                mod.load_state_dict(cpu({n[len(name) + 1:]: v for n, v in sd.items() if n.startswith(name + ".")}))
        else:
            e = torch.nn.TransformerEncoderLayer(Cc, heads, max(ffn, 1), dropout=0.0, activation=act, batch_first=True, norm_first=False).double()
            e.load_state_dict(cpu(sed.Csa_AvgPooling.encoder_layer_state(sd, l)), strict=False)
        c = ConvModule(Cc, k).double()
        c.load_state_dict(cpu(sed.Csa_AvgPooling.conv_module_state(sd, l)))
        enc.append(e.train(training))
        conv.append(c.train(training))
    fc = torch.nn.Linear(Cc, sd["event_fc.weight"].shape[0]).double()
    fc.load_state_dict({n[len("event_fc."):]: v.double().cpu() for n, v in sd.items() if n.startswith("event_fc.")})
    m = feat.mean(dim=2)
    h = m + torch.from_numpy(M.positional_table(m.shape[1], Cc)).float().double() if pos else m      # the table as rounded to fp32
    for e, c in zip(enc, conv):
        h = e.norm1(h + e.self_attn(h, h, h, need_weights=False)[0])
        h = c(h)
        if ffn:
            h = e.norm2(h + e.linear2(getattr(TF, act)(e.linear1(h))))
    out = fc(h).repeat_interleave(ratio, dim=1)
    N = min(out.shape[1], y.shape[1])
    loss = TF.binary_cross_entropy_with_logits(out[:, :N], y[:, :N], pos_weight=torch.tensor(W, dtype=torch.float64))
    loss.backward()
    grads, bufs = {}, {}
    for l, (e, c) in enumerate(zip(enc, conv)):
        an, nn_, fn, fnn = F.layer_names(l)
        cm, cn = V.conv_names(l)
        back = {"self_attn": an, "norm1": nn_, "linear1": fn + ".linear1", "linear2": fn + ".linear2", "norm2": fnn}
        for n, p in e.named_parameters():
            top, rest = n.split(".", 1)
            if ffn or top in ("self_attn", "norm1"):
                grads[back[top] + "." + rest] = p.grad
        for n, p in c.named_parameters():
            grads[(cn + n[len("conv_norm"):]) if n.startswith("conv_norm") else cm + "." + n] = p.grad
        bufs[cm + ".bn.running_mean"], bufs[cm + ".bn.running_var"] = c.bn.running_mean.clone(), c.bn.running_var.clone()
    grads.update({"event_fc." + n: p.grad for n, p in fc.named_parameters()})
    return out.detach(), loss.detach(), grads, bufs


def compare(sed, model, x, y, layers, ffn, k, training, tag, cfg=CFG, mel=MEL, heads=1, **oracle_kw):
    """one forward + backward of the model against the oracle fed by a head='none' engine; -> (the bare engine, its plan, feat, P).
    cfg, mel, heads, oracle_kw: another geometry than this module's (tests/test_gpu_sa_at_size.py)"""
    K, C = y.shape[-1], cfg[-1][0]
    sd0 = {n: v.clone() for n, v in model.state_dict().items()}
    model.train(training)
    model.zero_grad()
    out = model(x)
    loss = sed.WeightedBCE(W, True)(out, y)
    loss.backward()
    plan = the_plan(model)
    assert plan.sa is not None and len(plan.sa["layers"]) == layers and "cz" in plan.sa["layers"][0]
    P = model._tensor_dict()
    bare = sed.CnnEngine(K, cfg, 1, "fp32", head="none", mel_bins=mel)
    P0 = {n: v.cuda() for n, v in sd0.items()}
    bp = bare.forward(x, P0, training=training, update_running_stats=False, keep_for_grad=not training)
    assert torch.equal(bp.y[-1], plan.y[-1])
    feat = bp.y[-1][..., :C].double().cpu().requires_grad_(True)
    out_t, loss_t, grads, bufs = oracle(sed, sd0, feat, y.double().cpu(), heads, layers, ffn, k, model.engine.ratio, training, **oracle_kw)
    err = float((out.detach().cpu().double() - out_t).abs().max())
    print(f"{tag}: logits max error {err:.3e}, loss error {abs(loss.item() - float(loss_t)):.3e}")
    assert err < 1e-3 and abs(loss.item() - float(loss_t)) < 1e-4
    mine = {n for n, _ in model.named_parameters() if not n.startswith("conv_blocks.")}
    assert mine == set(grads), mine ^ set(grads)
    for n, g in grads.items():
        got = model.get_parameter(n).grad
        if training and n.endswith("depthwise.bias"):
            scale = float(grads[n.replace(".bias", ".weight")].norm())
            print(f"  {n}: |got| / |d weight| {float(got.norm()) / scale:.3e}, oracle {float(g.norm()) / scale:.3e}")
            assert float(got.norm()) < 3e-3 * scale and float(g.norm()) < 3e-3 * scale, n
            continue
        l2 = rel_l2(got, g)
        print(f"  {n}: relative L2 {l2:.3e}")
        assert l2 < 3e-3, (n, l2)
    sd1 = model.state_dict()
    for n, b in bufs.items():
        nbt = n.replace("running_mean", "num_batches_tracked").replace("running_var", "num_batches_tracked")
        if training:
            l2 = rel_l2(sd1[n], b)
            print(f"  {n}: relative L2 {l2:.3e}")
            assert l2 < 1e-4, (n, l2)
            assert int(sd1[nbt]) == int(sd0[nbt]) + 1
        else:
            assert torch.equal(sd1[n], sd0[n]) and torch.equal(sd1[nbt], sd0[nbt]), (n, "an eval forward changed a running statistic")
    return bare, bp, feat, P0


@pytest.mark.parametrize("layers,ffn,k", [(2, D, 7), (1, 0, 31)])
def test_fp32_model_matches_the_torch_oracle(sed, layers, ffn, k):
    K = 3
    x, y = batch(K)
    model = make_model(sed, K, layers=layers, ffn=ffn, k=k)
    bare, bp, feat, P0 = compare(sed, model, x, y, layers, ffn, k, True, f"train layers={layers} ffn={ffn} k={k}")
    # the oracle's feature gradient back through the pinned conv backward
    bp.dy[-1].zero_()
    bp.dy[-1][..., :C] = feat.grad.float().cuda()
    names = [n for n, _ in model.named_parameters() if n.startswith("conv_blocks.")]
    G = {n: torch.full_like(P0[n], float("nan")) for n in names}
    bare.backward(bp, P0, G)
    for n in names:
        assert rel_l2(model.get_parameter(n).grad, G[n]) < 3e-3, n
    # the eval-mode forward and backward (running statistics, the frozen-BatchNorm backward) against the oracle in eval mode
    compare(sed, model, x, y, layers, ffn, k, False, f"eval layers={layers} ffn={ffn} k={k}")
    # the input gradient exists in both modes (need_dx)
    for training in (False, True):
        model.train(training)
        xg = x.clone().requires_grad_(True)
        model.zero_grad()
        model(xg).sum().backward()
        assert bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0, training
        assert float(model.get_parameter("convm.depthwise.weight").grad.abs().max()) > 0, training


@pytest.mark.parametrize("precision", ["bf16", "f16x3", "bf16x3"])
def test_other_precisions_follow_fp32(sed, precision):
    """Bounds as tests/test_gpu_sa_encoder.py has them for the two-layer stack with FFNs (0.3 relative L2 and 6e-2 in the loss for bf16,
    4e-2 and 6e-3 for the split-operand modes).  The module adds two bf16-operand products per layer to the about twenty roundings
    counted there (a tenth more); its vector launches are fp32 in every mode.  depthwise.bias is left out: its gradient is zero in
    exact arithmetic (module docstring)."""
    x, y = batch()
    ref, model = make_model(sed).train(), make_model(sed, precision=precision).train()
    lr = sed.WeightedBCE(W, True)(ref(x), y)
    lm = sed.WeightedBCE(W, True)(model(x), y)
    lr.backward()
    lm.backward()
    print(f"{precision}: loss difference {abs(lr.item() - lm.item()):.3e}")
    assert abs(lr.item() - lm.item()) < (6e-2 if precision == "bf16" else 6e-3)
    for (n, p), (_, q) in zip(ref.named_parameters(), model.named_parameters()):
        assert bool(torch.isfinite(q.grad).all()), n
        if n.startswith(("attn", "ffn", "event_fc", "convm", "conv_norm")) and not n.endswith("depthwise.bias"):
            print(f"  {n}: relative L2 {rel_l2(q.grad, p.grad):.3e}")
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
    sde, sdg = eager.model.state_dict(), graph.model.state_dict()
    for n in sde:
        if n.startswith("convm") and ".bn." in n:
            assert torch.equal(sde[n], sdg[n]), n
    assert int(sdg["convm_l1.bn.num_batches_tracked"]) == 4 and float((sdg["convm.bn.running_mean"]).abs().max()) > 0


def test_attention_pooling_mean_teacher_options_and_pcen(sed):
    x, y = batch()
    model = make_model(sed, attention=True)
    tr = sed.FusedTrainer(model, lr=1e-3, recall_factor=W, weak_pooling="att", weak_only=True)
    for v in tr.flat.G.values():
        v.fill_(float("nan"))
    tr.forward_backward(x, y)
    for n, g in tr.flat.G.items():
        assert bool(torch.isfinite(g).all()), n
        if n.startswith(("attn", "ffn", "att_fc.", "convm.pointwise", "convm.depthwise.weight", "conv_norm")):
            assert float(g.abs().max()) > 0, n
    tr.forward_backward(x, y, torch.tensor([1, 2], device="cuda"))          # label kinds
    for pooling in ("linear", "max", "mean"):
        lin = sed.FusedTrainer(make_model(sed), lr=1e-3, recall_factor=W, weak_pooling=pooling, weak_only=True)
        assert bool(torch.isfinite(lin.train_step(x, y)).all()), pooling
    mt = sed.FusedTrainer(make_model(sed), lr=1e-3, recall_factor=W, mean_teacher=True, consistency_weight=2.0)
    teacher = mt.teacher
    assert isinstance(teacher, sed.Csa_AvgPooling) and teacher.engine is not mt.model.engine and teacher.engine.sa_conv_kernel == 7
    before = mt.teacher_flat.P["convm_l1.depthwise.weight"].clone()
    rm0 = teacher.convm.bn.running_mean.clone()
    for _ in range(2):
        loss = mt.train_step(x, y)
    assert bool(torch.isfinite(loss).all()) and not torch.equal(before, mt.teacher_flat.P["convm_l1.depthwise.weight"])
    # the teacher's BatchNorm buffers follow its own forwards, the student's its own
    assert not torch.equal(rm0, teacher.convm.bn.running_mean) and teacher.convm.bn.running_mean is not mt.model.convm.bn.running_mean
    assert int(teacher.state_dict()["convm.bn.num_batches_tracked"]) == 2 == int(mt.model.state_dict()["convm.bn.num_batches_tracked"])
    opt = sed.FusedTrainer(make_model(sed), lr=1e-3, recall_factor=W, weight_decay=1e-2, decoupled_weight_decay=True, max_grad_norm=0.5)
    start = opt.flat.P["convm.pointwise1.weight"].clone()
    assert bool(torch.isfinite(opt.train_step(x, y)).all()) and not torch.equal(start, opt.flat.P["convm.pointwise1.weight"])
    fe = sed.PCEN(MEL, trainable=True)
    pt = sed.FusedTrainer(make_model(sed, frontend=fe), lr=1e-3, recall_factor=W)
    pt.train_step(x.abs() + 0.1, y)
    assert all(bool(torch.isfinite(v).all()) for v in pt.flat.G.values()) and float(pt.flat.G["convm.depthwise.weight"].abs().max()) > 0


def test_backward_completion_order_and_launch_labels(sed):
    x, y = batch()
    model = make_model(sed).train()
    eng, P = model.engine, model._tensor_dict()
    G = {n: torch.empty_like(p) for n, p in model.named_parameters()}
    eng.timer = sed.engine.KernelTimer()
    plan = eng.forward(x, P, training=True)
    eng.loss_and_grad(plan, y, W)
    done = []
    eng.backward(plan, P, G, on_group_done=done.append)
    torch.cuda.synchronize()
    assert done == ["event_fc", "ffn_norm_l1", "ffn_l1", "conv_norm_l1", "convm_l1", "attn_norm_l1", "attn_l1", "ffn_norm", "ffn",
                    "conv_norm", "convm", "attn_norm", "attn", "conv_blocks.1", "conv_blocks.0"]
    labels = [lbl for lbl, _, _ in eng.timer.records]
    for name in NEW:
        assert [l for l in labels if l.split(":")[0] == name] == [name + ":sa"] * 2, name
    # a k = 0 model records exactly the launch labels tests/test_gpu_sa_model.py lists
    torch.manual_seed(0)
    sa = T0.step_labels(sed, sed.Csa_AvgPooling(3, CFG, precision="bf16", sa_heads=1, sa_conv_kernel=0).cuda())
    h, b = T0.PLAIN_STEP.index("sed_head_fwd"), T0.PLAIN_STEP.index("sed_head_bwd")
    assert sa == T0.PLAIN_STEP[:h] + T0.SA_FWD + T0.PLAIN_STEP[h + 1:b] + T0.SA_BWD + T0.PLAIN_STEP[b + 1:]
    # with the module: its launches between the attention's LayerNorm and the head (forward), mirrored in the backward
    full = T0.step_labels(sed, sed.Csa_AvgPooling(3, CFG, precision="bf16", sa_heads=1, sa_conv_kernel=7).cuda())
    fwd = ["sed_gemm_nt", "sed_dwconv_glu_fwd", "sed_bn_train_finalize", "sed_bn_silu_fwd", "sed_gemm_nt", "sed_add_layernorm_fwd"]
    bwd = ["sed_add_layernorm_bwd", "sed_transpose_shift", "sed_gemm_nt", "sed_gemm_tn", "sed_bn_silu_bwd_reduce", "sed_bn_bwd_finalize",
           "sed_dwconv_glu_bwd", "sed_gemm_tn", "sed_transpose_shift", "sed_gemm_nt"]
    assert full == T0.PLAIN_STEP[:h] + T0.SA_FWD[:-1] + fwd + T0.SA_FWD[-1:] + T0.PLAIN_STEP[h + 1:b] + T0.SA_BWD[:1] + bwd + T0.SA_BWD[1:] + \
        T0.PLAIN_STEP[b + 1:]


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
                               sa_ffn=256, sa_activation="gelu", sa_conv_kernel=15, attention=True)
    with torch.no_grad():
        model.convm.bn.running_mean.normal_(0.0, 0.2)
        model.convm_l1.bn.running_var.uniform_(0.5, 1.5)
    ck = str(tmp_path / "m.pth")
    torch.save({"iterations": 0, "model": model.state_dict()}, ck)
    res = infer.infer_file(p, ck, precision="fp32", cfg=sc.BENCH, clip_pooling="att", saliency=True)
    model = model.cuda().eval()
    with torch.no_grad():
        probs = torch.sigmoid(model(torch.from_numpy(res["log_mel"]).cuda()[None, None]))[0]
    assert np.array_equal(res["probabilities"], probs.cpu().numpy()), "the rebuilt model gives other bits"
    assert "clip_probs" in res and np.isfinite(res["saliency"]).all()
