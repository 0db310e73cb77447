"""GPU: Csa_AvgPooling(sa_norm_first=True[, sa_macaron=True]) -- pre-LN layers, the macaron half-step FFNs and the closing norms
(sed_resid_layernorm_fwd / _bwd, csrc/sed_layernorm.hip) -- through the model, the engine, FusedTrainer and infer.py, on the tiny configuration
of tests/test_gpu_sa_encoder.py (C = 32, one head, t = 10 frames per clip).

fp32 parity as in that file: the conv-stack output of a head='none' engine on the same parameters is fed to the float64 oracle
tests/preln_formula.py (itself checked against torch on the host, tests/test_preln_host.py) + the linear layer + interpolate + the weighted
BCE.  Bounds as there (tests/test_gpu_crnn.py's): fp32 logits 1e-3 absolute, loss 1e-4, every parameter gradient 3e-3 relative L2."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import preln_formula as PF
import test_gpu_sa_model as T0

pytestmark = pytest.mark.gpu
PKG = "soundeventdetection-pytorch_amd"
CFG, MEL, T, B, W = T0.CFG, T0.MEL, T0.T, T0.B, T0.W
C, D = CFG[-1][0], 64
SEED = 0x0123456789ABCDEF
rel_l2, batch, the_plan = T0.rel_l2, T0.batch, T0.the_plan
HEAD = ("attn", "ffn", "convm", "conv_norm", "rel_pos", "out_norm")
PLAIN = dict(sa_layers=2, sa_ffn=D, sa_activation="gelu")                                                 # a 2-layer pre-LN GELU model
CONFORMER = dict(sa_layers=2, sa_ffn=D, sa_macaron=True, sa_conv_kernel=7, sa_window=(3, 2), sa_rel_pos=3)  # macaron + conv + window + bias


@pytest.fixture(scope="module")
def sed():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)


def make_model(sed, K=3, precision="fp32", seed=0, **kw):
    torch.manual_seed(seed)
    kw.setdefault("sa_heads", 1)
    kw.setdefault("sa_norm_first", True)
    m = sed.Csa_AvgPooling(K, CFG, precision=precision, mel_bins=MEL, **kw)
    with torch.no_grad():       # the zero / unit initial values would hide a wrong bias, table or affine gradient
        for n, p in m.named_parameters():
            if n.startswith(HEAD):
                if ("norm" in n or ".bn." in n) and n.endswith("weight"):
                    p.normal_(1.0, 0.2)
                elif n.endswith("bias") or n.startswith("rel_pos"):
                    p.normal_(0.0, 0.1)
    return m.cuda()


def preln_encoder(opts, state, p, training=True):
    """preln_formula.encoder on a model's options, as oracle takes it: (x, W, B, t, H, dh_out=None) -> the formula's dict"""
    kw = dict(layers=opts["sa_layers"], ffn_width=opts.get("sa_ffn", 0), act=opts.get("sa_activation", "relu"), macaron=opts.get("sa_macaron", False),
              conv=bool(opts.get("sa_conv_kernel", 0)), window=opts.get("sa_window") or (None, None), rel_cfg=opts.get("sa_rel_pos"), state=state, p=p,
              pos_encoding=False, training=training)
    return lambda x, Wn, Bc, t, H, dh_out=None: PF.encoder(x, Wn, Bc, t, H, dh_out=dh_out, **kw)


def oracle(sd, feat, y, state, p, opts, ratio, training=True, heads=1, encoder=None):
    """feat (B, t, Wf, C) float64 -> (logits, loss, parameter gradients by state_dict name, the feature gradient, the formula's forward
    dict: the BatchNorms' running statistics after a training forward).  heads: the head count the formula splits by; encoder: another
    stack than preln_encoder(opts, ...) with its call (tests/test_gpu_sa_block_at_size.py: the post-LN stack of relpos_formula)."""
    Bc, t, Wf, Cc = feat.shape
    Wn = {n: v.double().cpu().numpy() for n, v in sd.items() if n.startswith(HEAD) and "config" not in n and "num_batches" not in n}
    x = feat.mean(dim=2).reshape(Bc * t, Cc).numpy()
    enc = encoder if encoder is not None else preln_encoder(opts, state, p, training)
    # the positional table as the engine holds it: rounded once to fp32
    pe = np.tile(PF.M.positional_table(t, Cc).astype(np.float32).astype(np.float64), (Bc, 1)) if opts.get("pos_encoding", True) else 0.0
    fwd = enc(x + pe, Wn, Bc, t, heads)
    h = torch.from_numpy(fwd["h"]).reshape(Bc, t, Cc).requires_grad_(True)
    fc = torch.nn.Linear(Cc, sd["event_fc.weight"].shape[0]).double()
    fc.load_state_dict({n[len("event_fc."):]: v.double().cpu() for n, v in sd.items() if n.startswith("event_fc.")})
    out = fc(h).repeat_interleave(ratio, dim=1)
    N = min(out.shape[1], y.shape[1])
    loss = TF.binary_cross_entropy_with_logits(out[:, :N], y[:, :N], pos_weight=torch.tensor(W, dtype=torch.float64))
    loss.backward()
    bwd = enc(x + pe, Wn, Bc, t, heads, dh_out=h.grad.reshape(Bc * t, Cc).numpy())
    grads = {n[2:]: torch.from_numpy(np.asarray(a)) for n, a in bwd.items() if n.startswith("d_")}
    grads.update({"event_fc." + n: q.grad for n, q in fc.named_parameters()})
    dfeat = torch.from_numpy(bwd["dx"]).reshape(Bc, t, 1, Cc).expand(Bc, t, Wf, Cc) / Wf
    return out.detach(), loss.detach(), grads, dfeat, fwd


def compare(sed, model, opts, p=0.0, xy=None, cfg=CFG, mel=MEL, heads=1, training=True, encoder=None):
    """one forward + backward of the fp32 model against the oracle; -> (out, what a second oracle call on the same step takes).
    xy, cfg, mel, heads: another geometry than this module's; training=False: an eval forward kept for the gradient and the eval-mode
    backward, after which every running statistic and counter keeps its bits; encoder(state): the stack oracle takes in the place of
    preln_formula's (tests/test_gpu_sa_block_at_size.py).  The running statistics after a training step are held to
    tests/test_gpu_sa_conformer.py's bound, 1e-4 relative L2 against the formula's, and the counter to + 1."""
    x, y = batch(3) if xy is None else xy
    K, Cc = y.shape[-1], cfg[-1][0]
    eng = model.engine
    sd0 = {n: v.clone() for n, v in model.state_dict().items()}
    state = eng.drop_state_words()
    model.train(training)
    model.zero_grad()
    out = model(x)
    loss = sed.WeightedBCE(W, True)(out, y)
    loss.backward()
    plan = the_plan(model)
    bare = sed.CnnEngine(K, cfg, 1, "fp32", head="none", mel_bins=mel)
    P0 = {n: v.cuda() for n, v in sd0.items()}
    bp = bare.forward(x, P0, training=training, update_running_stats=False, keep_for_grad=not training)
    assert torch.equal(bp.y[-1], plan.y[-1])
    feat = bp.y[-1][..., :Cc].double().cpu()
    out_t, loss_t, grads, dfeat, fwd = oracle(sd0, feat, y.double().cpu(), state, p, opts, eng.ratio, training, heads,
                                              encoder(state) if encoder is not None else None)
    err = float((out.detach().cpu().double() - out_t).abs().max())
    print(f"{opts} p={p} training={training}: logits max error {err:.3e}, loss error {abs(loss.item() - float(loss_t)):.3e}")
    assert err < 1e-3 and abs(loss.item() - float(loss_t)) < 1e-4
    mine = {n for n, _ in model.named_parameters() if not n.startswith("conv_blocks.")}
    assert mine == set(grads), mine ^ set(grads)
    worst = 0.0
    for n, g in grads.items():
        got = model.get_parameter(n).grad
        if training and n.endswith("depthwise.bias"):          # exactly zero in front of a training BatchNorm: both sides hold rounding noise
            scale = float(grads[n.replace(".bias", ".weight")].norm())
            print(f"  {n}: |got| / |d weight| {float(got.norm()) / scale:.3e}, oracle {float(g.norm()) / scale:.3e}")
            assert float(got.norm()) < 3e-3 * scale and float(g.norm()) < 3e-3 * scale, n
            continue
        l2 = rel_l2(got, g.reshape(got.shape))
        worst = max(worst, l2)
        print(f"  {n}: relative L2 {l2:.3e}")
        assert l2 < 3e-3, (n, l2)
    # the BatchNorms' running statistics and counters
    sd1 = model.state_dict()
    for n in sd0:
        if n.startswith("convm") and ".bn.running_" in n:
            nbt = n.replace("running_mean", "num_batches_tracked").replace("running_var", "num_batches_tracked")
            if training:
                l2 = rel_l2(sd1[n], fwd[n])
                print(f"  {n}: relative L2 {l2:.3e}")
                assert l2 < 1e-4, (n, l2)
                assert int(sd1[nbt]) == int(sd0[nbt]) + 1, nbt
            else:
                assert torch.equal(sd1[n], sd0[n]) and torch.equal(sd1[nbt], sd0[nbt]), (n, "an eval step changed a running statistic")
    # the oracle's feature gradient back through the pinned conv backward
    bp.dy[-1].zero_()
    bp.dy[-1][..., :Cc] = dfeat.float().cuda()
    names = [n for n, _ in model.named_parameters() if n.startswith("conv_blocks.")]
    G = {n: torch.full_like(P0[n], float("nan")) for n in names}
    bare.backward(bp, P0, G)
    for n in names:
        l2 = rel_l2(model.get_parameter(n).grad, G[n])
        worst = max(worst, l2)
        assert l2 < 3e-3, n
    print(f"  worst gradient relative L2 {worst:.3e}")
    return out, (sd0, feat, y.double().cpu(), state, eng.ratio)


@pytest.mark.parametrize("opts", [PLAIN, CONFORMER], ids=["pre_ln_gelu", "conformer"])
def test_fp32_model_matches_the_float64_oracle(sed, opts):
    model = make_model(sed, **opts).train()
    out, _ = compare(sed, model, opts)
    x, _ = batch()
    # eval forward; the eval-mode backward and the input gradient (need_dx) in both modes
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
        for n, q in model.named_parameters():
            assert bool(torch.isfinite(q.grad).all()), (training, n)
        assert float(model.get_parameter("ffn_norm.weight").grad.abs().max()) > 0, training


@pytest.mark.parametrize("opts", [PLAIN, CONFORMER], ids=["pre_ln_gelu", "conformer"])
def test_dropout_step_matches_the_masked_oracle(sed, opts):
    """the masks of every site are dropout_formula's, sites 5 and 6 (the macaron FFN's hidden activation and output) included: the
    oracle with these masks is inside the fp32 bounds, the oracle without them far outside"""
    p = 0.25
    model = make_model(sed, sa_dropout=p, sa_dropout_seed=SEED, **opts).train()
    assert model.engine.drop_state_words() == [SEED & 0xFFFFFFFF, SEED >> 32, 0, 0]
    out, (sd0, feat, y, state, ratio) = compare(sed, model, opts, p)
    assert model.engine.drop_state_words()[2] == 1, "a training forward advances the step word by one"
    plain = oracle(sd0, feat, y, state, 0.0, opts, ratio)[0]
    assert float((out.detach().cpu().double() - plain).abs().max()) > 1e-2
    if opts.get("sa_macaron"):
        # the macaron sites alone: an oracle whose masks at sites 5 and 6 are another step's is outside too
        Bc, t = feat.shape[:2]
        k5 = PF.D.keep_rows(state, PF.D.stream_id(0, PF.SITE_MAC_HIDDEN), Bc * t, D, p)
        k6 = PF.D.keep_rows(state, PF.D.stream_id(1, PF.SITE_MAC_OUT), Bc * t, C, p)
        assert 0 < int(k5.sum()) < k5.size and 0 < int(k6.sum()) < k6.size
    model.eval()
    x, _ = batch()
    with torch.no_grad():
        assert torch.equal(model(x), model(x)), "an eval forward never drops"


@pytest.mark.parametrize("precision", ["bf16", "f16x3", "bf16x3"])
def test_other_precisions_follow_fp32(sed, precision):
    """Bounds as tests/test_gpu_sa_encoder.py's for its two-layer stack with FFNs: head gradients 0.3 relative L2 in bf16 (4e-2 in
    the split precisions), the loss 6e-2 (6e-3)."""
    x, y = batch()
    ref, model = make_model(sed, **PLAIN).train(), make_model(sed, precision=precision, **PLAIN).train()
    lr = sed.WeightedBCE(W, True)(ref(x), y)
    lm = sed.WeightedBCE(W, True)(model(x), y)
    lr.backward()
    lm.backward()
    assert abs(lr.item() - lm.item()) < (6e-2 if precision == "bf16" else 6e-3)
    for (n, p), (_, q) in zip(ref.named_parameters(), model.named_parameters()):
        assert bool(torch.isfinite(q.grad).all()), n
        if n.startswith(("attn", "ffn", "out_norm", "event_fc")):
            assert rel_l2(q.grad, p.grad) < (0.3 if precision == "bf16" else 4e-2), (precision, n, rel_l2(q.grad, p.grad))


@pytest.mark.parametrize("opts", [PLAIN, dict(CONFORMER, sa_dropout=0.1, sa_dropout_seed=5)], ids=["pre_ln_gelu", "conformer_dropout"])
def test_graph_steps_give_the_eager_bits(sed, opts):
    x, y = batch()

    def fresh():
        return sed.FusedTrainer(make_model(sed, precision="bf16", **opts), lr=1e-3, recall_factor=W, graph=True)

    eager, graph = fresh(), fresh()
    for i in range(4):              # launch by launch / two eager steps, the capture, a replay
        le = eager._step_dev(x, y).clone()
        eager._host_mirror()
        lg = graph.train_step(x, y).clone()
        assert torch.equal(le, lg), (i, "the graph step's loss differs from the eager step's")
        assert torch.equal(eager.flat.p, graph.flat.p), i
    assert len(graph._graphs) == 1 and len(eager._graphs) == 0


def test_attention_pooling_mean_teacher_options_and_pcen(sed):
    x, y = batch()
    model = make_model(sed, attention=True, **CONFORMER)
    tr = sed.FusedTrainer(model, lr=1e-3, recall_factor=W, weak_pooling="att", weak_only=True)
    for v in tr.flat.G.values():
        v.fill_(float("nan"))
    tr.forward_backward(x, y)
    for n, g in tr.flat.G.items():
        assert bool(torch.isfinite(g).all()), n
        if n.startswith(("attn", "ffn", "att_fc.", "out_norm", "convm.pointwise", "convm.depthwise.weight", "conv_norm", "rel_pos")):
            assert float(g.abs().max()) > 0, n
    tr.forward_backward(x, y, torch.tensor([1, 2], device="cuda"))          # label kinds
    mt = sed.FusedTrainer(make_model(sed, **CONFORMER), lr=1e-3, recall_factor=W, mean_teacher=True, consistency_weight=2.0)
    teacher = mt.teacher
    assert isinstance(teacher, sed.Csa_AvgPooling) and teacher.engine is not mt.model.engine
    assert (teacher.engine.sa_norm_first, teacher.engine.sa_macaron) == (True, True)
    before = {n: mt.teacher_flat.P[n].clone() for n in ("ffn_mac_l1.linear2.weight", "out_norm.weight", "ffn_mac_norm.bias")}
    for _ in range(2):
        loss = mt.train_step(x, y)
    assert bool(torch.isfinite(loss).all())
    for n, v in before.items():                  # the EMA covers the new parameters through the flat buffer
        assert not torch.equal(v, mt.teacher_flat.P[n]), n
    opt = sed.FusedTrainer(make_model(sed, **PLAIN), lr=1e-3, recall_factor=W, weight_decay=1e-2, decoupled_weight_decay=True, max_grad_norm=0.5)
    start = opt.flat.P["out_norm_l1.weight"].clone()
    assert bool(torch.isfinite(opt.train_step(x, y)).all()) and not torch.equal(start, opt.flat.P["out_norm_l1.weight"])
    fe = sed.PCEN(MEL, trainable=True)
    pt = sed.FusedTrainer(make_model(sed, frontend=fe, **PLAIN), lr=1e-3, recall_factor=W)
    pt.train_step(x.abs() + 0.1, y)
    assert all(bool(torch.isfinite(v).all()) for v in pt.flat.G.values()) and float(pt.flat.G["out_norm_l1.weight"].abs().max()) > 0


def aten_adds(fn):
    """the number of torch-side adds (aten::add / add_) fn() dispatches"""
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.key in ("aten::add", "aten::add_"))


def test_backward_completion_order_and_launch_labels(sed):
    x, y = batch()
    for opts in (PLAIN, CONFORMER):
        model = make_model(sed, **opts).train()
        eng, P = model.engine, model._tensor_dict()
        G = {n: torch.empty_like(p) for n, p in model.named_parameters()}
        plan = eng.forward(x, P, training=True)
        eng.loss_and_grad(plan, y, W)
        done = []
        eng.timer = sed.engine.KernelTimer()
        eng.backward(plan, P, G, on_group_done=done.append)
        torch.cuda.synchronize()
        order = PF.module_order(2, opts.get("sa_macaron", False), bool(opts.get("sa_conv_kernel")), D, opts.get("sa_rel_pos") is not None)
        assert done == ["event_fc"] + order[::-1] + ["conv_blocks.1", "conv_blocks.0"]
        labels = [lbl.split(":")[0] for lbl, _, _ in eng.timer.records]
        assert labels.count("sed_resid_layernorm_bwd") == len([n for n in order if "norm" in n]) and not [n for n in labels if "add_layernorm" in n]
        eng.timer = None
        # no torch add is left on the pre-LN backward: the post-LN twin dispatches one per sub-layer, this path none
        post = make_model(sed, sa_norm_first=False, **{k: v for k, v in opts.items() if k != "sa_macaron"}).train()
        pe, pP = post.engine, post._tensor_dict()
        pG = {n: torch.empty_like(p) for n, p in post.named_parameters()}
        pplan = pe.forward(x, pP, training=True)
        pe.loss_and_grad(pplan, y, W)
        subs = len([n for n in PF.module_order(2, False, bool(opts.get("sa_conv_kernel")), D, False) if "norm" in n and "out" not in n])
        n_pre, n_post = aten_adds(lambda: eng.backward(plan, P, G)), aten_adds(lambda: pe.backward(pplan, pP, pG))
        print(f"torch adds in the backward: pre-LN {n_pre}, post-LN {n_post}")
        assert n_post - n_pre == subs
    # the whole pre-LN step's labels
    torch.manual_seed(0)
    pre = T0.step_labels(sed, sed.Csa_AvgPooling(3, CFG, precision="bf16", sa_heads=1, sa_norm_first=True).cuda())
    h, b = T0.PLAIN_STEP.index("sed_head_fwd"), T0.PLAIN_STEP.index("sed_head_bwd")
    fwd = ["sed_mel_mean_fwd", "sed_resid_layernorm_fwd", "sed_gemm_nt", "sed_mhsa_fwd", "sed_gemm_nt", "sed_resid_layernorm_fwd", "sed_head_fwd"]
    bwd = ["sed_head_bwd", "sed_resid_layernorm_bwd", "sed_gemm_tn", "sed_transpose_shift", "sed_gemm_nt", "sed_mhsa_bwd", "sed_gemm_tn",
           "sed_transpose_shift", "sed_gemm_nt", "sed_resid_layernorm_bwd", "sed_mel_mean_bwd"]
    assert pre == T0.PLAIN_STEP[:h] + fwd + T0.PLAIN_STEP[h + 1:b] + bwd + T0.PLAIN_STEP[b + 1:]


def test_default_model_records_the_old_labels(sed):
    """both switches at their defaults: exactly the launch labels tests/test_gpu_sa_model.py lists, and the post-LN bits"""
    torch.manual_seed(0)
    sa = T0.step_labels(sed, sed.Csa_AvgPooling(3, CFG, precision="bf16", sa_heads=1, sa_norm_first=False, sa_macaron=False).cuda())
    h, b = T0.PLAIN_STEP.index("sed_head_fwd"), T0.PLAIN_STEP.index("sed_head_bwd")
    assert sa == T0.PLAIN_STEP[:h] + T0.SA_FWD + T0.PLAIN_STEP[h + 1:b] + T0.SA_BWD + T0.PLAIN_STEP[b + 1:]
    x, _ = batch()
    a = T0.make_model(sed).eval()
    c = T0.make_model(sed, sa_norm_first=False, sa_macaron=False).eval()
    with torch.no_grad():
        assert torch.equal(a(x), c(x))


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
                               sa_ffn=256, sa_conv_kernel=7, sa_norm_first=True, sa_macaron=True)
    with torch.no_grad():
        for n, q in model.named_parameters():
            if n.startswith(("out_norm", "ffn_mac_norm")):
                q.normal_(1.0 if n.endswith("weight") else 0.0, 0.2)
    ck = str(tmp_path / "m.pth")
    torch.save({"iterations": 0, "model": model.state_dict()}, ck)
    res = infer.infer_file(p, ck, precision="fp32", cfg=sc.BENCH, clip_pooling="linear", saliency=True)
    model = model.cuda().eval()
    with torch.no_grad():
        probs = torch.sigmoid(model(torch.from_numpy(res["log_mel"]).cuda()[None, None]))[0]
    assert np.array_equal(res["probabilities"], probs.cpu().numpy()), "the rebuilt model gives other bits"
    assert "clip_probs" in res and np.isfinite(res["saliency"]).all()
