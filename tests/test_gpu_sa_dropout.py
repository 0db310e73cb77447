"""GPU: Csa_AvgPooling(sa_dropout=p) through the model, the engine and FusedTrainer, on the tiny configuration of
tests/test_gpu_sa_conformer.py.  The oracle is the masked float64 stack of tests/dropout_formula.py (encoder) fed by a head='none'
engine on the same parameters, with the masks of the state read off engine.drop_state BEFORE the forward, + the linear layer +
interpolate + the weighted BCE.  Bounds as the sibling tests' (tests/test_gpu_crnn.py's): fp32 logits 1e-3 absolute, every parameter
gradient 3e-3 relative L2; depthwise.bias as tests/test_gpu_sa_conformer.py argues (zero in exact arithmetic: held to 3e-3 of the
depthwise.weight gradient's norm)."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import dropout_formula as DF
import test_gpu_sa_conformer as T1
import test_gpu_sa_model as T0

pytestmark = pytest.mark.gpu
PKG = "soundeventdetection-pytorch_amd"
CFG, MEL, W = T0.CFG, T0.MEL, T0.W
C, D = CFG[-1][0], 64
rel_l2, batch, the_plan = T0.rel_l2, T0.batch, T0.the_plan
SEED = 0x00C0FFEE5EDD0001


@pytest.fixture(scope="module")
def sed():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)


def make_model(sed, p, K=3, precision="fp32", layers=2, ffn=D, k=7, seed=SEED, **kw):
    return T1.make_model(sed, K, precision, layers=layers, ffn=ffn, k=k, sa_dropout=p, sa_dropout_seed=seed, **kw)


def oracle(sd, feat, y, state, p, heads, layers, ffn, conv, ratio):
    """feat (B, t, Wf, C) float64 -> logits, loss, gradients by state_dict name, the feature gradient"""
    Bc, t, Wf, Cc = feat.shape
    Wn = {n: v.double().cpu().numpy() for n, v in sd.items() if v.is_floating_point()}
    x = feat.mean(dim=2).reshape(Bc * t, Cc).numpy()
    kw = dict(layers=layers, ffn_width=ffn, act="gelu", pos_encoding=True, conv=conv)
    Wn_pe = dict(Wn)
    fwd = DF.encoder(x, Wn_pe, Bc, t, heads, state, p, **kw)
    h = torch.from_numpy(fwd["h"]).reshape(Bc, t, Cc).requires_grad_(True)
    fc = torch.nn.Linear(Cc, sd["event_fc.weight"].shape[0]).double()
    fc.load_state_dict({n[len("event_fc."):]: v.double().cpu() for n, v in sd.items() if n.startswith("event_fc.")})
    out = fc(h).repeat_interleave(ratio, dim=1)
    N = min(out.shape[1], y.shape[1])
    loss = TF.binary_cross_entropy_with_logits(out[:, :N], y[:, :N], pos_weight=torch.tensor(W, dtype=torch.float64))
    loss.backward()
    bwd = DF.encoder(x, Wn_pe, Bc, t, heads, state, p, dh_out=h.grad.reshape(Bc * t, Cc).numpy(), **kw)
    grads = {n[2:]: torch.from_numpy(np.asarray(a)) for n, a in bwd.items() if n.startswith("d_")}
    grads.update({"event_fc." + n: q.grad for n, q in fc.named_parameters()})
    dfeat = torch.from_numpy(bwd["dx"]).reshape(Bc, t, 1, Cc).expand(Bc, t, Wf, Cc) / Wf
    return out.detach(), loss.detach(), grads, dfeat


@pytest.mark.parametrize("layers,ffn,k,p", [(2, D, 7, 0.1), (1, 0, 0, 0.5)])
def test_fp32_model_matches_the_masked_oracle(sed, layers, ffn, k, p):
    K = 3
    x, y = batch(K)
    model = make_model(sed, p, K, layers=layers, ffn=ffn, k=k).train()
    eng = model.engine
    sd0 = {n: v.clone() for n, v in model.state_dict().items()}
    state = eng.drop_state_words()
    assert state == [SEED & 0xFFFFFFFF, SEED >> 32, 0, 0]
    model.zero_grad()
    out = model(x)
    loss = sed.WeightedBCE(W, True)(out, y)
    loss.backward()
    assert eng.drop_state_words() == state[:2] + [1, 0], "a training forward advances the step word by one"
    plan = the_plan(model)
    bare = sed.CnnEngine(K, CFG, 1, "fp32", head="none", mel_bins=MEL)
    P0 = {n: v.cuda() for n, v in sd0.items()}
    bp = bare.forward(x, P0, training=True, update_running_stats=False)
    assert torch.equal(bp.y[-1], plan.y[-1])
    feat = bp.y[-1][..., :C].double().cpu()
    out_t, loss_t, grads, dfeat = oracle(sd0, feat, y.double().cpu(), state, p, 1, layers, ffn, bool(k), eng.ratio)
    err = float((out.detach().cpu().double() - out_t).abs().max())
    print(f"p={p} layers={layers}: logits max error {err:.3e}, loss error {abs(loss.item() - float(loss_t)):.3e}")
    assert err < 1e-3 and abs(loss.item() - float(loss_t)) < 1e-4
    mine = {n for n, _ in model.named_parameters() if not n.startswith("conv_blocks.")}
    assert mine == set(grads), mine ^ set(grads)
    for n, g in grads.items():
        got = model.get_parameter(n).grad
        if n.endswith("depthwise.bias"):
            scale = float(grads[n.replace(".bias", ".weight")].norm())
            assert float(got.norm()) < 3e-3 * scale and float(g.norm()) < 3e-3 * scale, n
            continue
        l2 = rel_l2(got, g.reshape(got.shape))
        print(f"  {n}: relative L2 {l2:.3e}")
        assert l2 < 3e-3, (n, l2)
    # the oracle's feature gradient back through the pinned conv backward
    bp.dy[-1].zero_()
    bp.dy[-1][..., :C] = dfeat.float().cuda()
    names = [n for n, _ in model.named_parameters() if n.startswith("conv_blocks.")]
    G = {n: torch.full_like(P0[n], float("nan")) for n in names}
    bare.backward(bp, P0, G)
    for n in names:
        assert rel_l2(model.get_parameter(n).grad, G[n]) < 3e-3, n
    # the oracle without the masks is somewhere else: the bound sees the dropout
    plain = oracle(sd0, feat, y.double().cpu(), state, 0.0, 1, layers, ffn, bool(k), eng.ratio)[0]
    assert float((out.detach().cpu().double() - plain).abs().max()) > 1e-2


@pytest.mark.parametrize("precision", ["bf16", "f16x3", "bf16x3"])
def test_other_precisions_run_and_stay_finite(sed, precision):
    x, y = batch()
    model = make_model(sed, 0.1, precision=precision).train()
    loss = sed.WeightedBCE(W, True)(model(x), y)
    loss.backward()
    assert bool(torch.isfinite(loss).all())
    for n, q in model.named_parameters():
        assert bool(torch.isfinite(q.grad).all()), n
        if n.startswith(("attn", "ffn", "convm.pointwise", "conv_norm", "event_fc")):
            assert float(q.grad.abs().max()) > 0, n


def test_eval_never_drops_and_training_forwards_differ(sed):
    x, _ = batch()
    drop, plain = make_model(sed, 0.5), make_model(sed, 0.0)
    assert list(drop.state_dict()) == list(plain.state_dict())
    plain.load_state_dict(drop.state_dict())
    drop.eval(), plain.eval()
    with torch.no_grad():
        assert torch.equal(drop(x), plain(x)), "an eval forward of a p > 0 model must give the p = 0 model's bits"
    assert drop.engine.drop_state_words()[2] == 0, "an eval forward does not advance the step word"
    # the eval-mode backward does not drop either
    for m in (drop, plain):
        m.zero_grad()
        m(x).sum().backward()
    for (n, a), (_, b) in zip(drop.named_parameters(), plain.named_parameters()):
        assert torch.equal(a.grad, b.grad), n
    assert drop.engine.drop_state_words()[2] == 0
    drop.train()
    with torch.no_grad():
        a = drop(x).clone()
        b = drop(x).clone()
    assert not torch.equal(a, b), "two training forwards draw different masks"
    assert drop.engine.drop_state_words()[2] == 2
    # the same state gives the same bits
    drop.engine.set_drop_state(drop.engine.drop_state_words()[:2] + [0, 0])
    with torch.no_grad():
        assert torch.equal(drop(x), a)


def test_graph_steps_give_the_eager_bits_and_the_state_round_trips(sed):
    x, y = batch()

    def fresh():
        return sed.FusedTrainer(make_model(sed, 0.1, precision="bf16"), lr=1e-3, recall_factor=W, graph=True)

    eager, graph = fresh(), fresh()
    for i in range(4):              # launch by launch / two eager steps, the capture, a replay
        le = eager._step_dev(x, y).clone()
        eager._host_mirror()
        lg = graph.train_step(x, y).clone()
        assert torch.equal(le, lg), (i, "the graph step's loss differs from the eager step's")
        assert torch.equal(eager.flat.p, graph.flat.p), i
        assert torch.equal(eager.engine.drop_state, graph.engine.drop_state), i
    assert graph.engine.drop_state_words()[2] == 4, "a replay advances the step word like an eager step"
    sde, sdg = eager.model.state_dict(), graph.model.state_dict()
    for n in sde:
        assert torch.equal(sde[n], sdg[n]), n
    # trainer.state_dict() carries the state; a state without it starts at step 0
    sd = graph.state_dict()
    assert sd["dropout_state"].tolist() == graph.engine.drop_state_words()
    other = fresh()
    other.load_state_dict(sd)
    assert other.engine.drop_state_words() == graph.engine.drop_state_words()
    other.model.load_state_dict(graph.model.state_dict())
    la, lb = graph.train_step(x, y).clone(), other.train_step(x, y).clone()
    assert torch.equal(la, lb), "a resumed trainer draws the masks the original draws next"
    del sd["dropout_state"]
    other.load_state_dict(sd)
    assert other.engine.drop_state_words() == [SEED & 0xFFFFFFFF, SEED >> 32, 0, 0]
    # a p = 0 trainer's state has no such key
    assert "dropout_state" not in sed.FusedTrainer(make_model(sed, 0.0), lr=1e-3, recall_factor=W).state_dict()


def test_options_take_a_step(sed):
    x, y = batch()
    tr = sed.FusedTrainer(make_model(sed, 0.1, attention=True), lr=1e-3, recall_factor=W, weak_pooling="att", weak_only=True)
    for v in tr.flat.G.values():
        v.fill_(float("nan"))
    tr.forward_backward(x, y)
    assert all(bool(torch.isfinite(g).all()) for g in tr.flat.G.values())
    tr.forward_backward(x, y, torch.tensor([1, 2], device="cuda"))          # label kinds
    assert all(bool(torch.isfinite(g).all()) for g in tr.flat.G.values())
    mt = sed.FusedTrainer(make_model(sed, 0.1), lr=1e-3, recall_factor=W, mean_teacher=True, consistency_weight=2.0)
    ts, ss = mt.teacher.engine.drop_state_words(), mt.engine.drop_state_words()
    seed_t = SEED ^ sed.train.TEACHER_DROPOUT_SEED_XOR
    assert ts == [seed_t & 0xFFFFFFFF, seed_t >> 32, 0, 0] and ts[:2] != ss[:2], "the teacher draws masks of its own"
    for _ in range(2):
        loss = mt.train_step(x, y)
    assert bool(torch.isfinite(loss).all())
    assert mt.teacher.engine.drop_state_words()[2] == 2 == mt.engine.drop_state_words()[2]
    sd = mt.state_dict()
    assert sd["teacher_dropout_state"].tolist() == mt.teacher.engine.drop_state_words()
    opt = sed.FusedTrainer(make_model(sed, 0.1), lr=1e-3, recall_factor=W, weight_decay=1e-2, decoupled_weight_decay=True, max_grad_norm=0.5)
    assert bool(torch.isfinite(opt.train_step(x, y)).all())
    fe = sed.PCEN(MEL, trainable=True)
    pt = sed.FusedTrainer(make_model(sed, 0.1, frontend=fe), lr=1e-3, recall_factor=W)
    pt.train_step(x.abs() + 0.1, y)
    assert all(bool(torch.isfinite(v).all()) for v in pt.flat.G.values())
    # need_dx in training mode
    model = make_model(sed, 0.1).train()
    xg = x.clone().requires_grad_(True)
    model(xg).sum().backward()
    assert bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0


def test_launch_labels(sed):
    """p = 0: the list of tests/test_gpu_sa_model.py; p > 0: the _drop twins in the plain launches' places"""
    torch.manual_seed(0)
    sa = T0.step_labels(sed, sed.Csa_AvgPooling(3, CFG, precision="bf16", sa_heads=1, sa_dropout=0.0).cuda())
    h, b = T0.PLAIN_STEP.index("sed_head_fwd"), T0.PLAIN_STEP.index("sed_head_bwd")
    assert sa == T0.PLAIN_STEP[:h] + T0.SA_FWD + T0.PLAIN_STEP[h + 1:b] + T0.SA_BWD + T0.PLAIN_STEP[b + 1:]
    drop = T0.step_labels(sed, sed.Csa_AvgPooling(3, CFG, precision="bf16", sa_heads=1, sa_dropout=0.1).cuda())
    twin = {"sed_mhsa_fwd", "sed_add_layernorm_fwd", "sed_mhsa_bwd", "sed_add_layernorm_bwd"}
    assert drop == [l + "_drop" if l in twin else l for l in sa]
