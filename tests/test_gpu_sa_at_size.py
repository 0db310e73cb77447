"""GPU: the self-attention head (csrc/sed_mhsa.hip, csrc/sed_ffn.hip, CnnEngine._plan_sa / _sa_forward / _sa_backward) through the
engine at a multi-head, multi-tile size, end to end against torch in float64 and launch by launch against float64.

Geometry: CFG = [(32, 2), (64, 2), (128, 2), (128, 1)], 8 mel bins, B = 4 clips of T = 1040 frames, 3 classes, recall weight 5:
C = 128, t = 130 frames per clip, R = B t = 520 rows.  t = 130: two workgroups per (clip, head), a last wave with two live rows, five
key tiles; R = 520: five ragged 128-row tiles; 3C = 384: three column tiles; R // 256 = 2: split-K 2 in every weight-gradient
sed_gemm_tn (asserted from the engine's formula, not patched) through g["tn_ws"].
  A  sa_heads 4 (head width 32), 2 layers, FFN of 256 with GELU, positional table
  B  sa_heads 2 (head width 64), 1 layer, no FFN, no positional table
Biases and LayerNorm affine parameters are randomised (tests/test_gpu_sa_encoder.py: make_model); the input is Gaussian, the conv
stack's output is taken as it comes.

End to end (fp32): as tests/test_gpu_sa_encoder.py / test_gpu_sa_model.py -- the conv output of a head='none' engine on the same
parameters feeds the torch CPU oracle in float64 (TransformerEncoderLayer per layer for A, MultiheadAttention + LayerNorm for B, split
into `heads` heads by torch), whose feature gradient goes back through that engine's backward.  Bounds, the project's own: logits 1e-3
absolute, loss 1e-4, every gradient 3e-3 relative L2.

Launch by launch (fp32 and bf16): one training forward, the loss, one backward; the callback on_group_done clones the shared gradient
buffers of plan.sa on the stream each time a group completes (each buffer is intact at the callback that follows the launch that
wrote it and precedes the one that overwrites it; dm is read at the next callback).  Every launch of the head is then checked per
element, no element left out, against float64 of that ONE operation on the engine's own inputs to it (rounded to bf16 where the
kernel rounds them, in bf16 mode):
  sed_gemm_nt     qkv, a, da (through du = da act'(u): the launch's gate times |act'| in its absolute-value form, plus
                  sed_ffn_act_bwd's own), dh1 - dres, dctx, dm - dres: SAFE (K + 1 + [bias]) u S of
                  tests/test_gpu_crnn_exact_oracle.py, plus u |value| for the in-place residual add
  sed_gemm_tn     every weight gradient and, as its column sums, every bias gradient: that docstring's gemm_tn and colsum gates
                  with ksplit = 2
  sed_mhsa_fwd    mhsa_formula.core / core_gates on the (rounded) thirds of the engine's qkv
  sed_mhsa_bwd    the teacher-forced core on the engine's own ctx, lse and dctx (raw_dctx gates in bf16)
  sed_add_layernorm_fwd / _bwd   mhsa_formula.add_layernorm* with stats = the engine's own; the statistics themselves within
                  tests/test_gpu_mhsa.py's gates
  sed_ffn_fwd, sed_ffn_act_bwd   ffn_formula.ffn_gates (with the mode) and act_bwd_gates
sed_mel_mean_*, sed_head_fwd / _bwd, sed_transpose_shift and the conv stack are pinned elsewhere; their outputs are taken as given.
Run with -s for the worst error / gate per launch kind.

Measured on the MI355X (-s):
  end to end       A: logits 2.1e-6, loss 1.5e-7, worst gradient 1.3e-6 relative L2 (a conv gradient; the head's are below 2.8e-7)
                   B: logits 2.0e-6, loss 1.1e-8, worst gradient 1.2e-6.  The project's bounds hold at R = 520; none was derived anew.
  launch by launch, worst error / gate over both configurations        fp32      bf16
    sed_gemm_nt                                                         0.0098    0.0035
    sed_gemm_tn (split-K 2)                                             0.010     0.0044
    sed_gemm_tn column sums                                             0.013     0.014
    sed_mhsa_fwd                                                        0.031     0.22
    sed_mhsa_bwd                                                        0.050     0.28
    sed_add_layernorm_fwd                                               0.014     0.012
    sed_add_layernorm_bwd                                               0.011     0.010
    sed_ffn_fwd                                                         0.035     0.42
    sed_ffn_act_bwd                                                     0.029     0.031
Tried against local edits of the engine that were not committed: sed_mhsa_fwd / _bwd called with 2 heads of 64 for the 4 x 32 model
fails A end to end (logits off by 0.11) and A launch by launch (sed_mhsa_fwd ctx 7e3 gates out in fp32, 67 in bf16), B passes; the
out-projection reading ctx with a row stride of C / 2 (over K = C / 2, to stay inside the buffer) fails every test, launch by launch
at "a" (1.5e4 gates out); g["tn_ws"] sized for one slab fails the workspace assertion before any backward launch.  (A leading
dimension below K is refused by sed_gemm_nt itself.)
"""
import importlib

import numpy as np
import pytest
import torch

import ffn_formula as FF
import mhsa_formula as F
import test_gpu_sa_encoder as E
import test_gpu_sa_model as T0

pytestmark = pytest.mark.gpu
PKG = "soundeventdetection-pytorch_amd"
CFG = [(32, 2), (64, 2), (128, 2), (128, 1)]
MEL, T, B, K, W = 8, 1040, 4, 3, 5.0
C, t, R = 128, 130, 520
CONF = {"A": dict(sa_heads=4, sa_layers=2, sa_ffn=256, sa_activation="gelu", pos_encoding=True),
        "B": dict(sa_heads=2, sa_layers=1, sa_ffn=0, pos_encoding=False)}
U, SAFE, KS = 2.0 ** -24, 4.0, 2
RATIOS = {}                     # (configuration, precision, launch kind) -> worst error / gate
rel_l2 = T0.rel_l2


@pytest.fixture(scope="module")
def sed():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if RATIOS:
        print("\nworst error / gate by configuration, precision and launch kind (1.0 = at the derived bound)")
        for k in sorted(RATIOS):
            print(f"  {k[0]} {k[1]:5s} {k[2]:28s} {RATIOS[k]:.3e}")


def make_model(sed, conf, precision="fp32", seed=0):
    torch.manual_seed(seed)
    m = sed.Csa_AvgPooling(K, CFG, precision=precision, mel_bins=MEL, **CONF[conf])
    with torch.no_grad():       # as tests/test_gpu_sa_encoder.py: zero / unit initial values would hide a wrong bias or affine gradient
        for n, p in m.named_parameters():
            if n.startswith(("attn", "ffn")):
                if "norm" in n and n.endswith("weight"):
                    p.normal_(1.0, 0.2)
                elif n.endswith("bias"):
                    p.normal_(0.0, 0.1)
    return m.cuda()


def batch():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 1, T, MEL, generator=g)
    y = (torch.rand(B, T, K, generator=g) < 0.3).float()
    return x.cuda(), y.cuda()


# ---- a. fp32, end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conf", ["A", "B"])
def test_fp32_model_matches_torch_at_size(sed, conf):
    cf = CONF[conf]
    x, y = batch()
    model = make_model(sed, conf).train()
    out = model(x)
    loss = sed.WeightedBCE(W, True)(out, y)
    loss.backward()
    plan = T0.the_plan(model)
    assert plan.sa is not None and plan.sa["R"] == R and plan.t_out == t and len(plan.sa["layers"]) == cf["sa_layers"]
    P = model._tensor_dict()
    bare = sed.CnnEngine(K, CFG, 1, "fp32", head="none", mel_bins=MEL)
    bp = bare.forward(x, P, training=True, update_running_stats=False)
    assert torch.equal(bp.y[-1], plan.y[-1])
    feat = bp.y[-1][..., :C].double().cpu().requires_grad_(True)
    assert feat.shape == (B, t, 1, C)
    if cf["sa_ffn"]:
        out_t, loss_t, grads = E.oracle(sed, model.state_dict(), feat, y.double().cpu(), cf["sa_heads"], cf["sa_layers"], cf["sa_ffn"],
                                        cf["sa_activation"], cf["pos_encoding"], model.engine.ratio)
    else:
        out_t, loss_t, grads = T0.oracle_head(model.state_dict(), feat, y.double().cpu(), cf["sa_heads"], cf["pos_encoding"], model.engine.ratio)
    assert out.shape == out_t.shape == (B, T, K)
    err = float((out.detach().cpu().double() - out_t).abs().max())
    print(f"{conf}: logits max error {err:.3e}, loss error {abs(loss.item() - float(loss_t)):.3e}")
    assert err < 1e-3 and abs(loss.item() - float(loss_t)) < 1e-4
    mine = {n for n, _ in model.named_parameters() if not n.startswith("conv_blocks.")}
    assert mine == set(grads), mine ^ set(grads)
    worst = 0.0
    for n, g in grads.items():
        l2 = rel_l2(model.get_parameter(n).grad, g)
        worst = max(worst, l2)
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
        worst = max(worst, l2)
        assert l2 < 3e-3, (n, l2)
    print(f"{conf}: worst gradient relative L2 {worst:.3e}")


# ---- b. launch by launch ---------------------------------------------------------------------------------------------------------------
def f32(x):
    return x.detach().float().cpu().numpy()


def f64(x):
    return np.asarray(x, dtype=np.float64)


class Checker:
    def __init__(self, conf, precision):
        self.key, self.mode = (conf, precision), "bf16" if precision == "bf16" else "f32"

    def opnd(self, a):
        """the operand an MFMA sees, as float64: the fp32 value or its nearest-even bf16 rounding"""
        return f64(F.round_bf16(a)) if self.mode == "bf16" else f64(a)

    def ok(self, kind, what, got, ref, gate):
        good, worst = F.check(got, ref, gate, self.key + (kind, what))
        k = self.key + (kind,)
        RATIOS[k] = max(RATIOS.get(k, 0.0), worst)
        assert good, (self.key, kind, what, worst)

    def nt_ref(self, A, Bm, bias=None):
        """A [M][K], Bm [N][K] fp32 -> (a b^T (+ bias), its gate SAFE (K + 1 + [bias]) u S)"""
        a, b = self.opnd(A), self.opnd(Bm)
        ref, S, count = a @ b.T, np.abs(a) @ np.abs(b).T, a.shape[1] + 1
        if bias is not None:
            ref, S, count = ref + f64(bias), S + np.abs(f64(bias)), count + 1
        return ref, SAFE * count * U * S

    def nt(self, what, got, A, Bm, bias=None, residual=None):
        ref, gate = self.nt_ref(A, Bm, bias)
        if residual is not None:        # the in-place add behind the launch: one more rounding of the sum
            ref = ref + f64(residual)
            gate = gate + U * (np.abs(ref) + gate)
        self.ok("sed_gemm_nt", what, got, ref, gate)

    def tn(self, what, got, got_colsum, A, Bm):
        """A [K][M], Bm [K][N] fp32: a^T b with split-K KS (k-step 64) and the column sums of the fp32 A"""
        a, b = self.opnd(A), self.opnd(Bm)
        rows = a.shape[0]
        kchunk = -(-(-(-rows // KS)) // 64) * 64
        nslab = -(-rows // kchunk)
        kc = min(kchunk, rows)
        assert nslab == KS
        self.ok("sed_gemm_tn", what, got, a.T @ b, SAFE * (kc + nslab) * U * (np.abs(a).T @ np.abs(b)))
        self.ok("sed_gemm_tn colsum", what, got_colsum, f64(A).sum(axis=0), SAFE * (-(-kc // 8) + 8 + nslab) * U * np.abs(f64(A)).sum(axis=0))


def launch_by_launch(sed, conf, precision):
    cf = CONF[conf]
    H, layers, D, act, pos = cf["sa_heads"], cf["sa_layers"], cf["sa_ffn"], cf.get("sa_activation", "relu"), cf["pos_encoding"]
    dh = C // H
    ck = Checker(conf, precision)
    x, y = batch()
    model = make_model(sed, conf, precision).train()
    eng, P = model.engine, model._tensor_dict()
    G = {n: torch.full_like(p, float("nan")) for n, p in model.named_parameters()}
    plan = eng.forward(x, P, training=True)
    eng.loss_and_grad(plan, y, W)
    g = plan.sa
    assert g["R"] == R and plan.t_out == t and len(g["layers"]) == layers
    lib = eng.lib
    assert max(1, min(g["ksplit"], R // 256)) == KS, "the weight-gradient products of this size are meant to run split-K 2"
    need = [lib.sed_gemm_tn_ws_floats(3 * C, C, KS)] + ([lib.sed_gemm_tn_ws_floats(C, D, KS), lib.sed_gemm_tn_ws_floats(D, C, KS)] if D else [])
    assert g["tn_ws"].numel() >= max(need) and need[0] == KS * (3 * C * C + 3 * C), "g['tn_ws'] is smaller than a split-K launch needs"
    shared = [n for n in ("dh", "dres", "dctx", "dqkv", "dm", "fda", "ffa", "dh1") if n in g]
    for n in shared:
        g[n].fill_(float("nan"))
    order, snaps = [], []

    def cb(name):                   # on the current stream: ordered behind the launches of the group, before the next group's
        order.append(name)
        snaps.append({n: g[n].clone() for n in shared})

    eng.backward(plan, P, G, on_group_done=cb)
    torch.cuda.synchronize()
    want = ["event_fc"]
    for l in reversed(range(layers)):
        an, nn_, fn, fnn = eng.sa_layer_names(l)
        want += ([fnn, fn] if D else []) + [nn_, an]
    assert order[:len(want)] == want and len(order) > len(want), order

    def at(name, buf):
        return f32(snaps[order.index(name)][buf])

    def after(name, buf):           # the callback that follows `name`
        return f32(snaps[order.index(name) + 1][buf])

    Pn = {n: f32(v) for n, v in P.items() if n.startswith(("attn", "ffn"))}
    Gn = {n: f32(v) for n, v in G.items() if n.startswith(("attn", "ffn"))}
    assert all(np.isfinite(v).all() for v in Gn.values())
    m = f32(g["m"])
    k_ln = (C + 8) * U

    def layernorm(tag, xin, a, gamma, beta, dy, y_got, stats_got, dres_got, dgamma_got, dbeta_got):
        r = F.add_layernorm(xin, a, gamma, beta, dy, stats=stats_got)
        gt = F.add_layernorm_gates(xin, a, gamma, beta, dy, stats=stats_got)
        ck.ok("sed_add_layernorm_fwd", tag + " y", y_got, r["y"], gt["y"])
        z = r["z"]
        M = np.abs(z).mean(axis=1)
        d = np.abs(z - r["mean"][:, None])
        ck.ok("sed_add_layernorm_fwd", tag + " mean", stats_got[:, 0], r["mean"], k_ln * M)
        ck.ok("sed_add_layernorm_fwd", tag + " rstd", stats_got[:, 1], r["rstd"],
              k_ln * r["rstd"] * (1.0 + r["rstd"] ** 2 * (d * (np.abs(z) + M[:, None])).mean(axis=1)))
        ck.ok("sed_add_layernorm_bwd", tag + " dres", dres_got, r["dres"], gt["dres"])
        ck.ok("sed_add_layernorm_bwd", tag + " dgamma", dgamma_got, r["dgamma"], gt["dgamma"])
        ck.ok("sed_add_layernorm_bwd", tag + " dbeta", dbeta_got, r["dbeta"], gt["dbeta"])

    gcur = at("event_fc", "dh")                     # the gradient of the last layer's output (sed_head_bwd: pinned elsewhere)
    for l in reversed(range(layers)):
        an, nn_, fn, fnn = eng.sa_layer_names(l)
        ly = {n: f32(v) for n, v in g["layers"][l].items()}
        xin = m if l == 0 else f32(g["layers"][l - 1]["h2" if D else "h"])
        tag = f"l{l}"
        Win, bin_, Wout, bout = (Pn[an + s] for s in (".in_proj_weight", ".in_proj_bias", ".out_proj.weight", ".out_proj.bias"))
        # ---- forward ----
        ck.nt(tag + " qkv", ly["qkv"], xin, Win, bin_)
        qkv_op = F.round_bf16(ly["qkv"]) if ck.mode == "bf16" else ly["qkv"]
        q, k, v = F.split_qkv(qkv_op, B, t, H, dh)
        ck.nt(tag + " a", ly["a"], ly["ctx"], Wout, bout)
        if D:
            w1, b1, w2, b2 = (Pn[fn + s] for s in (".linear1.weight", ".linear1.bias", ".linear2.weight", ".linear2.bias"))
            fr = FF.ffn(ly["h"], w1, b1, w2, b2, act)
            fg = FF.ffn_gates(ly["h"], w1, b1, w2, b2, act, mode=ck.mode)
            ck.ok("sed_ffn_fwd", tag + " u", ly["u"], fr["u"], fg["u"])
            ck.ok("sed_ffn_fwd", tag + " f", ly["f"], fr["y"], fg["y"])
            # ---- backward of the FFN sub-layer ----
            dres_f = at(fnn, "dres")
            assert np.array_equal(dres_f, at(fn, "dres"))
            layernorm(tag + " ffn_norm", ly["h"], ly["f"], Pn[fnn + ".weight"], Pn[fnn + ".bias"], gcur, ly["h2"], ly["stats2"], dres_f,
                      Gn[fnn + ".weight"], Gn[fnn + ".bias"])
            du, a_hid = at(fn, "fda"), at(fn, "ffa")
            da_ref, e_da = ck.nt_ref(dres_f, w2.T)
            u64 = f64(ly["u"])
            gabs = (u64 > 0).astype(np.float64) if act == "relu" else FF.Phi(u64) + np.abs(u64) * FF.phi(u64)
            ag = FF.act_bwd_gates(ly["u"], np.abs(da_ref) + e_da, act)
            ck.ok("sed_gemm_nt", tag + " da (through du)", du, da_ref * FF.act_grad(u64, act), e_da * gabs + ag["du"])
            ck.ok("sed_ffn_act_bwd", tag + " a", a_hid, FF.act_fwd(u64, act), ag["a"])
            ck.tn(tag + " linear2", Gn[fn + ".linear2.weight"], Gn[fn + ".linear2.bias"], dres_f, a_hid)
            ck.tn(tag + " linear1", Gn[fn + ".linear1.weight"], Gn[fn + ".linear1.bias"], du, ly["h"])
            gcur = at(nn_, "dh1")
            ck.nt(tag + " dh1", gcur, du, w1.T, residual=dres_f)
        # ---- backward of the attention sub-layer ----
        dres_a = at(nn_, "dres")
        assert np.array_equal(dres_a, at(an, "dres"))
        layernorm(tag + " attn_norm", xin, ly["a"], Pn[nn_ + ".weight"], Pn[nn_ + ".bias"], gcur, ly["h"], ly["stats"], dres_a,
                  Gn[nn_ + ".weight"], Gn[nn_ + ".bias"])
        ck.tn(tag + " out_proj", Gn[an + ".out_proj.weight"], Gn[an + ".out_proj.bias"], dres_a, ly["ctx"])
        dctx, dqkv = at(an, "dctx"), at(an, "dqkv")
        ck.nt(tag + " dctx", dctx, dres_a, Wout.T)
        d4, ctx4 = dctx.reshape(B, t, H, dh), ly["ctx"].reshape(B, t, H, dh)
        cr = F.core(q, k, v, d4, lse=ly["lse"], ctx=ctx4)
        cg = F.core_gates(q, k, v, d4, ck.mode, raw_dctx=ck.mode == "bf16", lse=ly["lse"], ctx=ctx4)
        ck.ok("sed_mhsa_fwd", tag + " ctx", ctx4, cr["ctx"], cg["ctx"])
        ck.ok("sed_mhsa_fwd", tag + " lse", ly["lse"], cr["lse"], cg["lse"])
        for name, got in zip(("dq", "dk", "dv"), F.split_qkv(dqkv, B, t, H, dh)):
            ck.ok("sed_mhsa_bwd", tag + " " + name, got, cr[name], cg[name])
        ck.tn(tag + " in_proj", Gn[an + ".in_proj_weight"], Gn[an + ".in_proj_bias"], dqkv, xin)
        gcur = after(an, "dm")
        ck.nt(tag + " dm", gcur, dqkv, Win.T, residual=dres_a)
    assert np.array_equal(gcur, f32(g["dm"])), "dm changed after the head's backward"
    kinds = {k[2] for k in RATIOS if k[:2] == ck.key}
    assert {"sed_gemm_nt", "sed_gemm_tn", "sed_gemm_tn colsum", "sed_mhsa_fwd", "sed_mhsa_bwd", "sed_add_layernorm_fwd",
            "sed_add_layernorm_bwd"} <= kinds and (not D or {"sed_ffn_fwd", "sed_ffn_act_bwd"} <= kinds)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("conf", ["A", "B"])
def test_every_launch_of_the_head_against_float64(sed, conf, precision):
    launch_by_launch(sed, conf, precision)
