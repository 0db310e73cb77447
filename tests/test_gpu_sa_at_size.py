"""GPU: the self-attention head (csrc/sed_mhsa.hip, csrc/sed_ffn.hip, heads.SaHead's plan / forward / backward) through the
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

The Conformer convolution module (csrc/sed_convmod.hip, heads.SaHead._conv_forward / _conv_backward) at the same geometry:
  AC  A plus sa_conv_kernel 7        BC  B plus sa_conv_kernel 31
Biases, the LayerNorm and BatchNorm affine parameters and the running statistics are randomised (tests/test_gpu_sa_conformer.py:
make_model).  What this size makes happen, asserted from the library (conv_geometry) or the engine (Step): three frame tiles of 64 per
clip, the last with 2 live frames, so that with k = 31 (p = 15) its halo reaches into the previous tile and, past frame 129, must be
zero and not the next of the B = 4 back-to-back clips; 12 forward and 5 backward partial rows, the last of 8 live rows; four 32-channel
groups; split-K 2 in the pointwise2 (C x C) and pointwise1 (2C x C, lda = 2C) weight gradients, whose workspace need is checked too.
End to end (fp32; AC and BC in training mode, AC also in eval mode): tests/test_gpu_sa_conformer.py's compare and oracle at this
geometry (the FFN-less BC from MultiheadAttention + LayerNorm, as B), with its bounds: logits 1e-3, loss 1e-4, gradients 3e-3 relative
L2, depthwise.bias in training mode by that file's rule, running statistics 1e-4 relative L2 and the counter + 1; in eval mode the
running statistics and the counter keep their bits.
Launch by launch (fp32 and bf16), between attn_norm and the FFN or the head, every element:
  sed_gemm_nt     cg, co; ds only through gz (the engine writes gz over it before any callback: ds_ref silu'(y) within the launch's
                  gate times A(y), the absolute-value form of silu', plus sed_bn_silu_bwd_reduce's own gate at |ds_ref| + e_ds:
                  convmod_formula.gz_through_ds); dhc - dres
  sed_gemm_tn     pointwise2 and pointwise1 (M = 2C) weight gradients, their bias gradients as column sums, split-K 2
  sed_dwconv_glu_fwd   cv, cz from the engine's cg (convmod_formula: glu, dwconv, fwd_gates); the 12 partial rows of the last layer
                  (the layers share g["cpart"]) as column sums against that layer's cz
  sed_bn_train_finalize   cmean, cinvstd, cscale, cshift and the running statistics from their values before the step: bn_coeffs on the
                  engine's cz, finalize_gates with gate_z = 0
  sed_bn_silu_fwd   cs from the engine's cz, cscale, cshift (bn_silu, bn_silu_gates)
  sed_add_layernorm_fwd / _bwd   conv_norm: hc, stats3, dres and its gradients, as the other LayerNorms
  sed_bn_silu_bwd_reduce   gz (above) and the 5 partial rows of g["cbpart"] as column sums (gates widened by the ds term)
  sed_bn_bwd_finalize   ca, cb, cc and the BatchNorm's gradients from the float64 column sums of the engine's own partial rows
                  (convmod_formula.bn_bwd_finalize: the gate forms of tests/test_gpu_ops_exact_oracle.py's test_bn_bwd_finalize)
  sed_dwconv_glu_bwd   cdg and the depthwise gradients from the engine's gz, cz, coefficients, cv, cg (dwconv_bwd, glu_bwd, bwd_gates)
The vector launches are fp32 in every mode, so their gates are the same in both; the gate of an input a launch takes from the engine
is zero.  Eval-mode route (AC, fp32; the module's launches only): sed_bn_eval_coeffs, sed_bn_eval_stats (convmod_formula.bn_eval: the
gates of test_bn_eval_coeffs), sed_bn_eval_bwd_finalize (ca within one rounding, cb and cc exactly 0, the gradients against the column
sums), then dg, dw, dbias as above; the running statistics keep their bits.  Two states of the forward, on bits: an eval forward
without keep_for_grad leaves a NaN-filled cv NaN; update_running_stats=False changes no bit of cz and cs and touches no buffer.

Measured on the MI355X (-s):
  end to end       AC training: logits 2.1e-6, loss 1.1e-8, worst gradient 3.8e-6 relative L2 (convm_l1.pointwise1.bias; the conv
                   stack's 1.3e-6), depthwise.bias 1.6e-6 of the filter gradient's norm, running statistics 4.9e-8
                   BC training: logits 1.5e-6, loss 8.4e-8, worst gradient 1.3e-6 (a conv-stack gradient; the head's 1.2e-6),
                   depthwise.bias 2.8e-7, running statistics 4.7e-8
                   AC eval: logits 2.9e-6, loss 4.6e-9, worst gradient 2.7e-7; every running statistic and counter bit kept
  launch by launch, worst error / gate over AC and BC                  fp32      bf16      AC eval, fp32
    sed_gemm_nt                                                         0.0088    0.0047
    sed_gemm_tn (split-K 2)                                             0.012     0.0044
    sed_gemm_tn column sums                                             0.013     0.013
    sed_mhsa_fwd                                                        0.030     0.21
    sed_mhsa_bwd                                                        0.044     0.29
    sed_add_layernorm_fwd                                               0.013     0.014
    sed_add_layernorm_bwd                                               0.011     0.011
    sed_ffn_fwd (AC)                                                    0.034     0.37
    sed_ffn_act_bwd (AC)                                                0.026     0.028
    sed_dwconv_glu_fwd                                                  0.20      0.18      0.23
    sed_bn_train_finalize                                               0.57      0.58
    sed_bn_silu_fwd                                                     0.067     0.068     0.067
    sed_bn_silu_bwd_reduce (through the GEMM's gate)                    0.0084    0.0030    0.0081
    sed_bn_bwd_finalize                                                 0.25      0.24
    sed_dwconv_glu_bwd                                                  0.11      0.11      0.11
    sed_bn_eval_coeffs / _stats / _bwd_finalize                                             0.11 / 0.090 / 0.24
No launch missed a gate and no bug was found.  Tried against local edits of the engine, each once, none committed (failing tests of
this file; tests/test_gpu_sa_conformer.py's tiny configuration beside them):
  - the number of clips B as the part count of sed_bn_train_finalize (4 of the 12 rows): AC and BC fail end to end (logits off by
    1.9 and 1.1) and launch by launch at "mean" (1.6e5 gates out); the tiny configuration passes, its 2 clips being its 2 rows;
  - nparts - 1 passed to sed_bn_bwd_finalize: launch by launch fails at "cb" (1.8e7 gates out in AC, 4.0e6 in BC); end to end the
    worst gradient is 5.3e-3 (AC) and 1.3e-2 (BC) relative L2, little above the 3e-3 bound; at the tiny size the part count becomes 0,
    which the library refuses;
  - layer 0's cz passed to layer 1's sed_dwconv_glu_bwd: AC fails end to end (attn.in_proj_weight 0.54) and launch by launch at
    "l1 dg" (6.5e6 gates out), BC has one layer and passes; the tiny two-layer case fails too (1.5);
  - eval_bwd forced True in a training step: sed_bn_eval_stats overwrites the batch statistics, so launch by launch fails at
    "mean" (1.9e6 gates out in AC, 8.0e5 in BC), end to end at 6.8e-2 and 6.5e-2; the tiny cases fail too;
  - sed_dwconv_glu_fwd called with (B, t) = (1, R), the clips as one sequence: every training and eval test fails, launch by launch
    at "cz" (1.9e6 gates out with k = 7, 4.0e5 with k = 31), end to end with logits off by 1.5 / 0.95 / 0.13; the tiny cases fail too.
"""
import importlib

import numpy as np
import pytest
import torch

import convmod_formula as V
import ffn_formula as FF
import mhsa_formula as F
import test_gpu_sa_conformer as CM
import test_gpu_sa_encoder as E
import test_gpu_sa_model as T0

pytestmark = pytest.mark.gpu
PKG = "soundeventdetection-pytorch_amd"
CFG = [(32, 2), (64, 2), (128, 2), (128, 1)]
MEL, T, B, K, W = 8, 1040, 4, 3, 5.0
C, t, R = 128, 130, 520
CONF = {"A": dict(sa_heads=4, sa_layers=2, sa_ffn=256, sa_activation="gelu", pos_encoding=True),
        "B": dict(sa_heads=2, sa_layers=1, sa_ffn=0, pos_encoding=False)}
CONF["AC"] = dict(CONF["A"], sa_conv_kernel=7)
CONF["BC"] = dict(CONF["B"], sa_conv_kernel=31)
U, SAFE, KS = 2.0 ** -24, 4.0, 2
RED_ROWS = 128                  # rows a workgroup of sed_bn_silu_bwd_reduce owns (include/sed_hip.h); conv_geometry checks the part count
CONV_KINDS = ["sed_dwconv_glu_fwd", "sed_bn_silu_fwd", "sed_bn_silu_bwd_reduce", "sed_dwconv_glu_bwd", "sed_bn_train_finalize",
              "sed_bn_bwd_finalize"]
EVAL_KINDS = ["sed_bn_eval_coeffs", "sed_bn_eval_stats", "sed_bn_eval_bwd_finalize"]
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
            if n.startswith(("attn", "ffn", "convm", "conv_norm")):
                if ("norm" in n or ".bn." in n) and n.endswith("weight"):
                    p.normal_(1.0, 0.2)
                elif n.endswith("bias"):
                    p.normal_(0.0, 0.1)
        for n, b in m.named_buffers():      # as tests/test_gpu_sa_conformer.py: nor may the running statistics stay at 0 / 1
            if n.startswith("convm") and n.endswith("running_mean"):
                b.normal_(0.0, 0.2)
            if n.startswith("convm") and n.endswith("running_var"):
                b.uniform_(0.5, 1.5)
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


@pytest.mark.parametrize("conf,training", [("AC", True), ("BC", True), ("AC", False)], ids=["AC-train", "BC-train", "AC-eval"])
def test_fp32_conformer_model_matches_torch_at_size(sed, conf, training):
    """tests/test_gpu_sa_conformer.py's compare at this geometry: its bounds, its rule for depthwise.bias in training mode, the running
    statistics within 1e-4 relative L2 and the counter + 1 (training) or every bit of them kept (eval)"""
    cf = CONF[conf]
    x, y = batch()
    model = make_model(sed, conf)
    bare, bp, feat, P0 = CM.compare(sed, model, x, y, cf["sa_layers"], cf["sa_ffn"], cf["sa_conv_kernel"], training, f"{conf} training={training}",
                                    cfg=CFG, mel=MEL, heads=cf["sa_heads"], pos=cf["pos_encoding"], act=cf.get("sa_activation", "relu"),
                                    plain_attention=not cf["sa_ffn"])
    plan = T0.the_plan(model)
    assert plan.sa["R"] == R and plan.t_out == t and feat.shape == (B, t, 1, C)
    # the oracle's feature gradient back through the pinned conv backward
    bp.dy[-1].zero_()
    bp.dy[-1][..., :C] = feat.grad.float().cuda()
    names = [n for n, _ in model.named_parameters() if n.startswith("conv_blocks.")]
    G = {n: torch.full_like(P0[n], float("nan")) for n in names}
    bare.backward(bp, P0, G)
    worst = 0.0
    for n in names:
        l2 = rel_l2(model.get_parameter(n).grad, G[n])
        worst = max(worst, l2)
        assert l2 < 3e-3, (n, l2)
    print(f"{conf} training={training}: worst conv-stack gradient relative L2 {worst:.3e}")


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


class Step:
    """One forward, the loss and one backward of a configuration through its engine; the shared gradient buffers of plan.sa are cloned
    at every callback.  training=False: the eval-mode route, forward(training=False, keep_for_grad=True)."""

    def __init__(self, sed, conf, precision, training=True):
        cf = CONF[conf]
        layers, D, kc = cf["sa_layers"], cf["sa_ffn"], cf.get("sa_conv_kernel", 0)
        x, y = batch()
        self.model = model = make_model(sed, conf, precision).train(training)
        self.eng, self.P = eng, P = model.engine, model._tensor_dict()
        self.G = G = {n: torch.full_like(p, float("nan")) for n, p in model.named_parameters()}
        self.run0 = {n: f32(v) for n, v in P.items() if n.startswith("convm") and ".bn.running_" in n}       # before the step
        self.plan = plan = eng.forward(x, P, training=True) if training else eng.forward(x, P, training=False, keep_for_grad=True)
        eng.loss_and_grad(plan, y, W)
        self.g = g = plan.sa
        assert g["R"] == R and plan.t_out == t and len(g["layers"]) == layers
        lib = eng.lib
        assert max(1, min(g["ksplit"], R // 256)) == KS, "the weight-gradient products of this size are meant to run split-K 2"
        need = [lib.sed_gemm_tn_ws_floats(3 * C, C, KS)] + ([lib.sed_gemm_tn_ws_floats(C, D, KS), lib.sed_gemm_tn_ws_floats(D, C, KS)] if D else []) \
            + ([lib.sed_gemm_tn_ws_floats(2 * C, C, KS)] if kc else [])
        assert g["tn_ws"].numel() >= max(need) and need[0] == KS * (3 * C * C + 3 * C), "g['tn_ws'] is smaller than a split-K launch needs"
        shared = [n for n in ("dh", "dres", "dctx", "dqkv", "dm", "fda", "ffa", "dh1", "cds", "cdg", "dhc", "ccoef", "cbpart") if n in g]
        assert ("cds" in shared) == bool(kc)
        for n in shared:
            g[n].fill_(float("nan"))
        self.order, self.snaps = order, snaps = [], []

        def cb(name):                   # on the current stream: ordered behind the launches of the group, before the next group's
            order.append(name)
            snaps.append({n: g[n].clone() for n in shared})

        eng.backward(plan, P, G, on_group_done=cb)
        torch.cuda.synchronize()
        want = ["event_fc"]
        for l in reversed(range(layers)):
            an, nn_, fn, fnn = eng.sa_layer_names(l)
            cm, cn = eng.sa_conv_names(l)
            want += ([fnn, fn] if D else []) + ([cn, cm] if kc else []) + [nn_, an]
        assert order[:len(want)] == want and len(order) > len(want), order

    def at(self, name, buf):
        return f32(self.snaps[self.order.index(name)][buf])

    def after(self, name, buf):         # the callback that follows `name`
        return f32(self.snaps[self.order.index(name) + 1][buf])


def conv_geometry(lib, kc):
    """what R = 520 makes happen in the module's launches, asked of the library; -> the forward's frame tile"""
    tile = lib.sed_dwconv_tile()
    assert tile == 64 and -(-t // tile) == 3 and t - 2 * tile == 2, "three frame tiles per clip, the last with 2 live frames"
    assert kc != 31 or (kc - 1) // 2 > t - 2 * tile, "k = 31: the last tile's halo reaches past its own live frames into the previous tile"
    assert lib.sed_dwconv_nparts(B, t) == 12 and lib.sed_dwconv_glu_fwd_ws_floats(B, t, C) == 12 * 2 * C
    assert lib.sed_bn_silu_bwd_nparts(R) == 5 == -(-R // RED_ROWS) and R - 4 * RED_ROWS == 8, "five backward parts, the last with 8 live rows"
    assert C // 32 == 4
    return tile


def conv_module(ck, lib, tag, kc, ly, snap, ds, Wc, dWc, run0, run1, training, cpart=None):
    """The vector launches of one layer's convolution module and its BatchNorm finalisations, each against float64 of that one
    operation on the engine's own inputs to it (their gates zero).  ly: the layer's kept buffers; snap: cds (gz), cbpart, ccoef, cdg at
    the module's callback; ds = (reference, gate) of the product the engine overwrites with gz; Wc / dWc: the module's parameters and
    gradients without the prefix; run0 / run1: the running statistics before and after the step; cpart: the forward partial rows
    (the layers share them: the last layer's alone survive)."""
    tile = conv_geometry(lib, kc)
    wd, bd, gamma, beta = Wc["depthwise.weight"].reshape(C, kc), Wc["depthwise.bias"], Wc["bn.weight"], Wc["bn.bias"]
    cg, cv, cz = ly["cg"], ly["cv"], ly["cz"]
    # ---- sed_dwconv_glu_fwd from the engine's cg
    rv = V.glu(cg)
    fg = V.fwd_gates(cg, wd, bd, B, t, tile)
    ck.ok("sed_dwconv_glu_fwd", tag + " cv", cv, rv, fg["v"])
    ck.ok("sed_dwconv_glu_fwd", tag + " cz", cz, V.dwconv(rv, wd, bd, B, t), fg["z"])
    if cpart is not None:
        sums = V.exact_colsum(cpart)
        ck.ok("sed_dwconv_glu_fwd", tag + " sum z", sums[0], f64(cz).sum(axis=0), fg["sum"])
        ck.ok("sed_dwconv_glu_fwd", tag + " sum z^2", sums[1], (f64(cz) ** 2).sum(axis=0), fg["sumsq"])
    # ---- the BatchNorm's coefficients
    if training:
        # V.finalize_gates is an absolute error relative to mean(z^2), not to the variance; with the engine's own cz as the
        # reference's input (gate_z = 0) that only loosens the gate, it hides no error of the sums.
        bn = V.bn_coeffs(cz, gamma, beta, run0["mean"], run0["var"], True)
        fin = V.finalize_gates(cz, np.zeros_like(cz, dtype=np.float64), gamma, beta, run0["mean"], run0["var"], tile)
        for name, got in (("mean", ly["cmean"]), ("invstd", ly["cinvstd"]), ("scale", ly["cscale"]), ("shift", ly["cshift"]),
                          ("running_mean", run1["mean"]), ("running_var", run1["var"])):
            ck.ok("sed_bn_train_finalize", f"{tag} {name}", got, bn[name], fin[name])
    else:
        ref, gt = V.bn_eval(gamma, beta, run0["mean"], run0["var"])
        for name, kind in (("scale", "sed_bn_eval_coeffs"), ("shift", "sed_bn_eval_coeffs"), ("mean", "sed_bn_eval_stats"), ("invstd", "sed_bn_eval_stats")):
            ck.ok(kind, f"{tag} {name}", ly["c" + name], ref[name], gt[name])
        assert np.array_equal(run1["mean"], run0["mean"]) and np.array_equal(run1["var"], run0["var"]), "an eval step changed a running statistic"
    sc, sh, mu, inv = ly["cscale"], ly["cshift"], ly["cmean"], ly["cinvstd"]
    # ---- sed_bn_silu_fwd
    ck.ok("sed_bn_silu_fwd", tag + " cs", ly["cs"], V.bn_silu(cz, sc, sh)[1], V.bn_silu_gates(cz, sc, sh)["s"])
    # ---- sed_bn_silu_bwd_reduce, gz over the GEMM's ds: gz and the five partial rows
    (rgz, rsum, rsumx), bg = V.gz_through_ds(ds[0], ds[1], cz, sc, sh, mu, inv, RED_ROWS)
    gz, part = snap["cds"], snap["cbpart"]
    assert part.shape == (5, 2, C)
    ck.ok("sed_bn_silu_bwd_reduce", tag + " gz (and ds through it)", gz, rgz, bg["gz"])
    bsum = V.exact_colsum(part)
    ck.ok("sed_bn_silu_bwd_reduce", tag + " sum gz", bsum[0], rsum, bg["sum"])
    ck.ok("sed_bn_silu_bwd_reduce", tag + " sum gz xhat", bsum[1], rsumx, bg["sumx"])
    # ---- the finalisation on the engine's own partial rows
    ref, gt = V.bn_bwd_finalize(part, R, gamma, mu, inv, training)
    coef = snap["ccoef"]
    kind = "sed_bn_bwd_finalize" if training else "sed_bn_eval_bwd_finalize"
    for name, got in (("ca", coef[0]), ("cb", coef[1]), ("cc", coef[2]), ("dgamma", dWc["bn.weight"]), ("dbeta", dWc["bn.bias"])):
        ck.ok(kind, f"{tag} {name}", got, ref[name], gt[name])
    assert training or not (coef[1].any() or coef[2].any())
    # ---- sed_dwconv_glu_bwd from the engine's gz, cz, coefficients, cv and cg
    dz = f64(coef[0]) * f64(gz) + f64(coef[1]) * f64(cz) + f64(coef[2])
    rdv, rdw, rdb = V.dwconv_bwd(dz, cv, wd, B, t)
    wg = V.bwd_gates(gz, cz, coef[0], coef[1], coef[2], cv, cg, wd, B, t, tile)
    ck.ok("sed_dwconv_glu_bwd", tag + " dg", snap["cdg"], V.glu_bwd(rdv, cg), wg["dg"])
    ck.ok("sed_dwconv_glu_bwd", tag + " dw", dWc["depthwise.weight"].reshape(C, kc), rdw, wg["dw"])
    ck.ok("sed_dwconv_glu_bwd", tag + " dbias", dWc["depthwise.bias"], rdb, wg["dbias"])


def conv_operands(st, l):
    """layer l's module as conv_module takes it: (the module callback's snapshot, parameters, gradients, running statistics before /
    after), numpy, names without the prefix"""
    cm, cn = st.eng.sa_conv_names(l)
    snap = {n: st.at(cm, n) for n in ("cds", "cbpart", "ccoef", "cdg", "dres")}
    Wc = {n[len(cm) + 1:]: f32(v) for n, v in st.P.items() if n.startswith(cm + ".") and v.is_floating_point()}
    dWc = {n[len(cm) + 1:]: f32(v) for n, v in st.G.items() if n.startswith(cm + ".")}
    run0 = dict(mean=st.run0[cm + ".bn.running_mean"], var=st.run0[cm + ".bn.running_var"])
    run1 = dict(mean=Wc["bn.running_mean"], var=Wc["bn.running_var"])
    return snap, Wc, dWc, run0, run1


def launch_by_launch(sed, conf, precision):
    cf = CONF[conf]
    H, layers, D, act, pos = cf["sa_heads"], cf["sa_layers"], cf["sa_ffn"], cf.get("sa_activation", "relu"), cf["pos_encoding"]
    kc = cf.get("sa_conv_kernel", 0)
    dh = C // H
    ck = Checker(conf, precision)
    st = Step(sed, conf, precision)
    eng, P, G, g, at, after = st.eng, st.P, st.G, st.g, st.at, st.after
    mine = ("attn", "ffn", "convm", "conv_norm")
    Pn = {n: f32(v) for n, v in P.items() if n.startswith(mine) and v.is_floating_point()}
    Gn = {n: f32(v) for n, v in G.items() if n.startswith(mine)}
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
        cm, cn = eng.sa_conv_names(l)
        ly = {n: f32(v) for n, v in g["layers"][l].items()}
        xin = m if l == 0 else f32(eng._sa_layer_out(g["layers"][l - 1]))
        assert l == 0 or eng._sa_layer_out(g["layers"][l - 1]) is g["layers"][l - 1]["h2" if D else "hc" if kc else "h"]
        fin = ly["hc"] if kc else ly["h"]           # the FFN sub-layer's input
        tag = f"l{l}"
        Win, bin_, Wout, bout = (Pn[an + s] for s in (".in_proj_weight", ".in_proj_bias", ".out_proj.weight", ".out_proj.bias"))
        # ---- forward ----
        ck.nt(tag + " qkv", ly["qkv"], xin, Win, bin_)
        qkv_op = F.round_bf16(ly["qkv"]) if ck.mode == "bf16" else ly["qkv"]
        q, k, v = F.split_qkv(qkv_op, B, t, H, dh)
        ck.nt(tag + " a", ly["a"], ly["ctx"], Wout, bout)
        if D:
            w1, b1, w2, b2 = (Pn[fn + s] for s in (".linear1.weight", ".linear1.bias", ".linear2.weight", ".linear2.bias"))
            fr = FF.ffn(fin, w1, b1, w2, b2, act)
            fg = FF.ffn_gates(fin, w1, b1, w2, b2, act, mode=ck.mode)
            ck.ok("sed_ffn_fwd", tag + " u", ly["u"], fr["u"], fg["u"])
            ck.ok("sed_ffn_fwd", tag + " f", ly["f"], fr["y"], fg["y"])
            # ---- backward of the FFN sub-layer ----
            dres_f = at(fnn, "dres")
            assert np.array_equal(dres_f, at(fn, "dres"))
            layernorm(tag + " ffn_norm", fin, ly["f"], Pn[fnn + ".weight"], Pn[fnn + ".bias"], gcur, ly["h2"], ly["stats2"], dres_f,
                      Gn[fnn + ".weight"], Gn[fnn + ".bias"])
            du, a_hid = at(fn, "fda"), at(fn, "ffa")
            da_ref, e_da = ck.nt_ref(dres_f, w2.T)
            u64 = f64(ly["u"])
            gabs = (u64 > 0).astype(np.float64) if act == "relu" else FF.Phi(u64) + np.abs(u64) * FF.phi(u64)
            ag = FF.act_bwd_gates(ly["u"], np.abs(da_ref) + e_da, act)
            ck.ok("sed_gemm_nt", tag + " da (through du)", du, da_ref * FF.act_grad(u64, act), e_da * gabs + ag["du"])
            ck.ok("sed_ffn_act_bwd", tag + " a", a_hid, FF.act_fwd(u64, act), ag["a"])
            ck.tn(tag + " linear2", Gn[fn + ".linear2.weight"], Gn[fn + ".linear2.bias"], dres_f, a_hid)
            ck.tn(tag + " linear1", Gn[fn + ".linear1.weight"], Gn[fn + ".linear1.bias"], du, fin)
            gcur = at(cn if kc else nn_, "dh1")
            ck.nt(tag + " dh1", gcur, du, w1.T, residual=dres_f)
        if kc:
            # ---- the convolution module: its two products forward, conv_norm, then the backward down to the gradient of h
            snap, Wc, dWc, run0, run1 = conv_operands(st, l)
            W1, W2 = Wc["pointwise1.weight"].reshape(2 * C, C), Wc["pointwise2.weight"].reshape(C, C)
            ck.nt(tag + " cg", ly["cg"], ly["h"], W1, Wc["pointwise1.bias"])
            ck.nt(tag + " co", ly["co"], ly["cs"], W2, Wc["pointwise2.bias"])
            dres_c = at(cn, "dres")
            assert np.array_equal(dres_c, snap["dres"])
            layernorm(tag + " conv_norm", ly["h"], ly["co"], Pn[cn + ".weight"], Pn[cn + ".bias"], gcur, ly["hc"], ly["stats3"], dres_c,
                      Gn[cn + ".weight"], Gn[cn + ".bias"])
            ck.tn(tag + " pointwise2", dWc["pointwise2.weight"].reshape(C, C), dWc["pointwise2.bias"], dres_c, ly["cs"])
            conv_module(ck, eng.lib, tag, kc, ly, snap, ck.nt_ref(dres_c, W2.T), Wc, dWc, run0, run1, True,
                        cpart=f32(g["cpart"])[:12 * 2 * C].reshape(12, 2, C) if l == layers - 1 else None)
            ck.tn(tag + " pointwise1", dWc["pointwise1.weight"].reshape(2 * C, C), dWc["pointwise1.bias"], snap["cdg"], ly["h"])
            gcur = at(nn_, "dhc")
            ck.nt(tag + " dhc", gcur, snap["cdg"], W1.T, residual=dres_c)
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
    assert not kc or set(CONV_KINDS) <= kinds
    assert kc or not (set(CONV_KINDS) | set(EVAL_KINDS)) & kinds


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("conf", ["A", "B"])
def test_every_launch_of_the_head_against_float64(sed, conf, precision):
    launch_by_launch(sed, conf, precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("conf", ["AC", "BC"])
def test_every_launch_of_the_conformer_head_against_float64(sed, conf, precision):
    launch_by_launch(sed, conf, precision)


# ---- c. the module's eval-mode route and two states of its forward ---------------------------------------------------------------------
def test_eval_route_of_the_module_launch_by_launch(sed):
    """AC, fp32, forward(training=False, keep_for_grad=True): the module's launches only (the other halves do not differ by mode)"""
    conf, kc = "AC", CONF["AC"]["sa_conv_kernel"]
    ck = Checker(conf + " eval", "fp32")
    st = Step(sed, conf, "fp32", training=False)
    for l in reversed(range(CONF[conf]["sa_layers"])):
        ly = {n: f32(v) for n, v in st.g["layers"][l].items()}
        snap, Wc, dWc, run0, run1 = conv_operands(st, l)
        ds = ck.nt_ref(snap["dres"], Wc["pointwise2.weight"].reshape(C, C).T)
        conv_module(ck, st.eng.lib, f"eval l{l}", kc, ly, snap, ds, Wc, dWc, run0, run1, False)
    kinds = {k[2] for k in RATIOS if k[:2] == ck.key}
    assert kinds == (set(CONV_KINDS) - {"sed_bn_train_finalize", "sed_bn_bwd_finalize"}) | set(EVAL_KINDS), kinds


def test_forward_states_of_the_module(sed):
    """v is stored only for a backward; update_running_stats=False changes no bit of the forward and leaves the running buffers alone"""
    x, _ = batch()
    model = make_model(sed, "AC")
    eng, P = model.engine, model._tensor_dict()
    names = [n for n in P if n.startswith("convm") and ".bn.running_" in n]
    before = {n: P[n].clone() for n in names}
    plan = eng.forward(x, P, training=True)
    lys = plan.sa["layers"]
    run = {n: P[n].clone() for n in names}
    assert len(run) == 4 and not any(torch.equal(run[n], before[n]) for n in names), "a training forward updates the running statistics"
    kept = [{n: ly[n].clone() for n in ("cz", "cs", "cv")} for ly in lys]
    assert all(bool(torch.isfinite(k["cv"]).all()) for k in kept)
    for ly in lys:
        ly["cz"].fill_(float("nan"))
        ly["cs"].fill_(float("nan"))
    assert eng.forward(x, P, training=True, update_running_stats=False) is plan
    torch.cuda.synchronize()
    for ly, k in zip(lys, kept):
        assert torch.equal(ly["cz"], k["cz"]) and torch.equal(ly["cs"], k["cs"]), "update_running_stats=False changed the forward's bits"
    for n, v in run.items():
        assert torch.equal(P[n], v), (n, "update_running_stats=False touched a running buffer")
    for ly in lys:
        ly["cv"].fill_(float("nan"))
    assert eng.forward(x, P, training=False) is plan
    torch.cuda.synchronize()
    for ly in lys:
        assert bool(torch.isnan(ly["cv"]).all()), "an eval forward without keep_for_grad stored v"
        assert bool(torch.isfinite(ly["cz"]).all())
    for n, v in run.items():
        assert torch.equal(P[n], v), (n, "an eval forward touched a running buffer")
