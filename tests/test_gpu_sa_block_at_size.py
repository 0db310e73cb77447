"""GPU: the pre-LN / Conformer attention block (heads.SaHead: _plan_chain, _forward_pre, _backward_pre, _mhsa_opts and the _rel / _win /
_drop entries) and the post-LN path with every option composed, through the engine at the multi-head, multi-tile size of
tests/test_gpu_sa_at_size.py -- end to end against float64 and launch by launch against float64.

Geometry, that file's unchanged: CFG = [(32, 2), (64, 2), (128, 2), (128, 1)], 8 mel bins, B = 4 clips of T = 1040 frames, 3 classes,
recall weight 5: C = 128, t = 130 frames per clip, R = 520 rows.
  P   pre-LN: sa_heads 4, 2 layers, FFN of 256 with GELU, positional table.  Layer 0 has no closing norm (the add crosses the layer
      boundary); out_norm closes layer 1.
  M   the Conformer block: pre-LN, macaron, sa_heads 2 (width 64), 2 layers, FFNs of 256 with GELU, sa_conv_kernel 31, window (40, 7),
      log buckets (32, 128), one table per layer, no positional table.
  MD  M plus sa_dropout 0.1 with a fixed seed.
  AR  post-LN (_forward / _backward): configuration A of that file plus sa_conv_kernel 7, window (3, 0), sa_rel_pos 5 and sa_dropout 0.1
      with a fixed seed.  Window (3, 0): a query's first visited key tile lies wholly outside its window.
Biases, the LayerNorm and BatchNorm affine parameters and the running statistics are randomised as that file's make_model does; the
rel_pos* tables are drawn N(0, 1).

What the size exercises, asserted from the library and the engine's plan (size_conditions; none is patched in):
  - sed_mhsa_win_tiles(t, left, right, pass) is 16 (window (40, 7)) and 9 (window (3, 0)) in each pass, below the 25 unwindowed tiles
    per (clip, head): tiles are skipped;
  - sed_mhsa_bwd_rel_ws_floats(B, t, H, dh, left, right) = 11280 (M, MD) and 14368 (AR) exceeds B t H = 1040 / 2080, and g["core_ws"]
    holds it: the per-wave diagonal partials are spread over several workgroups, waves and clips;
  - every weight-gradient sed_gemm_tn runs split-K 2 (the engine's formula max(1, min(ksplit, R // 256))), and g["tn_ws"] covers the
    largest need (in_proj 3C x C; both FFNs C x D, D x C; pointwise1 with M = 2C);
  - sed_resid_layernorm_bwd_ws_floats(R, C) = 9 * 2 * C: 9 partial rows of 64, the last of 8 live rows; g["ln_ws"] holds it;
  - the rows of each layer's rel table differ between heads and between layers.
Buffer sizes are checked by these host-side assertions on numel() alone.

a. End to end, fp32: tests/test_gpu_sa_preln.py's compare at this geometry.  The conv-stack output of a head='none' engine on the same
parameters feeds preln_formula.encoder (P, M, MD) or relpos_formula.encoder (AR) with H heads, the window, the table configuration and the
dropout state words read before the forward, then the linear layer, repeat_interleave and the weighted BCE; the oracle's feature
gradient goes back through the bare engine's backward.  Both stacks are checked on the host against torch with several heads, a window
and tables together (tests/test_preln_host.py, tests/test_relpos_host.py).  The project's bounds: logits 1e-3 absolute, loss 1e-4, every
parameter gradient 3e-3 relative L2, depthwise.bias by tests/test_gpu_sa_conformer.py's rule, running statistics 1e-4 relative L2 and the
counter + 1.  P, M, MD, AR in training mode; M also in eval mode (an eval forward kept for the gradient, the eval backward; running
statistics and counters keep their bits); an eval forward of MD is M's bit for bit on the same parameters; for MD and AR the oracle with
the masks is inside the bounds, the oracle with p = 0 more than 1e-2 outside, and the step word advances by exactly one.

b. Launch by launch, fp32 and bf16: one training forward, the loss, one backward per configuration.  The instance's eng._k is wrapped
for the backward: in front of and behind EVERY launch, on the stream, the shared gradient buffers of plan.sa (dh, dn, ds[0], ds[1], da,
dres, dctx, dqkv, dm, fda, ffa, dh1, dhc, cds, cdg, ccoef, cbpart -- those the configuration has) are cloned.  So each is intact where it is
read: the clone behind launch i holds what launch i wrote, before anything else runs; the clone in front of launch i holds what launch i
read, the torch adds of the post-LN path between two launches included (each is bit-equal to the fp32 sum); in particular the in-place
stream gradient exists before and after each sed_resid_layernorm_bwd, and the product fda before sed_ffn_act_bwd overwrites it, cds
before sed_bn_silu_bwd_reduce does.  What a forward
launch writes (qkv, ctx, lse, a, u, f, mu, mf, rel, the module's buffers, every chain node's x, y, stats) and drel are per layer or per
node and written once a step: read after it.  The module's forward partial rows g["cpart"] are shared: the last layer's are checked.
After every sed_resid_layernorm_bwd no shared buffer but its dx (and da) has changed a bit.
Every launch of the head is checked per element, no element left out, against float64 of that ONE operation on the engine's own
inputs to it (rounded to bf16 where the kernel rounds them):
  sed_resid_layernorm_fwd / _bwd   every chain node of P, M, MD, those without an add and the closing norms too: preln_formula.
                  resid_layernorm / resid_layernorm_gates on the engine's src, a, s (1 or 1/2) and keep_rows(state, 8 la + site, R, C, p);
                  xsum, y, the mean; backward on the engine's gy, the stream gradient before the launch as dres_in, x and stats: dx, da
                  (where s != 1 or dropout), dgamma, dbeta
  sed_mhsa_fwd_rel / _bwd_rel (M, MD, AR), sed_mhsa_fwd / _bwd (P)   relpos_formula.core / core_gates (mhsa_formula's for P) on the
                  thirds of the engine's qkv, its expanded rel, the window, keep_attn(state, 8 l, B, H, t, p) and s = 1 / (1 - p); the
                  backward teacher-forced on the engine's ctx, lse, dctx (raw_dctx gates in bf16); drel on all H (2t - 1) diagonals, those
                  no window reaches exactly 0
  sed_relpos_expand   bit-equal to w[g][map[x]];   sed_relpos_fold   relpos_formula.fold of the engine's own drel, core_gates' dw gate
  sed_ffn_fwd[_drop], sed_ffn_act_bwd[_drop]   dropout_formula.ffn / ffn_gates / act_bwd_gates (ffn_formula's for p = 0), hidden streams
                  8 l + 3 (FFN) and 8 l + 5 (macaron FFN); the activation backward on the engine's own da
  sed_add_layernorm_fwd_drop / _bwd_drop (AR)   dropout_formula.add_layernorm / add_layernorm_gates, the statistics within
                  tests/test_gpu_mhsa.py's gates
  sed_gemm_nt / sed_gemm_tn   every projection, input gradient, weight gradient and (column sums) bias gradient, the macaron FFNs'
                  included: tests/test_gpu_sa_at_size.py's Checker (SAFE (K + 1 + [bias]) u S; gemm_tn and colsum gates, ksplit = 2)
  the convolution module   inside the chain (M, MD) and behind attn_norm (AR): that file's conv_module on n["y"] / h as its input
sed_mel_mean_*, sed_head_*, sed_transpose_shift and the conv stack are pinned elsewhere; their outputs are taken as given.
Run with -s for the worst error / gate per configuration, precision and launch kind.

Measured on the MI355X (-s):
  end to end (fp32)    logits     loss       worst gradient (relative L2)   depthwise.bias / |d weight|   running statistics
    P                  2.2e-6     6.7e-8     1.1e-6
    M                  2.1e-6     4.8e-8     2.4e-6                         5.5e-7                        4.7e-8
    MD                 2.0e-6     2.4e-8     2.9e-6                         5.8e-7                        5.0e-8     p = 0: 1.5 away
    AR                 2.7e-6     1.6e-7     3.2e-6                         1.3e-6                        4.3e-8     p = 0: 1.8 away
    M eval             2.0e-6     5.6e-8     1.9e-6                         (8.1e-8 relative L2)          every bit kept
  The project's bounds hold at this size with more than two decades to spare; none was derived anew.
  launch by launch, worst error / gate        P fp32   P bf16   M fp32   M bf16   MD fp32  MD bf16  AR fp32  AR bf16
    sed_resid_layernorm_fwd                   0.50     0.50     0.50     0.50     0.50     0.50
    sed_resid_layernorm_bwd                   0.035    0.032    0.093    0.11     0.11     0.11
    sed_add_layernorm_fwd_drop                                                                      0.011    0.012
    sed_add_layernorm_bwd_drop                                                                      0.013    0.013
    sed_mhsa_fwd / _fwd_rel                   0.029    0.21     0.019    0.53     0.017    0.64     0.033    0.92
    sed_mhsa_bwd / _bwd_rel                   0.048    0.28     0.036    0.74     0.028    0.81     0.099    0.96
    sed_relpos_fold                                             1.0e-5   7.6e-8   7.6e-6   1.0e-7   0        0
    sed_ffn_fwd[_drop]                        0.036    0.46     0.034    0.39     0.035    0.37     0.032    0.39
    sed_ffn_act_bwd[_drop]                    0.029    0.028    0.035    0.041    0.030    0.038    0.030    0.032
    sed_gemm_nt                               0.012    0.0034   0.0090   0.0033   0.014    0.0033   0.011    0.0038
    sed_gemm_tn (split-K 2)                   0.010    0.0041   0.010    0.0027   0.0071   0.0031   0.0080   0.0034
    sed_gemm_tn column sums                   0.014    0.013    0.012    0.013    0.012    0.011    0.013    0.011
    sed_dwconv_glu_fwd                                          0.060    0.064    0.065    0.074    0.15     0.17
    sed_bn_train_finalize                                       0.62     0.61     0.58     0.63     0.64     0.64
    sed_bn_silu_fwd                                             0.065    0.063    0.071    0.070    0.063    0.068
    sed_bn_silu_bwd_reduce (through the GEMM's gate)            0.0086   0.0039   0.0075   0.0042   0.0076   0.0034
    sed_bn_bwd_finalize                                         0.24     0.25     0.25     0.25     0.24     0.24
    sed_dwconv_glu_bwd                                          0.079    0.073    0.073    0.067    0.10     0.11
  sed_relpos_expand is bit-equal everywhere.  xsum sits at 0.50 by construction (one rounding against a gate of two); AR's fold is exact
  because under window (3, 0) with L = 5 every bucket that is reached holds one distance.  The windowed bf16 core stands close to its gate:
  a row of window (3, 0) has at most four keys, so nothing averages and the operand roundings of p~ and dctx arrive near their worst case.
One gate was wrong, neither the kernel nor the engine: at first AR bf16 missed sed_mhsa_bwd_rel's dv gate at 1.19 (layer 1; M and MD stood at
0.75 and 0.84 against 0.28 unwindowed).  The raw-dctx term the formula modules add in bf16 for a dctx the kernel rounds as an MFMA operand was
capped at 2^-9 of its absolute-value form, the half ulp at the TOP of a binade; the half ulp of 8 significant bits reaches 2^-8 at the bottom,
and the last key of a clip has ONE query under window (3, 0), whose dv is moved by that whole rounding.  A float64 emulation of the documented
nearest-even rounding with exact accumulation missed the same gate at 1.24 (tests/test_relpos_host.py holds it now).  window_formula /
relpos_formula cap at 2^-8 with the derivation in their docstrings; where the shift lies below the 2^-9 form -- every sum of more than a few
terms, all earlier tests -- the gate is the number it was.  mhsa_formula (unwindowed, sums over all t keys) is left as it is.
Tried against local edits of heads.py, each once, none committed, every access in bounds (failing tests of this file; beside them the tiny
configurations of tests/test_gpu_sa_preln.py, its fp32 and dropout tests):
  - the macaron FFN's backward regenerates its hidden mask from stream 8 l + 3 instead of 8 l + 5: MD fails end to end
    (ffn_mac_l1.linear1.weight 0.12 relative L2) and launch by launch at "ffn_mac_l1 a" of sed_ffn_act_bwd_drop (6.6e4 gates out, fp32 and
    bf16); P, M, AR pass (no dropout, or no macaron); the tiny Conformer dropout test fails too (0.48);
  - _backward_pre passes s = 1.0 for the half-step adds: M, MD and M eval fail end to end (ffn_l1.linear1.weight 1.0: twice the gradient)
    and launch by launch at "out_norm_l1 da" (7.7e4 gates out); P and AR pass (no half step); the tiny Conformer tests fail too (1.0);
  - layer 0's rel table passed to layer 1's core backward: M, MD, AR and M eval fail end to end (rel_pos_l1.weight 0.87 / 0.90 / 1.2 on
    attn_l1.in_proj_weight / 1.0) and launch by launch at "attn_l1 dq" (1.5e4 gates out in fp32, 64 in bf16; AR 3.1e5 and 516); the tiny
    Conformer tests fail too, by less (0.25 and 0.12: tables of N(0, 0.1));
  - ga taken from dx where da is due: M, MD and M eval fail end to end (ffn_l1.linear1.weight 1.0) and launch by launch at
    "ffn_l1 da (hidden)" of sed_gemm_nt (1.5e4 / 1.9e4 gates out); P and AR pass; all three tiny tests with a da fail too (0.29 -- 1.0);
  - the closing-norm buffer flip removed (dx may be the buffer gy is): M, MD and M eval fail end to end (out_norm.weight 0.64, 0.62, 1.3:
    layer 0's closing norm reads its dy from the buffer it writes) and launch by launch at the first closing norm; P has one closing norm
    and computes the same numbers (end to end passes) -- its launch-by-launch test fails only because it reads dx from ds[1], where the
    engine no longer writes it; the tiny Conformer tests fail too (0.43, 0.38).
So at this size no edit is caught that the tiny Conformer configuration misses; what the size adds is where: each edit fails at the launch
it breaks, by four decades, and the head count, the tiles, the workspace and the partial rows above are now under a test at all.
"""
import importlib

import numpy as np
import pytest
import torch

import dropout_formula as DF
import ffn_formula as FF
import mhsa_formula as F
import preln_formula as PF
import relpos_formula as RF
import test_gpu_sa_at_size as AS
import test_gpu_sa_model as T0
import test_gpu_sa_preln as PL

pytestmark = pytest.mark.gpu
PKG = AS.PKG
CFG, MEL, T, B, K, W = AS.CFG, AS.MEL, AS.T, AS.B, AS.K, AS.W
C, t, R = AS.C, AS.t, AS.R
U, KS = AS.U, AS.KS
D = 256
SEED = 0x0123456789ABCDEF
CONF = {"P": dict(sa_norm_first=True, sa_heads=4, sa_layers=2, sa_ffn=D, sa_activation="gelu", pos_encoding=True),
        "M": dict(sa_norm_first=True, sa_macaron=True, sa_heads=2, sa_layers=2, sa_ffn=D, sa_activation="gelu", sa_conv_kernel=31,
                  sa_window=(40, 7), sa_rel_pos=(32, 128), pos_encoding=False)}
CONF["MD"] = dict(CONF["M"], sa_dropout=0.1, sa_dropout_seed=SEED)
CONF["AR"] = dict(AS.CONF["A"], sa_norm_first=False, sa_conv_kernel=7, sa_window=(3, 0), sa_rel_pos=5, sa_dropout=0.1, sa_dropout_seed=SEED)
SHARED = ("dh", "dn", "ds0", "ds1", "da", "dres", "dctx", "dqkv", "dm", "fda", "ffa", "dh1", "dhc", "cds", "cdg", "ccoef", "cbpart")
RATIOS = {}                     # (configuration, precision, launch kind) -> worst error / gate
f32, f64, rel_l2, batch = AS.f32, AS.f64, T0.rel_l2, AS.batch


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
            print(f"  {k[0]:3s} {k[1]:5s} {k[2]:28s} {RATIOS[k]:.3e}")


def make_model(sed, conf, precision="fp32", seed=0):
    torch.manual_seed(seed)
    m = sed.Csa_AvgPooling(K, CFG, precision=precision, mel_bins=MEL, **CONF[conf])
    with torch.no_grad():       # as tests/test_gpu_sa_at_size.py: zero / unit initial values would hide a wrong bias, affine or table gradient
        for n, p in m.named_parameters():
            if n.startswith(PL.HEAD):
                if ("norm" in n or ".bn." in n) and n.endswith("weight"):
                    p.normal_(1.0, 0.2)
                elif n.endswith("bias"):
                    p.normal_(0.0, 0.1)
                elif n.startswith("rel_pos"):
                    p.normal_(0.0, 1.0)
        for n, b in m.named_buffers():
            if n.startswith("convm") and n.endswith("running_mean"):
                b.normal_(0.0, 0.2)
            if n.startswith("convm") and n.endswith("running_var"):
                b.uniform_(0.5, 1.5)
    return m.cuda()


def drop_of(cf):
    """(p, sd): the probability and the fp32 scale 1 / (1 - p) as float; (0, 1) without dropout"""
    p = cf.get("sa_dropout", 0.0)
    return p, (float(DF.thr_scale(p)[1]) if p else 1.0)


def size_conditions(eng, g, conf):
    """what R = 520, t = 130 make happen in the head's launches (module docstring), from the library and the engine's plan"""
    cf, lib = CONF[conf], eng.lib
    H, kc = cf["sa_heads"], cf.get("sa_conv_kernel", 0)
    assert g["R"] == R and len(g["layers"]) == cf["sa_layers"]
    assert ("sa_window" in cf) == (eng.head_impl._win is not None)
    if "sa_window" in cf:
        left, right = cf["sa_window"]
        assert eng.head_impl._win == (left, right)
        full = (-(-t // 32)) ** 2
        assert full == 25
        for which in (0, 1, 2):
            n = lib.sed_mhsa_win_tiles(t, left, right, which)
            assert 0 < n < full, (conf, which, n, "the window skips no tile")
    if "sa_rel_pos" in cf:
        need = lib.sed_mhsa_bwd_rel_ws_floats(B, t, H, C // H, *cf["sa_window"])
        assert need > B * t * H and g["core_ws"].numel() >= need, (need, g["core_ws"].numel())
    else:
        assert g["core_ws"].numel() >= lib.sed_mhsa_bwd_ws_floats(B, t, H, C // H) == B * t * H
    assert max(1, min(g["ksplit"], R // 256)) == KS, "the weight-gradient products of this size are meant to run split-K 2"
    need = [lib.sed_gemm_tn_ws_floats(3 * C, C, KS), lib.sed_gemm_tn_ws_floats(C, D, KS), lib.sed_gemm_tn_ws_floats(D, C, KS)] \
        + ([lib.sed_gemm_tn_ws_floats(2 * C, C, KS)] if kc else [])
    assert g["tn_ws"].numel() >= max(need) and need[0] == KS * (3 * C * C + 3 * C), "g['tn_ws'] is smaller than a split-K launch needs"
    ws_floats = lib.sed_resid_layernorm_bwd_ws_floats if cf["sa_norm_first"] else lib.sed_add_layernorm_bwd_ws_floats
    assert ws_floats(R, C) == 9 * 2 * C and -(-R // 64) == 9 and R - 8 * 64 == 8 and g["ln_ws"].numel() >= 9 * 2 * C


# ---- a. fp32, end to end ---------------------------------------------------------------------------------------------------------------
def stack_of(conf):
    """what PL.compare takes as `encoder`: None for the pre-LN configurations (preln_formula.encoder on the options), for AR
    relpos_formula.encoder's post-LN stack with the module, as a function of the state words and p"""
    cf = CONF[conf]
    if cf["sa_norm_first"]:
        return None

    def make(state, p):
        return lambda x, Wn, Bc, tt, H, dh_out=None: RF.encoder(
            x, Wn, cf["sa_rel_pos"], Bc, tt, H, *cf["sa_window"], state=state, p=p, layers=cf["sa_layers"], ffn_width=cf["sa_ffn"],
            act=cf["sa_activation"], pos_encoding=False, conv=True, dh_out=dh_out)
    return make


def end_to_end(sed, conf, training=True):
    cf = CONF[conf]
    p = cf.get("sa_dropout", 0.0)
    model = make_model(sed, conf)
    stack = stack_of(conf)
    step0 = model.engine.drop_state_words()
    out, (sd0, feat, y64, state, ratio) = PL.compare(sed, model, cf, p if training else 0.0, xy=batch(), cfg=CFG, mel=MEL, heads=cf["sa_heads"],
                                                     training=training, encoder=None if stack is None else (lambda st: stack(st, p)))
    plan = T0.the_plan(model)
    assert plan.sa["R"] == R and plan.t_out == t and feat.shape == (B, t, 1, C)
    assert state == step0
    return model, out, (sd0, feat, y64, state, ratio)


@pytest.mark.parametrize("conf", ["P", "M", "MD", "AR"])
def test_fp32_model_matches_the_float64_oracle_at_size(sed, conf):
    cf = CONF[conf]
    model, out, (sd0, feat, y64, state, ratio) = end_to_end(sed, conf)
    words = model.engine.drop_state_words()
    if "sa_dropout" not in cf:
        assert words == state
        return
    # the masks are seen: the oracle without them is far outside, and the next forward draws new ones
    assert state == [SEED & 0xFFFFFFFF, SEED >> 32, 0, 0] and words == state[:2] + [1, 0], "a training forward advances the step word by one"
    stack = stack_of(conf)
    plain = PL.oracle(sd0, feat, y64, state, 0.0, cf, ratio, True, cf["sa_heads"], None if stack is None else stack(state, 0.0))[0]
    away = float((out.detach().cpu().double() - plain).abs().max())
    print(f"{conf}: the oracle with p = 0 is {away:.3e} away")
    assert away > 1e-2


def test_fp32_conformer_block_in_eval_mode_at_size(sed):
    """M: an eval forward kept for the gradient and the eval-mode backward against the oracle in eval mode (the running statistics in
    the BatchNorm, sed_bn_eval_*); every running statistic and counter keeps its bits (PL.compare)"""
    end_to_end(sed, "M", training=False)


def test_an_eval_forward_never_drops(sed):
    """MD and M hold the same parameters (the dropout options draw nothing): their eval forwards agree bit for bit"""
    x, _ = batch()
    m, md = make_model(sed, "M").eval(), make_model(sed, "MD").eval()
    sm, smd = m.state_dict(), md.state_dict()
    assert all(torch.equal(sm[n], smd[n]) for n in sm if "config" not in n) and set(sm) == set(smd)
    with torch.no_grad():
        a, b = m(x), md(x)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert md.engine.drop_state_words()[2] == 0, "an eval forward advanced the step word"


# ---- b. launch by launch ---------------------------------------------------------------------------------------------------------------
class Checker(AS.Checker):
    def ok(self, kind, what, got, ref, gate):
        good, worst = F.check(got, ref, gate, self.key + (kind, what))
        k = self.key + (kind,)
        RATIOS[k] = max(RATIOS.get(k, 0.0), worst)
        assert good, (self.key, kind, what, worst)


class Step:
    """One training forward, the loss and one backward of a configuration through its engine; eng._k of the instance is wrapped for
    the backward and clones the shared gradient buffers of plan.sa in front of and behind every launch (module docstring).  launches[i] is the
    name of launch i; before(i, buf) / after(i, buf) the buffer as launch i found and left it."""

    def __init__(self, sed, conf, precision):
        cf = CONF[conf]
        x, y = batch()
        self.model = model = make_model(sed, conf, precision).train()
        self.eng, self.P = eng, P = model.engine, model._tensor_dict()
        self.G = G = {n: torch.full_like(p, float("nan")) for n, p in model.named_parameters()}
        self.run0 = {n: f32(v) for n, v in P.items() if n.startswith("convm") and ".bn.running_" in n}       # before the step
        self.state = eng.drop_state_words()
        self.plan = plan = eng.forward(x, P, training=True)
        eng.loss_and_grad(plan, y, W)
        self.g = g = plan.sa
        assert plan.t_out == t
        size_conditions(eng, g, conf)
        self.bufs = bufs = {n: (g["ds"][int(n[2])] if n in ("ds0", "ds1") else g[n]) for n in SHARED if (n in ("ds0", "ds1") and "ds" in g) or n in g}
        assert ("dn" in bufs) == cf["sa_norm_first"] and ("cds" in bufs) == bool(cf.get("sa_conv_kernel")) and ("da" in bufs) == (
            "sa_dropout" in cf or cf.get("sa_macaron", False))
        for v in bufs.values():
            v.fill_(float("nan"))
        self.launches, self.pre, self.post = launches, pre, post = [], [], []
        clones = lambda: {n: v.clone() for n, v in bufs.items()}
        inner, live = eng._k, [True]

        def k(name, fn, *args):         # on the current stream: the clones are ordered around this launch, behind the last and before the next
            if live[0]:
                pre.append(clones())
            inner(name, fn, *args)
            if live[0]:
                launches.append(name)
                post.append(clones())
                live[0] = name != "sed_mel_mean_bwd"

        eng._k = k
        try:
            eng.backward(plan, P, G)
        finally:
            del eng._k
        torch.cuda.synchronize()
        assert launches.count("sed_head_bwd") == 1 and launches[-1] == "sed_mel_mean_bwd" and not live[0] and len(pre) == len(post) == len(launches)
        self.head_bwd = launches.index("sed_head_bwd")
        self.i = self.head_bwd + 1      # the next launch to account for
        self._np = {}

    def _get(self, snaps, j, buf):
        key = (id(snaps), j, buf)
        if key not in self._np:
            self._np[key] = f32(snaps[j][buf])
        return self._np[key]

    def before(self, i, buf):
        return self._get(self.pre, i, buf)

    def after(self, i, buf):
        return self._get(self.post, i, buf)

    def take(self, name):
        """the index of the next launch, which must be `name` (transposes of a weight, pinned elsewhere, are passed over)"""
        while self.launches[self.i] == "sed_transpose_shift":
            self.i += 1
        assert self.launches[self.i] == name, (self.i, self.launches[self.i], name)
        self.i += 1
        return self.i - 1

    def only_changed(self, i, names):
        """launch i changed no bit of a shared buffer outside `names`"""
        for n in self.bufs:
            if n not in names:
                a, b = self.pre[i][n], self.post[i][n]
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (self.launches[i], i, n, "a buffer the launch does not own changed")


class Head:
    """the checks of one Step, shared by the pre-LN chain and the post-LN path"""

    def __init__(self, sed, conf, precision):
        self.conf, self.cf = conf, CONF[conf]
        cf = self.cf
        self.H, self.layers, self.act, self.kc = cf["sa_heads"], cf["sa_layers"], cf["sa_activation"], cf.get("sa_conv_kernel", 0)
        self.dh = C // self.H
        self.p, self.sd = drop_of(cf)
        self.ck = Checker(conf, precision)
        self.st = st = Step(sed, conf, precision)
        self.eng, self.g, self.state = st.eng, st.g, st.state
        mine = PL.HEAD
        self.Pn = {n: f32(v) for n, v in st.P.items() if n.startswith(mine) and v.is_floating_point()}
        self.Gn = {n: f32(v) for n, v in st.G.items() if n.startswith(mine)}
        assert all(np.isfinite(v).all() for v in self.Gn.values())
        self.win = cf.get("sa_window")
        self.rel_cfg = cf.get("sa_rel_pos")
        if self.rel_cfg is not None:
            tabs = [self.Pn[RF.rel_name(l) + ".weight"] for l in range(self.layers)]
            assert all(tb.shape == (self.H, RF.num_buckets(self.rel_cfg)) for tb in tabs)
            for l, tb in enumerate(tabs):
                assert all(not np.array_equal(tb[a], tb[b]) for a in range(self.H) for b in range(a)), "two heads share a table row"
                assert all(not np.array_equal(tb[a], o[b]) for o in tabs[:l] for a in range(self.H) for b in range(self.H)), "two layers share a row"
            mp = self.g["rel_map"].cpu().numpy()
            assert np.array_equal(mp, RF.bucket_map(self.rel_cfg, t))
            self.map = mp

    # ---- masks --------------------------------------------------------------------------------------------------------------------
    def rows(self, stream, N):
        return DF.keep_rows(self.state, stream, R, N, self.p) if self.p else None

    # ---- attention ------------------------------------------------------------------------------------------------------------------
    def attention_forward(self, tag, l, ly, xin, mod):
        ck, Pn, H, dh = self.ck, self.Pn, self.H, self.dh
        Win, bin_, Wout, bout = (Pn[mod + s] for s in (".in_proj_weight", ".in_proj_bias", ".out_proj.weight", ".out_proj.bias"))
        ck.nt(tag + " qkv", ly["qkv"], xin, Win, bin_)
        if self.rel_cfg is not None:
            w = Pn[RF.rel_name(l) + ".weight"]
            assert np.array_equal(ly["rel"].view(np.uint32), w[:, self.map].view(np.uint32)), (tag, "the expanded table is not w[g][map[x]]")
            k = ck.key + ("sed_relpos_expand",)
            RATIOS[k] = 0.0
        ck.nt(tag + " a", ly["a"], ly["ctx"], Wout, bout)

    def core(self, tag, l, ly, dctx, dqkv):
        """the forward and the teacher-forced backward of layer l's core on the engine's qkv, ctx, lse and dctx"""
        ck, H, dh = self.ck, self.H, self.dh
        qkv_op = F.round_bf16(ly["qkv"]) if ck.mode == "bf16" else ly["qkv"]
        q, k, v = F.split_qkv(qkv_op, B, t, H, dh)
        d4, ctx4 = dctx.reshape(B, t, H, dh), ly["ctx"].reshape(B, t, H, dh)
        raw = ck.mode == "bf16"
        if self.rel_cfg is None and self.win is None and not self.p:
            sfx = ""
            cr = F.core(q, k, v, d4, lse=ly["lse"], ctx=ctx4)
            cg = F.core_gates(q, k, v, d4, ck.mode, raw_dctx=raw, lse=ly["lse"], ctx=ctx4)
        else:
            assert self.rel_cfg is not None
            sfx = "_rel"
            left, right = self.win
            ka = DF.keep_attn(self.state, DF.stream_id(l, DF.SITE_ATTN), B, H, t, self.p) if self.p else None
            kw = dict(keep=ka, s=self.sd, lse=ly["lse"], ctx=ctx4, cfg=self.rel_cfg)
            cr = RF.core(q, k, v, ly["rel"], left, right, d4, **kw)
            cg = RF.core_gates(q, k, v, ly["rel"], left, right, d4, mode=ck.mode, raw_dctx=raw, **kw)
        ck.ok("sed_mhsa_fwd" + sfx, tag + " ctx", ctx4, cr["ctx"], cg["ctx"])
        ck.ok("sed_mhsa_fwd" + sfx, tag + " lse", ly["lse"], cr["lse"], cg["lse"])
        for name, got in zip(("dq", "dk", "dv"), F.split_qkv(dqkv, B, t, H, dh)):
            ck.ok("sed_mhsa_bwd" + sfx, tag + " " + name, got, cr[name], cg[name])
        if sfx:
            drel = ly["drel"]
            assert drel.shape == (H, 2 * t - 1)
            ck.ok("sed_mhsa_bwd_rel", tag + " drel", drel, cr["drel"], cg["drel"])
            d = np.arange(-(t - 1), t)
            out = (d < -left) | (d > right)
            assert out.any() and not drel[:, out].any(), (tag, "a diagonal no window reaches is not exactly 0")
            return cg["dw"]
        return None

    def attention_backward(self, tag, l, ly, mod, xin, ga, dx_name):
        """ga: the gradient of the sub-layer's output a -> the gradient of xin through the projections, left in the shared buffer dx_name
        (without the residual branch); returns (that product, the index of its launch)"""
        st, ck, Pn, Gn = self.st, self.ck, self.Pn, self.Gn
        Win, Wout = Pn[mod + ".in_proj_weight"], Pn[mod + ".out_proj.weight"]
        sfx = "_rel" if self.rel_cfg is not None else ""
        st.take("sed_gemm_tn")
        ck.tn(tag + " out_proj", Gn[mod + ".out_proj.weight"], Gn[mod + ".out_proj.bias"], ga, ly["ctx"])
        i = st.take("sed_gemm_nt")
        dctx = st.after(i, "dctx")
        ck.nt(tag + " dctx", dctx, ga, Wout.T)
        i = st.take("sed_mhsa_bwd" + sfx)
        dqkv = st.after(i, "dqkv")
        dw_gate = self.core(tag, l, ly, dctx, dqkv)
        if sfx:
            st.take("sed_relpos_fold")
            ck.ok("sed_relpos_fold", tag + " dw", Gn[RF.rel_name(l) + ".weight"], RF.fold(ly["drel"], self.rel_cfg, t), dw_gate)
        st.take("sed_gemm_tn")
        ck.tn(tag + " in_proj", Gn[mod + ".in_proj_weight"], Gn[mod + ".in_proj_bias"], dqkv, xin)
        i = st.take("sed_gemm_nt")
        prod = st.after(i, dx_name)
        ck.nt(tag + " d input (attention)", prod, dqkv, Win.T)
        return prod, i

    # ---- FFN --------------------------------------------------------------------------------------------------------------------------
    def ffn_forward(self, tag, mod, xin, u, f, stream):
        ck, Pn = self.ck, self.Pn
        w1, b1, w2, b2 = (Pn[mod + s] for s in (".linear1.weight", ".linear1.bias", ".linear2.weight", ".linear2.bias"))
        if self.p:
            kh = self.rows(stream, D)
            fr = DF.ffn(xin, w1, b1, w2, b2, self.act, kh, self.sd)
            fg = DF.ffn_gates(xin, w1, b1, w2, b2, self.act, kh, self.sd, mode=ck.mode)
            kind = "sed_ffn_fwd_drop"
        else:
            fr = FF.ffn(xin, w1, b1, w2, b2, self.act)
            fg = FF.ffn_gates(xin, w1, b1, w2, b2, self.act, mode=ck.mode)
            kind = "sed_ffn_fwd"
        ck.ok(kind, tag + " u", u, fr["u"], fg["u"])
        ck.ok(kind, tag + " f", f, fr["y"], fg["y"])

    def ffn_backward(self, tag, mod, xin, u, ga, stream, dx_name):
        """ga: the gradient of the FFN's output -> the product du . w1 left in dx_name; returns (it, the index of its launch)"""
        st, ck, Pn, Gn = self.st, self.ck, self.Pn, self.Gn
        w1, w2 = Pn[mod + ".linear1.weight"], Pn[mod + ".linear2.weight"]
        i = st.take("sed_gemm_nt")
        da = st.after(i, "fda")                              # before the activation backward overwrites it with du
        ck.nt(tag + " da (hidden)", da, ga, w2.T)
        kind = "sed_ffn_act_bwd_drop" if self.p else "sed_ffn_act_bwd"
        i = st.take(kind)
        a_hid, du = st.after(i, "ffa"), st.after(i, "fda")
        u64 = f64(u)
        if self.p:
            kh = self.rows(stream, D)
            ms = kh.astype(np.float64) * self.sd
            ag = DF.act_bwd_gates(u, da, self.act, kh, self.sd)
        else:
            ms = 1.0
            ag = FF.act_bwd_gates(u, da, self.act)
        ck.ok(kind, tag + " a", a_hid, ms * FF.act_fwd(u64, self.act), ag["a"])
        ck.ok(kind, tag + " du", du, f64(da) * ms * FF.act_grad(u64, self.act), ag["du"])
        st.take("sed_gemm_tn")
        ck.tn(tag + " linear2", Gn[mod + ".linear2.weight"], Gn[mod + ".linear2.bias"], ga, a_hid)
        st.take("sed_gemm_tn")
        ck.tn(tag + " linear1", Gn[mod + ".linear1.weight"], Gn[mod + ".linear1.bias"], du, xin)
        i = st.take("sed_gemm_nt")
        prod = st.after(i, dx_name)
        ck.nt(tag + " d input (FFN)", prod, du, w1.T)
        return prod, i

    # ---- the convolution module -----------------------------------------------------------------------------------------------------
    def conv_weights(self, l):
        cm = self.eng.sa_conv_names(l)[0]
        Wc = {n[len(cm) + 1:]: f32(v) for n, v in self.st.P.items() if n.startswith(cm + ".") and v.is_floating_point()}
        dWc = {n[len(cm) + 1:]: f32(v) for n, v in self.st.G.items() if n.startswith(cm + ".")}
        run0 = dict(mean=self.st.run0[cm + ".bn.running_mean"], var=self.st.run0[cm + ".bn.running_var"])
        run1 = dict(mean=Wc["bn.running_mean"], var=Wc["bn.running_var"])
        return Wc, dWc, run0, run1

    def conv_forward(self, tag, l, ly, xin):
        Wc = self.conv_weights(l)[0]
        self.ck.nt(tag + " cg", ly["cg"], xin, Wc["pointwise1.weight"].reshape(2 * C, C), Wc["pointwise1.bias"])
        self.ck.nt(tag + " co", ly["co"], ly["cs"], Wc["pointwise2.weight"].reshape(C, C), Wc["pointwise2.bias"])

    def conv_backward(self, tag, l, ly, xin, ga, dx_name):
        """the module's backward (heads.SaHead._conv_inner_backward) and, through tests/test_gpu_sa_at_size.py's conv_module, every vector
        launch of its forward too; ga: the gradient of co -> the product dg . pointwise1.weight left in dx_name"""
        st, ck = self.st, self.ck
        Wc, dWc, run0, run1 = self.conv_weights(l)
        W1, W2 = Wc["pointwise1.weight"].reshape(2 * C, C), Wc["pointwise2.weight"].reshape(C, C)
        i = st.take("sed_gemm_nt")
        ck.nt(tag + " ds", st.after(i, "cds"), ga, W2.T)                 # before sed_bn_silu_bwd_reduce writes gz over it
        st.take("sed_gemm_tn")
        ck.tn(tag + " pointwise2", dWc["pointwise2.weight"].reshape(C, C), dWc["pointwise2.bias"], ga, ly["cs"])
        i = st.take("sed_bn_silu_bwd_reduce")
        snap = dict(cds=st.after(i, "cds"), cbpart=st.after(i, "cbpart"))
        i = st.take("sed_bn_bwd_finalize")
        snap["ccoef"] = st.after(i, "ccoef")
        i = st.take("sed_dwconv_glu_bwd")
        snap["cdg"] = st.after(i, "cdg")
        last = l == self.layers - 1
        AS.conv_module(ck, self.eng.lib, tag, self.kc, ly, snap, ck.nt_ref(ga, W2.T), Wc, dWc, run0, run1, True,
                       cpart=f32(self.g["cpart"])[:12 * 2 * C].reshape(12, 2, C) if last else None)
        st.take("sed_gemm_tn")
        ck.tn(tag + " pointwise1", dWc["pointwise1.weight"].reshape(2 * C, C), dWc["pointwise1.bias"], snap["cdg"], xin)
        i = st.take("sed_gemm_nt")
        prod = st.after(i, dx_name)
        ck.nt(tag + " d input (module)", prod, snap["cdg"], W1.T)
        return prod, i

    def kinds(self):
        return {k[2] for k in RATIOS if k[:2] == self.ck.key}


def pre_ln_launches(sed, conf, precision):
    """P, M, MD: the chain of heads.SaHead._plan_chain forward, then in reverse as _backward_pre walks it"""
    hd = Head(sed, conf, precision)
    st, ck, g, Pn, Gn, cf = hd.st, hd.ck, hd.g, hd.Pn, hd.Gn, hd.cf
    chain = g["chain"]
    macaron = cf.get("sa_macaron", False)
    want = [nm for nm in PF.module_order(hd.layers, macaron, bool(hd.kc), D, hd.rel_cfg is not None) if "norm" in nm]
    assert [n["norm"] for n in chain] == want and g["h"] is chain[-1]["y"]
    assert sum(n["sub"] is None for n in chain) == (hd.layers if macaron else 1)
    assert macaron or (chain[-1]["sub"] is None and chain[2]["add"] is not None and chain[2]["add"][3] == 0 and chain[2]["sub"][2] == 1), "P: the add crosses the layer boundary"
    lys = [{n: f32(v) for n, v in ly.items() if isinstance(v, torch.Tensor)} for ly in g["layers"]]
    nodes = []
    for n in chain:
        a, s, site, la = n["add"] if n["add"] is not None else (None, 1.0, 0, 0)
        nodes.append(dict(norm=n["norm"], src=f32(n["src"]), x=f32(n["x"]), y=f32(n["y"]), stats=f32(n["stats"]), a=None if a is None else f32(a),
                          s=s, stream=8 * la + site, sub=n["sub"], gamma=Pn[n["norm"] + ".weight"], beta=Pn[n["norm"] + ".bias"]))
        assert s == (0.5 if macaron and n["add"] is not None and site in (DF.SITE_FFN_OUT, PF.SITE_MAC_OUT) else 1.0)
    assert np.array_equal(nodes[0]["src"], f32(g["m"])) and nodes[0]["a"] is None
    # ---- forward: every node's LayerNorm (with the add in front of it) and the sub-layer behind it
    for n in nodes:
        tag = n["norm"]
        keep = hd.rows(n["stream"], C) if n["a"] is not None else None
        n["keep"] = keep
        r = PF.resid_layernorm(n["src"], n["a"], n["s"], n["gamma"], n["beta"], keep, hd.sd)
        gt = PF.resid_layernorm_gates(n["src"], n["a"], n["s"], n["gamma"], n["beta"], keep, hd.sd)
        if n["a"] is not None:
            ck.ok("sed_resid_layernorm_fwd", tag + " xsum", n["x"], r["xsum"], gt["xsum"])
        else:
            assert np.array_equal(n["x"], n["src"])
        ck.ok("sed_resid_layernorm_fwd", tag + " y", n["y"], r["y"], gt["y"])
        ck.ok("sed_resid_layernorm_fwd", tag + " mean", n["stats"][:, 0], r["mean"], gt["mean"])
        if n["sub"] is None:
            continue
        kind, mod, l, _ = n["sub"]
        ly = lys[l]
        if kind == "attn":
            hd.attention_forward(mod, l, ly, n["y"], mod)
        elif kind == "conv":
            hd.conv_forward(mod, l, ly, n["y"])
        elif kind == "ffn":
            hd.ffn_forward(mod, mod, n["y"], ly["u"], ly["f"], 8 * l + DF.SITE_FFN_HIDDEN)
        else:
            hd.ffn_forward(mod, mod, n["y"], ly["mu"], ly["mf"], 8 * l + PF.SITE_MAC_HIDDEN)
    # ---- backward: the chain in reverse.  gy: the gradient of the node's y; gs: the running stream gradient
    gy_name, gs_name, ga_name, flip = "dh", None, None, 0
    for n in reversed(nodes):
        tag = n["norm"]
        if n["sub"] is not None:
            kind, mod, l, _ = n["sub"]
            ly = lys[l]
            ga = st.before(st.i, ga_name)              # the gradient of the sub-layer's output, as its first launch finds it
            if kind == "attn":
                hd.attention_backward(mod, l, ly, mod, n["y"], ga, "dn")
            elif kind == "conv":
                hd.conv_backward(mod, l, ly, n["y"], ga, "dn")
            elif kind == "ffn":
                hd.ffn_backward(mod, mod, n["y"], ly["u"], ga, 8 * l + DF.SITE_FFN_HIDDEN, "dn")
            else:
                hd.ffn_backward(mod, mod, n["y"], ly["mu"], ga, 8 * l + PF.SITE_MAC_HIDDEN, "dn")
            gy_name = "dn"
        else:
            gy_name, gs_name = (gs_name if gs_name is not None else gy_name), None
        if gs_name is None:
            flip ^= 1
            dx_name = f"ds{flip}"
        else:
            dx_name = gs_name
        assert dx_name != gy_name
        has_da = n["a"] is not None and (bool(hd.p) or n["s"] != 1.0)
        i = st.take("sed_resid_layernorm_bwd")
        gy = st.before(i, gy_name)
        dres_in = st.before(i, gs_name) if gs_name is not None else None
        assert np.isfinite(gy).all() and (dres_in is None or np.isfinite(dres_in).all())
        keep = n["keep"] if has_da else None
        a_in, s_in = (n["a"], n["s"]) if n["a"] is not None else (None, 1.0)
        rb = PF.resid_layernorm(n["src"], a_in, s_in, n["gamma"], n["beta"], keep, hd.sd, gy, dres_in, xsum=n["x"], stats=n["stats"])
        gb = PF.resid_layernorm_gates(n["src"], a_in, s_in, n["gamma"], n["beta"], keep, hd.sd, gy, dres_in, xsum=n["x"], stats=n["stats"])
        ck.ok("sed_resid_layernorm_bwd", tag + " dx", st.after(i, dx_name), rb["dxsum"], gb["dxsum"])
        if has_da:
            ck.ok("sed_resid_layernorm_bwd", tag + " da", st.after(i, "da"), rb["da"], gb["da"])
        ck.ok("sed_resid_layernorm_bwd", tag + " dgamma", Gn[n["norm"] + ".weight"], rb["dgamma"], gb["dgamma"])
        ck.ok("sed_resid_layernorm_bwd", tag + " dbeta", Gn[n["norm"] + ".bias"], rb["dbeta"], gb["dbeta"])
        st.only_changed(i, {dx_name} | ({"da"} if has_da else set()))
        gs_name = dx_name
        ga_name = "da" if has_da else dx_name
    i = st.take("sed_mel_mean_bwd")
    assert i == len(st.launches) - 1
    kinds = hd.kinds()
    want = {"sed_gemm_nt", "sed_gemm_tn", "sed_gemm_tn colsum", "sed_resid_layernorm_fwd", "sed_resid_layernorm_bwd"}
    want |= {"sed_mhsa_fwd_rel", "sed_mhsa_bwd_rel", "sed_relpos_expand", "sed_relpos_fold"} if hd.rel_cfg is not None else {"sed_mhsa_fwd", "sed_mhsa_bwd"}
    want |= {"sed_ffn_fwd_drop", "sed_ffn_act_bwd_drop"} if hd.p else {"sed_ffn_fwd", "sed_ffn_act_bwd"}
    want |= set(AS.CONV_KINDS) if hd.kc else set()
    assert kinds == want, kinds ^ want


def post_ln_launches(sed, conf, precision):
    """AR: heads.SaHead._forward / _backward with the module, the window, the table and dropout composed"""
    hd = Head(sed, conf, precision)
    st, ck, g, Pn, Gn, eng = hd.st, hd.ck, hd.g, hd.Pn, hd.Gn, hd.eng
    assert hd.p and hd.kc and hd.rel_cfg is not None
    lys = [{n: f32(v) for n, v in ly.items() if isinstance(v, torch.Tensor)} for ly in g["layers"]]
    k_ln = (C + 8) * U

    def layernorm(tag, xin, a, stream, norm, dy, y_got, stats_got, i):
        """the residual LayerNorm under dropout stream `stream`, forward, and backward at launch i -> (dres, da)"""
        keep, gamma, beta = hd.rows(stream, C), Pn[norm + ".weight"], Pn[norm + ".bias"]
        r = DF.add_layernorm(xin, a, keep, hd.sd, gamma, beta, dy, stats=stats_got)
        gt = DF.add_layernorm_gates(xin, a, keep, hd.sd, gamma, beta, dy, stats=stats_got)
        ck.ok("sed_add_layernorm_fwd_drop", tag + " y", y_got, r["y"], gt["y"])
        z = r["z"]
        Mz = np.abs(z).mean(axis=1)
        d = np.abs(z - r["mean"][:, None])
        ck.ok("sed_add_layernorm_fwd_drop", tag + " mean", stats_got[:, 0], r["mean"], k_ln * Mz)
        ck.ok("sed_add_layernorm_fwd_drop", tag + " rstd", stats_got[:, 1], r["rstd"],
              k_ln * r["rstd"] * (1.0 + r["rstd"] ** 2 * (d * (np.abs(z) + Mz[:, None])).mean(axis=1)))
        dres, da = st.after(i, "dres"), st.after(i, "da")
        ck.ok("sed_add_layernorm_bwd_drop", tag + " dres", dres, r["dres"], gt["dres"])
        ck.ok("sed_add_layernorm_bwd_drop", tag + " da", da, r["da"], gt["da"])
        ck.ok("sed_add_layernorm_bwd_drop", tag + " dgamma", Gn[norm + ".weight"], r["dgamma"], gt["dgamma"])
        ck.ok("sed_add_layernorm_bwd_drop", tag + " dbeta", Gn[norm + ".bias"], r["dbeta"], gt["dbeta"])
        st.only_changed(i, {"dres", "da"})
        return dres, da

    def residual(prod, i, name, dres):
        """the torch add behind launch i: what the next launch finds in `name` is the fp32 sum of the product and dres"""
        got = st.before(i + 1, name)
        assert np.array_equal(got.view(np.uint32), (prod + dres).view(np.uint32)), (name, "the residual add is not the fp32 sum")
        return got

    m = f32(g["m"])
    gcur = st.after(st.head_bwd, "dh")                        # the gradient of the last layer's output (sed_head_bwd: pinned elsewhere)
    for l in reversed(range(hd.layers)):
        an, nn_, fn, fnn = eng.sa_layer_names(l)
        cm, cn = eng.sa_conv_names(l)
        ly = lys[l]
        xin = m if l == 0 else lys[l - 1]["h2"]
        assert l == 0 or eng._sa_layer_out(g["layers"][l - 1]) is g["layers"][l - 1]["h2"]
        tag = f"l{l}"
        # ---- forward (the launches of a layer in any order: every buffer is the layer's own)
        hd.attention_forward(tag, l, ly, xin, an)
        hd.conv_forward(tag, l, ly, ly["h"])
        hd.ffn_forward(tag, fn, ly["hc"], ly["u"], ly["f"], 8 * l + DF.SITE_FFN_HIDDEN)
        # ---- backward: the FFN sub-layer, the module, the attention sub-layer
        i = st.take("sed_add_layernorm_bwd_drop")
        dres, da = layernorm(tag + " ffn_norm", ly["hc"], ly["f"], 8 * l + DF.SITE_FFN_OUT, fnn, gcur, ly["h2"], ly["stats2"], i)
        prod, i = hd.ffn_backward(tag, fn, ly["hc"], ly["u"], da, 8 * l + DF.SITE_FFN_HIDDEN, "dh1")
        gcur = residual(prod, i, "dh1", dres)
        i = st.take("sed_add_layernorm_bwd_drop")
        dres, da = layernorm(tag + " conv_norm", ly["h"], ly["co"], 8 * l + DF.SITE_CONV_OUT, cn, gcur, ly["hc"], ly["stats3"], i)
        prod, i = hd.conv_backward(tag, l, ly, ly["h"], da, "dhc")
        gcur = residual(prod, i, "dhc", dres)
        i = st.take("sed_add_layernorm_bwd_drop")
        dres, da = layernorm(tag + " attn_norm", xin, ly["a"], 8 * l + DF.SITE_ATTN_OUT, nn_, gcur, ly["h"], ly["stats"], i)
        prod, i = hd.attention_backward(tag, l, ly, an, xin, da, "dm")
        gcur = residual(prod, i, "dm", dres)
    assert st.take("sed_mel_mean_bwd") == len(st.launches) - 1
    assert np.array_equal(gcur, f32(g["dm"])), "dm changed after the head's backward"
    want = {"sed_gemm_nt", "sed_gemm_tn", "sed_gemm_tn colsum", "sed_add_layernorm_fwd_drop", "sed_add_layernorm_bwd_drop", "sed_mhsa_fwd_rel",
            "sed_mhsa_bwd_rel", "sed_relpos_expand", "sed_relpos_fold", "sed_ffn_fwd_drop", "sed_ffn_act_bwd_drop"} | set(AS.CONV_KINDS)
    assert hd.kinds() == want, hd.kinds() ^ want


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("conf", ["P", "M", "MD"])
def test_every_launch_of_the_pre_ln_chain_against_float64(sed, conf, precision):
    pre_ln_launches(sed, conf, precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_every_launch_of_the_composed_post_ln_head_against_float64(sed, precision):
    post_ln_launches(sed, "AR", precision)
