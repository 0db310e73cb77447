"""GPU: the attention pooling head (csrc/sed_attn.hip) through the C ABI -- sed_att_loss_fwd_bwd, sed_att_pool_fwd, sed_att_logits_fwd,
sed_att_bwd_pack / sed_head_bwd / sed_att_bwd_split -- and the layers on top of them (CnnEngine, FusedTrainer, the mean teacher,
label kinds, graph replay, infer_file).

Reference: tests/att_formula.py (float64; checked against torch autograd on the host in tests/test_att_host.py).  Every check is per
element.  Gates:
  loss, clip_prob, dpre, datt   |got - ref| <= 2^-23 |ref| + 2^-40 A + 2^-150, A the same expression over absolute values with p_i + P
                                in place of p_i - P (att_formula.gate: double arithmetic, one rounding to fp32; 2^-150 is half a step
                                of fp32's subnormal grid, which logits of +-104 reach: p q = e^-104 is below the normal range)
  att (linear layer)            (C + 2) 2^-24 (|m| |w| + |b|): the dot-product bound, valid for any summation order
  datt_w, datt_b                (rows + 2) 2^-24 sum |datt| |m|
  feature gradient              out_bound(dt, ref, (2K + 2) 2^-24 S), S the sum over absolute values: one rounding in fp32 and bf16
  event_fc gradients            the head test's own bound (tests/test_gpu_ops_exact_oracle.py): 4 (1 + rows per workgroup + 1) 2^-24 S
Cells that must be zero are compared with array_equal.  Every output lies in a sentinel-filled buffer between two canary regions;
every input must be unmodified afterwards."""
import importlib
import itertools
import json

import numpy as np
import pytest
import torch

from att_formula import att_loop, att_vectorised, feature_grad, gate, linear_bwd, linear_fwd
from test_gpu_weak import MANY_CLASSES, events_reach_the_last_slice_and_pass, label_slices
from weak_formula import frame_counts

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
GUARD = 1024
FILL = {torch.float32: (float("nan"), -1024.0), torch.float64: (float("nan"), -4096.0), torch.bfloat16: (float("nan"), -1024.0)}
# the last two: many classes, where att_label_slice (the maxima of a strong target, the twin of label_slice in csrc/sed_weak.hip) takes
# several passes of 256 classes, the slice count is capped at ATT_MAX_SLICES (the first) or clamped to the frames N (the second):
# the cuts of test_gpu_weak.test_shapes_reach_the_label_slice_branches, which the two files share constant for constant
SHAPES = [(1, 1, 1), (2, 5, 3), (3, 63, 1), (3, 64, 14), (2, 65, 17), (2, 257, 2), (1, 1025, 1), (2, 125, 527), (1, 3, 8200)]
W = 5.0                     # recall factor
U = 2.0 ** -24
F32, BF16 = 0, 1
DT = {F32: torch.float32, BF16: torch.bfloat16}


@pytest.fixture(scope="module")
def sed():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def L(sed):
    return sed._lib


class Guards:
    """output buffers: a sentinel inside, a canary region on both sides"""

    def __init__(self):
        self.bufs = []

    def new(self, dtype, *shape):
        n = int(np.prod(shape))
        inside, canary = FILL[dtype]
        buf = torch.full((n + 2 * GUARD,), canary, dtype=dtype, device="cuda")
        buf[GUARD:GUARD + n] = inside
        self.bufs.append((buf, n, canary))
        return buf[GUARD:GUARD + n].view(shape)

    def intact(self):
        torch.cuda.synchronize()
        for buf, n, canary in self.bufs:
            assert bool((buf[:GUARD] == canary).all()) and bool((buf[GUARD + n:] == canary).all()), "write outside an output buffer"


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.ndim else np.float32(a).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(np.asarray(a, dtype=np.float32)), bits(np.asarray(b, dtype=np.float32)))


def within(got, ref, A, tag):
    ok, worst = gate(got, ref, A)
    print(f"{tag}: worst error / bound {worst:.3f}")
    assert ok, (tag, worst)


def bound_check(got, ref, bound, tag):
    got, ref, bound = (np.asarray(v, dtype=np.float64) for v in (got, ref, bound))
    assert np.isfinite(got).all(), (tag, "an element is NaN/inf (not written, or overflowed)")
    err = np.abs(got - ref)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max()) if err.size else 0.0
    print(f"{tag}: worst error / bound {worst:.3f}")
    assert (err <= bound).all(), (tag, worst)


def bf16_half_ulp(x):
    """half a bf16 ulp of |x| (float64): bf16 has 8 significand bits, |x| = m * 2^e with m in [0.5, 1) -> ulp 2^(e-8)"""
    _, e = np.frexp(np.maximum(np.abs(x), 2.0 ** -126))
    return np.exp2(e.astype(np.float64) - 9.0)


def out_bound(dt, ref, bound):
    """the fp32-path bound, plus the storage rounding of a bf16 output (as in tests/test_gpu_ops_exact_oracle.py)"""
    return bound if dt == F32 else bound + bf16_half_ulp(np.abs(ref) + bound)


# ---- loss and pool through the C ABI ---------------------------------------------------------------------------------------------
def run_loss(L, pre, att, target, ratio, Tt, criterion="bce", sel=None, weight=1.0, grad_scale=1.0, with_clip=True, with_grad=True,
             into=None):
    """-> (clip_prob or None, loss, dpre or None, datt or None) as numpy.  into = (loss, dpre) numpy: accumulate = 1 on top of them"""
    B, t, K = pre.shape
    lib = L.lib()
    g = Guards()
    d_pre, d_att, d_tgt = dev(pre), dev(att), dev(target)
    d_sel = None if sel is None else dev(np.asarray(sel, dtype=np.uint8))
    clip = g.new(torch.float32, B, K) if with_clip else None
    loss = g.new(torch.float32, 1)
    dpre = g.new(torch.float32, B, t, K) if with_grad else None
    datt = g.new(torch.float32, B, t, K) if with_grad else None
    if into is not None:
        loss.copy_(dev(np.float32(into[0]).reshape(1)))
        dpre.copy_(dev(into[1]))
    nws = lib.sed_att_loss_ws_bytes(B, t, K)
    assert nws % 8 == 0 and nws >= 8
    ws = g.new(torch.float64, nws // 8)
    frames = target.shape[1] if target.ndim == 3 else 0
    assert frames in (0, Tt)
    L.check(lib.sed_att_loss_fwd_bwd(L.ptr(d_pre), L.ptr(d_att), L.ptr(d_tgt), frames, L.ptr(d_sel), {"bce": 0, "mse": 1}[criterion],
                                     L.ptr(clip), L.ptr(loss), L.ptr(dpre), L.ptr(datt), 0 if into is None else 1, B, t, K, ratio, Tt,
                                     W, weight, grad_scale, L.ptr(ws), stream()), "att_loss_fwd_bwd")
    g.intact()
    assert np.array_equal(d_pre.cpu().numpy(), pre) and np.array_equal(d_att.cpu().numpy(), att), "an input was modified"
    assert np.array_equal(d_tgt.cpu().numpy(), target) and (sel is None or np.array_equal(d_sel.cpu().numpy(), sel)), "an input was modified"
    out = tuple(None if a is None else a.cpu().numpy() for a in (clip, loss, dpre, datt))
    for a in out:
        assert a is None or not np.isnan(a).any(), "an output cell was not written"
    return out[0], out[1][0], out[2], out[3]


def run_pool(L, pre, att, ratio, Tt):
    B, t, K = pre.shape
    g = Guards()
    d_pre, d_att = dev(pre), dev(att)
    clip = g.new(torch.float32, B, K)
    L.check(L.lib().sed_att_pool_fwd(L.ptr(d_pre), L.ptr(d_att), L.ptr(clip), B, t, K, ratio, Tt, stream()), "att_pool_fwd")
    g.intact()
    assert np.array_equal(d_pre.cpu().numpy(), pre) and np.array_equal(d_att.cpu().numpy(), att), "an input was modified"
    return clip.cpu().numpy()


def check(got, ref, t, ratio, Tt, sel, tag):
    clip, loss, dpre, datt = got
    if clip is not None:
        within(clip, ref["P"], ref["A_P"], (tag, "clip_prob"))
    within(loss, ref["loss"], ref["A_loss"], (tag, "loss"))
    if dpre is None:
        return
    within(dpre, ref["dpre"], ref["A_dpre"], (tag, "dpre"))
    within(datt, ref["datt"], ref["A_datt"], (tag, "datt"))
    _, c = frame_counts(t, ratio, Tt)
    zero = np.zeros(dpre.shape, dtype=bool)
    zero[:, c == 0] = True
    if sel is not None:
        zero[np.asarray(sel) == 0] = True
        if not np.asarray(sel).any():
            zero[:] = True
            assert loss == 0.0
    for a in (dpre, datt):
        assert np.array_equal(a[zero], np.zeros(int(zero.sum()), dtype=np.float32)), (tag, "cells that must be exactly 0")


def targets(rng, B, K, Tt):
    clip = np.where(rng.random((B, K)) > 0.5, rng.uniform(0.3, 1.0, (B, K)), 0.0).astype(np.float32)
    clip[rng.random((B, K)) > 0.7] = 1.0
    strong = np.zeros((B, Tt, K), dtype=np.float32)
    for b in range(B):
        for k in range(K):
            if rng.random() > 0.4:
                a = int(rng.integers(0, Tt))
                strong[b, a:a + 1 + int(rng.integers(0, max(1, Tt // 3))), k] = 1.0 if rng.random() > 0.3 else 0.625
    return clip, strong


def frame_totals(t, ratio):
    """Tt = t*ratio, t*ratio - 3 (a partial last row) and a value that leaves whole rows with c_i = 0, where such a Tt exists"""
    return sorted({Tt for Tt in (t * ratio, t * ratio - 3, (t // 2) * ratio - 1 if t > 3 else ratio - 5) if Tt > 0})


def selections(B):
    """S = 0, 1 and B"""
    one = np.zeros(B, dtype=np.uint8)
    one[B // 2] = 1
    return [np.zeros(B, dtype=np.uint8), one, np.full(B, 3, dtype=np.uint8)]


def test_shapes_reach_the_label_slice_branches():
    """att_label_slice through test_att_loss_against_formula.  (2, 125, 527): three passes over the classes, the last with 15 live
    classes, in 4 to 63 slices; with ratio 8 and Tt around 1000 more than 64 slices are asked for and the count is capped.
    (1, 3, 8200): 33 passes, and more slices asked for than frames, so the count is clamped to N.  SHAPES before them: one pass."""
    B, t, K = MANY_CLASSES
    assert MANY_CLASSES in SHAPES and SHAPES[-1] == (1, 3, 8200) and K - 2 * 256 == 15
    assert [label_slices(min(t * r, Tt), K) for r in (1, 8) for Tt in frame_totals(t, r)] == \
        [(4, 4, 16, 3), (8, 8, 16, 3), (9, 9, 14, 3), (32, 31, 16, 3), (65, 63, 16, 3), (65, 63, 16, 3)]
    assert [label_slices(min(3 * r, Tt), 8200) for r in (1, 8) for Tt in frame_totals(3, r)] == \
        [(4, 3, 1, 33), (4, 3, 1, 33), (22, 21, 1, 33), (25, 24, 1, 33)]
    assert all(label_slices(min(s[1] * r, Tt), s[2])[3] == 1 for s in SHAPES[:-2] for r in (1, 8) for Tt in frame_totals(s[1], r))


@pytest.mark.parametrize("ratio", [1, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_att_loss_against_formula(L, shape, ratio):
    B, t, K = shape
    rng = np.random.default_rng(B * 100000 + t * 100 + K + ratio)
    pre = rng.normal(0.0, 3.0, shape).astype(np.float32)
    pre.reshape(-1)[rng.integers(0, pre.size, max(1, pre.size // 16))] = 104.0
    pre.reshape(-1)[rng.integers(0, pre.size, max(1, pre.size // 16))] = -104.0
    combos = itertools.cycle(itertools.product((0, 1), ("bce", "mse"), (None, 0, 1, 2), (False, True)))
    into_l, into_d = np.float32(0.375), rng.normal(0.0, 1e-3, shape).astype(np.float32)
    for Tt in frame_totals(t, ratio):
        _, c = frame_counts(t, ratio, Tt)
        for sigma in (1.0, 30.0):
            att = rng.normal(0.0, sigma, shape).astype(np.float32)
            tgts = targets(rng, B, K, Tt)
            if shape == MANY_CLASSES:
                events_reach_the_last_slice_and_pass(tgts[1], min(t * ratio, Tt))
            for _ in range(8):         # 8 of the 32 combinations per (Tt, sigma), the next 8 for the next pair
                form, crit, s, acc = next(combos)
                sel = None if s is None else selections(B)[s]
                tag = (shape, ratio, Tt, sigma, form, crit, None if sel is None else int((sel != 0).sum()), acc)
                ref = att_vectorised(pre, att, tgts[form], ratio, Tt, W, 0.75, 0.5, crit, sel)
                got = run_loss(L, pre, att, tgts[form], ratio, Tt, crit, sel, 0.75, 0.5)
                check(got, ref, t, ratio, Tt, sel, tag)
                if acc:
                    both = run_loss(L, pre, att, tgts[form], ratio, Tt, crit, sel, 0.75, 0.5, into=(into_l, into_d))
                    idle = np.zeros(shape, dtype=bool)
                    idle[:, c == 0] = True
                    if sel is not None:
                        idle[sel == 0] = True
                    want = np.where(idle, into_d, into_d + got[2])                  # ONE IEEE add per element; idle cells untouched
                    assert same_bits(both[2], want) and same_bits(both[1], np.float32(into_l + got[1])), tag
                    assert same_bits(both[3], got[3]) and same_bits(both[0], got[0]), (tag, "datt is overwritten, never accumulated")
            # the forward-only call gives the same clip probabilities, bit for bit; the optional outputs may be left out; two runs: equal bits
            assert same_bits(run_pool(L, pre, att, ratio, Tt), got[0]), (shape, ratio, Tt)
            bare = run_loss(L, pre, att, tgts[form], ratio, Tt, crit, sel, 0.75, 0.5, with_clip=False, with_grad=False)
            assert bare[0] is None and bare[2] is None and same_bits(bare[1], got[1])
            again = run_loss(L, pre, att, tgts[form], ratio, Tt, crit, sel, 0.75, 0.5)
            assert all(same_bits(a, b) for a, b in zip(got, again)), "two runs gave different bits"
    if B * t * K <= 64:                 # the loop form of the formula, where it is quick
        ref = att_loop(pre, att, tgts[form], ratio, Tt, W, 0.75, 0.5, crit, sel)
        check(got, ref, t, ratio, Tt, sel, (shape, ratio, "loop"))


@pytest.mark.parametrize("ratio", [1, 8])
def test_attention_spread_above_800_underflows_to_exact_zero_weights(L, ratio):
    rng = np.random.default_rng(2)
    B, t, K = 2, 70, 3
    pre = rng.normal(0.0, 3.0, (B, t, K)).astype(np.float32)
    att = rng.normal(-850.0, 5.0, (B, t, K)).astype(np.float32)
    top = rng.integers(0, t - 1, (B, K))
    for b in range(B):
        for k in range(K):
            att[b, top[b, k], k] = 20.0             # the only row whose weight survives: the others are exp(< -800) = 0 in double
    att[:, t - 1] = 4000.0                          # takes no part below (c = 0): must not enter the maximum
    Tt = (t - 1) * ratio
    clip_t, strong_t = targets(rng, B, K, Tt)
    for target, crit in ((clip_t, "bce"), (strong_t, "mse")):
        ref = att_vectorised(pre, att, target, ratio, Tt, W, 1.0, 1.0, crit)
        got = run_loss(L, pre, att, target, ratio, Tt, crit)
        assert all(np.isfinite(a).all() for a in got)
        check(got, ref, t, ratio, Tt, None, ("spread", ratio, crit))
        assert int((got[2] != 0).sum()) <= B * K          # one row per (b, k) carries dpre
        p = 1.0 / (1.0 + np.exp(-np.take_along_axis(pre.astype(np.float64), top[:, None, :], axis=1)[:, 0]))
        within(got[0], p, p, ("spread", ratio, "P is that row's probability"))


# ---- the linear layer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 63, 64, 65, 257])
@pytest.mark.parametrize("geom", [(128, 128, 1), (128, 100, 2), (512, 512, 17), (96, 80, 33), (32, 1, 1), (128, 128, 527),
                                  (516, 513, 30), (2048, 2048, 7), (1028, 1025, 3)], ids=lambda g: "x".join(map(str, g)))
def test_att_logits_against_formula(L, geom, rows):
    """the last four geoms: more classes than one LDS weight chunk holds, kch = ATT_LDS_FLOATS / (64 NV) = 12288 / (64 NV), so the
    weights are restaged per chunk between two barriers and the last chunk is partial -- (128, 128, 527): NV = 2, kch = 96, 6
    chunks, the last of 47 classes; (516, 513, 30): NV = 16, kch = 12, 3 chunks, the last of 6; (2048, 2048, 7): NV = 32, kch = 6,
    2 chunks, the last of 1 -- and the NV = 16 and NV = 32 instantiations (C > 512, one row per group of 16 lanes), of which
    (1028, 1025, 3) is the single-chunk case"""
    Cp, C, K = geom
    rng = np.random.default_rng(Cp + 3 * C + 5 * K + rows)
    m = rng.normal(0.0, 1.0, (rows, Cp)).astype(np.float32)
    m[:, C:] = np.nan                                # the padding holds garbage: it must not be read
    w, b = rng.normal(0.0, 0.2, (K, C)).astype(np.float32), rng.normal(0.0, 1.0, K).astype(np.float32)
    g = Guards()
    d_m, d_w, d_b = dev(m), dev(w), dev(b)
    att = g.new(torch.float32, rows, K)
    L.check(L.lib().sed_att_logits_fwd(L.ptr(d_m), L.ptr(d_w), L.ptr(d_b), L.ptr(att), rows, C, Cp, K, stream()), "att_logits_fwd")
    g.intact()
    for d, h in ((d_m, m), (d_w, w), (d_b, b)):
        assert np.array_equal(d.cpu().numpy(), h, equal_nan=True), "an input was modified"
    ref, scale = linear_fwd(np.nan_to_num(m), w, b)
    got = att.cpu().numpy()
    bound_check(got, ref, (C + 2) * U * scale, ("att_logits", geom, rows))
    again = g.new(torch.float32, rows, K)
    L.check(L.lib().sed_att_logits_fwd(L.ptr(d_m), L.ptr(d_w), L.ptr(d_b), L.ptr(again), rows, C, Cp, K, stream()), "att_logits_fwd")
    assert same_bits(again.cpu().numpy(), got)


@pytest.mark.parametrize("case", [(32, 32, 32, 3), (32, 128, 128, 100), (16, 516, 513, 13)], ids=lambda c: "x".join(map(str, c)))
def test_att_logits_more_rows_than_one_grid_pass(L, case):
    """att_logits_kernel's loop over `it`: rows = 768 * per_wg + 5, so iters = 2 and the second pass holds 5 rows, in workgroup 0.
    (32, 32, 32, 3): one chunk -- the weights staged at it == 0 serve it == 1 (the branch `nch > 1 || it == 0` not taken).
    (32, 128, 128, 100): kch = 96, two chunks per iteration, restaged in both.  (16, 516, 513, 13): NV = 16, one row per group, kch
    = 12, two chunks."""
    per_wg, Cp, C, K = case
    GRID_CAP = 768                      # launch_att_logits in csrc/sed_attn.hip: `if (grid > 768) grid = 768`
    ROWS_PER_WG = {2: 32, 1: 16}        # 4 waves * ATT_GPW (4 groups of 16 lanes) * RG rows; RG = 2 for C <= 512 (NV <= 8), else 1
    assert per_wg == ROWS_PER_WG[2 if C <= 512 else 1]
    edge = GRID_CAP * per_wg            # the first row of the second iteration
    rows = edge + 5
    rng = np.random.default_rng(Cp + 3 * C + 5 * K + rows)
    m = rng.normal(0.0, 1.0, (rows, Cp)).astype(np.float32)
    m[:, C:] = np.nan                                # the padding holds garbage: it must not be read
    w, b = rng.normal(0.0, 0.2, (K, C)).astype(np.float32), rng.normal(0.0, 1.0, K).astype(np.float32)
    g = Guards()
    d_m, d_w, d_b = dev(m), dev(w), dev(b)
    att = g.new(torch.float32, rows, K)
    L.check(L.lib().sed_att_logits_fwd(L.ptr(d_m), L.ptr(d_w), L.ptr(d_b), L.ptr(att), rows, C, Cp, K, stream()), "att_logits_fwd")
    g.intact()
    for d, h in ((d_m, m), (d_w, w), (d_b, b)):
        assert np.array_equal(d.cpu().numpy(), h, equal_nan=True), "an input was modified"
    ref, scale = linear_fwd(np.nan_to_num(m), w, b)
    got = att.cpu().numpy()
    bound = (C + 2) * U * scale
    for name, sl in (("the last row of the first iteration", slice(edge - 1, edge)), ("the first row of the second", slice(edge, edge + 1)),
                     ("the last 5 rows", slice(rows - 5, rows))):
        bound_check(got[sl], ref[sl], bound[sl], ("att_logits", case, name))
    bound_check(got, ref, bound, ("att_logits", case, rows))
    again = g.new(torch.float32, rows, K)
    L.check(L.lib().sed_att_logits_fwd(L.ptr(d_m), L.ptr(d_w), L.ptr(d_b), L.ptr(again), rows, C, Cp, K, stream()), "att_logits_fwd")
    g.intact()
    assert same_bits(again.cpu().numpy(), got)


def test_att_logits_unaligned_rows_take_the_scalar_loads(L):
    """a channel pitch that is no multiple of 4: rows do not start on 16 bytes"""
    rng = np.random.default_rng(9)
    rows, Cp, C, K = 37, 99, 97, 5
    m = rng.normal(0.0, 1.0, (rows, Cp)).astype(np.float32)
    m[:, C:] = np.nan
    w, b = rng.normal(0.0, 0.2, (K, C)).astype(np.float32), rng.normal(0.0, 1.0, K).astype(np.float32)
    g = Guards()
    att = g.new(torch.float32, rows, K)
    d_m, d_w, d_b = dev(m), dev(w), dev(b)
    L.check(L.lib().sed_att_logits_fwd(L.ptr(d_m), L.ptr(d_w), L.ptr(d_b), L.ptr(att), rows, C, Cp, K, stream()), "att_logits_fwd")
    g.intact()
    assert np.array_equal(d_m.cpu().numpy(), m, equal_nan=True), "the input was modified"
    ref, scale = linear_fwd(np.nan_to_num(m), w, b)
    bound_check(att.cpu().numpy(), ref, (C + 2) * U * scale, "att_logits, pitch 99")


# ---- the backward of both linear layers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("bt", [(1, 1), (3, 21), (5, 13), (1, 257)], ids=lambda v: f"rows{v[0] * v[1]}")
@pytest.mark.parametrize("geom", [(128, 128, 1, 4), (128, 100, 2, 2), (512, 512, 17, 1), (96, 80, 33, 1), (32, 1, 1, 1)],
                         ids=lambda g: "x".join(map(str, g)))
def test_backward_branch(L, geom, bt, dt):
    (Cp, C, K, Wf), (B, t) = geom, bt
    rows = B * t
    lib, P, st = L.lib(), L.ptr, stream()
    gen = torch.Generator(device="cuda").manual_seed(Cp + 3 * C + 5 * K + rows)
    feat = torch.randn(B, t, Wf, Cp, device="cuda", generator=gen).abs_()
    feat = (feat * (torch.rand(B, t, Wf, Cp, device="cuda", generator=gen) < 0.6)).to(DT[dt])
    feat[..., C:] = 0
    fc_w = torch.randn(K, C, device="cuda", generator=gen) * 0.2
    fc_b = torch.randn(K, device="cuda", generator=gen)
    att_w = torch.randn(K, C, device="cuda", generator=gen) * 0.2
    dpre = torch.randn(rows, K, device="cuda", generator=gen) * 1e-2
    datt = torch.randn(rows, K, device="cuda", generator=gen) * 1e-2
    g = Guards()
    m, pre = g.new(torch.float32, B, t, Cp), g.new(torch.float32, B, t, K)
    L.check(lib.sed_head_fwd(dt, P(feat), P(fc_w), P(fc_b), P(m), P(pre), B, t, Wf, C, Cp, K, st), "head_fwd")
    dcat, wcat = g.new(torch.float32, rows, 2 * K), g.new(torch.float32, 2 * K, C)
    dwcat, dbcat = g.new(torch.float32, 2 * K, C), g.new(torch.float32, 2 * K)
    ws = g.new(torch.float32, lib.sed_head_bwd_ws_floats(B, t, C, 2 * K))
    dfeat = g.new(DT[dt], B, t, Wf, Cp)
    grads = [g.new(torch.float32, K, C), g.new(torch.float32, K), g.new(torch.float32, K, C), g.new(torch.float32, K)]
    keep = [v.clone() for v in (dpre, datt, fc_w, att_w)]
    L.check(lib.sed_att_bwd_pack(P(dpre), P(datt), P(fc_w), P(att_w), P(dcat), P(wcat), rows, C, K, st), "att_bwd_pack")
    L.check(lib.sed_head_bwd(dt, P(dcat), P(m), P(wcat), P(dwcat), P(dbcat), P(dfeat), P(ws), B, t, Wf, C, Cp, 2 * K, 1, st), "head_bwd")
    L.check(lib.sed_att_bwd_split(P(dwcat), P(dbcat), *(P(v) for v in grads), C, K, st), "att_bwd_split")
    g.intact()
    assert all(torch.equal(a, b) for a, b in zip(keep, (dpre, datt, fc_w, att_w))), "an input was modified"
    assert torch.equal(dcat, torch.cat([dpre, datt], dim=1)) and torch.equal(wcat, torch.cat([fc_w, att_w], dim=0))
    mh = m.cpu().numpy().reshape(rows, Cp)
    dp, da, fw, aw = (v.cpu().numpy() for v in (dpre, datt, fc_w, att_w))
    tag = (geom, bt, dt)
    dw, db, sw, sb = linear_bwd(da, mh, C)
    bound_check(grads[2].cpu().numpy(), dw, (rows + 2) * U * sw, (tag, "datt_w"))
    bound_check(grads[3].cpu().numpy(), db, (rows + 2) * U * sb, (tag, "datt_b"))
    big = 2 * K <= 32 and 2 * K * C <= 8192 and 256 % (Cp // 8) == 0      # sed_head_bwd's 64-row form (test_gpu_ops_exact_oracle.py)
    cw = 4.0 * (1 + (64 if big else 8) + 1) * U
    dw, db, sw, sb = linear_bwd(dp, mh, C)
    bound_check(grads[0].cpu().numpy(), dw, cw * sw, (tag, "dfc_w"))
    bound_check(grads[1].cpu().numpy(), db, cw * sb, (tag, "dfc_b"))
    ref, S = feature_grad(dp, da, fw, aw, Wf)
    got = dfeat.float().cpu().numpy().reshape(rows, Wf, Cp)
    for wi in range(Wf):
        bound_check(got[:, wi, :C], ref, out_bound(dt, ref, (2 * K + 2) * U * S), (tag, "feature gradient", wi))
    assert np.array_equal(got[:, :, C:], np.zeros((rows, Wf, Cp - C), dtype=np.float32)), "padded channels must be exactly 0"


# ---- through the model and the trainer -------------------------------------------------------------------------------------------
CFG = [(32, 2), (32, 2)]
K_CLASSES = 3


def make_model(sed, kind, precision, attention=True, seed=0):
    torch.manual_seed(seed)
    if kind == "cnn":
        return sed.Cnn_AvgPooling(K_CLASSES, CFG, precision=precision, attention=attention).cuda()
    return sed.Crnn_AvgPooling(K_CLASSES, CFG, precision=precision, gru_hidden=32, attention=attention).cuda()


def batch():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 1, 32, 64, generator=g)
    y = torch.zeros(2, 32, K_CLASSES)
    y[0, 4:13, 0] = 1.0
    y[1, 20:30, 1] = 1.0
    y[1, 2:6, 0] = 0.5
    return x.cuda(), y.cuda()


def the_plan(model):
    plans = list(model.engine._plans.values())
    assert len(plans) == 1
    return plans[0]


def head_m(model, plan):
    """(m (rows, Cp) float64, C): what both linear layers read"""
    if plan.gru is not None:
        return plan.gru["fc_m"].double().cpu().numpy(), 64
    return plan.m.double().cpu().numpy().reshape(-1, plan.m.shape[-1]), CFG[-1][0]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["cnn", "crnn"])
def test_engine_chain_against_float64(sed, L, monkeypatch, kind, precision):
    monkeypatch.setenv("SED_C1_MODE", "0")          # stage snapshots (debug) need conv1's output in memory
    x, y = batch()
    model = make_model(sed, kind, precision).train()
    eng = model.engine
    P = model._tensor_dict()
    G = {n: torch.full_like(p, float("nan")) for n, p in model.named_parameters()}
    plan = eng.forward(x, P, training=True)
    assert eng.ratio == 4 and plan.pre.shape == (2, 8, K_CLASSES) and plan.att.shape == plan.pre.shape
    m, C = head_m(model, plan)
    rows = m.shape[0]
    pre, att = plan.pre.cpu().numpy(), plan.att.cpu().numpy()
    aw, ab = model.att_fc.weight.detach().cpu().numpy(), model.att_fc.bias.detach().cpu().numpy()
    fw = model.event_fc.weight.detach().cpu().numpy()
    ref, scale = linear_fwd(m, aw, ab)
    bound_check(att.reshape(rows, -1), ref, (C + 2) * U * scale, (kind, precision, "plan.att"))
    loss = eng.loss_and_grad(plan, y, W, weak=("att", 0.5, True)).clone()
    assert plan.att_pending
    r = att_vectorised(pre, att, y.cpu().numpy(), 4, 32, W, 0.5)
    dpre, datt = plan.dpre.cpu().numpy(), plan.datt.cpu().numpy()
    check((plan.clip_prob.cpu().numpy(), loss.cpu().numpy()[0], dpre, datt), r, 8, 4, 32, None, (kind, precision, "loss"))
    clip = plan.clip_prob.cpu().numpy().copy()
    assert same_bits(eng.clip_probs(plan, "att").cpu().numpy(), clip)       # the pooling alone: the same bits
    with pytest.raises(RuntimeError, match="pending"):
        eng.backward(plan, P, G, dlogits=torch.zeros(2, 32, K_CLASSES, device="cuda"))
    debug = {}
    done = []
    eng.backward(plan, P, G, debug=debug, on_group_done=done.append)
    assert done[:2] == ["att_fc", "event_fc"] and done.count("att_fc") == 1
    dp, da = dpre.reshape(rows, -1), datt.reshape(rows, -1)
    dw, db, sw, sb = linear_bwd(da, m, C)
    bound_check(G["att_fc.weight"].cpu().numpy(), dw, (rows + 2) * U * sw, (kind, precision, "datt_w"))
    bound_check(G["att_fc.bias"].cpu().numpy(), db, (rows + 2) * U * sb, (kind, precision, "datt_b"))
    dw, db, sw, sb = linear_bwd(dp, m, C)
    cw = 4.0 * (1 + 64 + 1) * U
    bound_check(G["event_fc.weight"].cpu().numpy(), dw, cw * sw, (kind, precision, "dfc_w"))
    bound_check(G["event_fc.bias"].cpu().numpy(), db, cw * sb, (kind, precision, "dfc_b"))
    if kind == "cnn":
        Wf = plan.w_out
        fref, S = feature_grad(dp, da, fw, aw, Wf)
        dy = debug["dy1"].cpu().numpy().reshape(rows, Wf, -1)
        dt = BF16 if precision == "bf16" else F32
        for wi in range(Wf):
            bound_check(dy[:, wi, :C], fref, out_bound(dt, fref, (2 * K_CLASSES + 2) * U * S), (kind, precision, "dy1", wi))
    else:
        fref, S = feature_grad(dp, da, fw, aw, 1)
        bound_check(plan.gru["dhseq"].cpu().numpy(), fref, (2 * K_CLASSES + 2) * U * S, (kind, precision, "dhseq"))
        assert bool(torch.isfinite(debug["dy1"]).all()) and float(debug["dy1"].abs().max()) > 0
    assert all(bool(torch.isfinite(v).all()) for v in G.values())
    # a new forward clears the pending flag: the model's own autograd backward covers the frame logits only
    out = model(x)
    assert not the_plan(model).att_pending
    out.sum().backward()
    assert not model.att_fc.weight.grad.any() and not model.att_fc.bias.grad.any() and bool(model.event_fc.weight.grad.any())


@pytest.mark.parametrize("kind", ["cnn", "crnn"])
def test_trainer_teacher_kinds_and_other_poolings(sed, L, kind):
    x, y = batch()
    yn = y.cpu().numpy()
    # label kinds: clip 0 weak, clip 1 unlabelled -> the attention loss over clip 0 alone
    model = make_model(sed, kind, "fp32")
    tr = sed.FusedTrainer(model, lr=1e-3, recall_factor=W, weak_pooling="att", weak_weight=0.5, weak_only=True)
    loss = tr.forward_backward(x, y, torch.tensor([1, 2], device="cuda")).clone()
    plan = the_plan(model)
    pre, att = plan.pre.cpu().numpy(), plan.att.cpu().numpy()
    r = att_vectorised(pre, att, yn, 4, 32, W, 0.5, sel=[1, 0])
    check((plan.clip_prob.cpu().numpy(), loss.cpu().numpy()[0], plan.dpre.cpu().numpy(), plan.datt.cpu().numpy()), r, 8, 4, 32,
          np.array([1, 0]), (kind, "kind"))
    assert float(tr.flat.G["att_fc.weight"].abs().max()) > 0
    # a weak-linear step on the attention model: att_fc's gradient is exactly 0, whatever the buffer held
    lin = sed.FusedTrainer(make_model(sed, kind, "fp32"), lr=1e-3, recall_factor=W, weak_pooling="linear", weak_only=True)
    for v in lin.flat.G.values():
        v.fill_(float("nan"))
    lin.forward_backward(x, y)
    assert not lin.flat.G["att_fc.weight"].any() and not lin.flat.G["att_fc.bias"].any()
    assert all(bool(torch.isfinite(v).all()) for v in lin.flat.G.values()) and float(lin.flat.G["event_fc.weight"].abs().max()) > 0
    # the mean teacher: the frame term as always, the clip term with both models pooled by their own attention
    model = make_model(sed, kind, "fp32")
    mt = sed.FusedTrainer(model, lr=1e-3, recall_factor=W, weak_pooling="att", weak_weight=0.5, mean_teacher=True,
                          consistency_weight=2.0)
    with torch.no_grad():                            # a teacher that differs from the student
        for p in mt.teacher.parameters():
            p.mul_(0.9)
    mt.forward_backward(x, y)
    plan, tplan = the_plan(model), the_plan(mt.teacher)
    pre, att = plan.pre.cpu().numpy(), plan.att.cpu().numpy()
    tP = att_vectorised(tplan.pre.cpu().numpy(), tplan.att.cpu().numpy(), np.zeros((2, K_CLASSES)), 4, 32, W)
    within(plan.teacher_clip.cpu().numpy(), tP["P"], tP["A_P"], (kind, "the teacher's clip probabilities"))
    r = att_vectorised(pre, att, plan.teacher_clip.cpu().numpy(), 4, 32, W, 2.0, criterion="mse")
    within(mt.last_consistency.cpu().numpy()[1], r["loss"], r["A_loss"], (kind, "clip consistency term"))
    within(plan.clip_prob.cpu().numpy(), r["P"], r["A_P"], (kind, "the student's clip probabilities"))
    within(plan.datt_clip.cpu().numpy(), r["datt"], r["A_datt"], (kind, "the clip term's datt"))
    s = att_vectorised(pre, att, yn, 4, 32, W, 0.5)
    # each term rounded once (2^-23 |term| + 2^-40 A + 2^-150 as above), then one fp32 add (2^-24 of the sum; exact among subnormals)
    bound_check(plan.datt.cpu().numpy(), s["datt"] + r["datt"],
                2.0 ** -23 * (np.abs(s["datt"]) + np.abs(r["datt"])) + 2.0 ** -24 * np.abs(s["datt"] + r["datt"])
                + 2.0 ** -40 * (s["A_datt"] + r["A_datt"]) + 2.0 ** -149, (kind, "datt of both clip terms: two roundings and one add"))
    assert float(mt.flat.G["att_fc.weight"].abs().max()) > 0 and all(bool(torch.isfinite(v).all()) for v in mt.flat.G.values())


@pytest.mark.parametrize("kind", ["cnn", "crnn"])
def test_a_later_loss_replaces_the_pending_attention_gradient(sed, kind):
    """backward() follows the LAST loss_and_grad on the plan: the attention loss, then the strong loss, is a strong-only step"""
    x, y = batch()
    model = make_model(sed, kind, "fp32").train()
    eng, P = model.engine, model._tensor_dict()

    def grads():
        return {n: torch.full_like(p, float("nan")) for n, p in model.named_parameters()}

    strong, mixed, lin = grads(), grads(), grads()
    plan = eng.forward(x, P, training=True)
    eng.loss_and_grad(plan, y, W)
    assert not plan.att_pending
    eng.backward(plan, P, strong)
    plan = eng.forward(x, P, training=True)             # (batch statistics: the same activations)
    eng.loss_and_grad(plan, y, W, weak=("att", 0.5, True))
    assert plan.att_pending and float(plan.datt.abs().max()) > 0
    eng.loss_and_grad(plan, y, W)
    assert not plan.att_pending
    eng.backward(plan, P, mixed)
    assert not mixed["att_fc.weight"].any() and not mixed["att_fc.bias"].any()
    for n in strong:
        assert torch.equal(strong[n], mixed[n]), n
    assert float(strong["event_fc.weight"].abs().max()) > 0 and float(strong["conv_blocks.0.conv1.weight"].abs().max()) > 0
    # the same after a parameter-free weak loss, after a loss without a gradient, and a backward from dlogits is taken again
    eng.loss_and_grad(plan, y, W, weak=("att", 0.5, True))
    eng.loss_and_grad(plan, y, W, weak=("linear", 0.5, True))
    assert not plan.att_pending
    eng.backward(plan, P, lin)
    assert not lin["att_fc.weight"].any() and not lin["att_fc.bias"].any() and bool(lin["event_fc.weight"].any())
    eng.loss_and_grad(plan, y, W, weak=("att", 0.5, True))
    eng.loss_and_grad(plan, y, W, weak=("att", 0.5, True), need_grad=False)
    assert not plan.att_pending
    eng.backward(plan, P, lin, dlogits=torch.zeros(2, 32, K_CLASSES, device="cuda"))
    assert not lin["att_fc.weight"].any() and not lin["event_fc.weight"].any()


@pytest.mark.parametrize("kind", ["cnn", "crnn"])
def test_graph_steps_give_the_eager_parameter_bits(sed, kind):
    x, y = batch()
    yc = y.max(dim=1).values.contiguous()

    def fresh():
        return sed.FusedTrainer(make_model(sed, kind, "bf16"), lr=1e-3, recall_factor=W, graph=True, weak_pooling="att", weak_only=True)

    eager, graph = fresh(), fresh()
    start = eager.flat.P["att_fc.weight"].clone()
    for i in range(5):                  # the same device-scalar step: launch by launch / two eager steps, the capture, three replays
        eager._step_dev(x, yc)
        eager._host_mirror()
        graph.train_step(x, yc)
        assert torch.equal(eager.flat.p, graph.flat.p), (i, "the graph step differs from the eager step")
    assert len(graph._graphs) == 1 and len(eager._graphs) == 0
    assert not torch.equal(eager.flat.P["att_fc.weight"], start), "att_fc was not trained"


def test_infer_file_att_clip_probs(sed, tmp_path):
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
    model = sed.Cnn_AvgPooling(sc.BENCH.classes_num, cfg, precision="fp32", mel_bins=sc.BENCH.mel_bins, attention=True)
    ck = str(tmp_path / "m.pth")
    torch.save({"iterations": 0, "model": model.state_dict()}, ck)
    plain = infer.infer_file(p, ck, precision="fp32", cfg=sc.BENCH)
    res = infer.infer_file(p, ck, precision="fp32", cfg=sc.BENCH, clip_pooling="att")
    assert "clip_probs" not in plain and np.array_equal(res["probabilities"], plain["probabilities"])
    model = model.cuda().eval()
    with torch.no_grad():
        model(torch.from_numpy(plain["log_mel"]).cuda()[None, None])
    plan = the_plan(model)
    assert np.array_equal(res["clip_probs"], model.engine.clip_probs(plan, "att").cpu().numpy())
    pre, att = plan.pre.cpu().numpy(), plan.att.cpu().numpy()
    r = att_vectorised(pre, att, np.zeros((1, sc.BENCH.classes_num)), model.engine.ratio, pre.shape[1] * model.engine.ratio, W)
    within(res["clip_probs"], r["P"], r["A_P"], "infer_file clip_probs")
    assert np.array_equal(infer.infer_file(p, ck, precision="fp32", cfg=sc.BENCH, clip_pooling="linear")["probabilities"], plain["probabilities"])
    # a checkpoint without the head: refused
    torch.manual_seed(0)
    bare = sed.Cnn_AvgPooling(sc.BENCH.classes_num, cfg, precision="fp32", mel_bins=sc.BENCH.mel_bins)
    ck2 = str(tmp_path / "bare.pth")
    torch.save({"iterations": 0, "model": bare.state_dict()}, ck2)
    with pytest.raises(ValueError, match="att_fc.weight"):
        infer.infer_file(p, ck2, precision="fp32", cfg=sc.BENCH, clip_pooling="att")


def test_eval_ranking_with_attention_pooled_clips(sed):
    syn = importlib.import_module(PKG + ".dataset.synthetic")
    from torch.utils.data import DataLoader
    loader = DataLoader(syn.SyntheticSedDataset(n_train_crops=8, crop=32, n_val=3, val_frames=200, classes=3, seed=5), batch_size=4)
    model = make_model(sed, "cnn", "fp32", seed=5).eval()
    dev_ = torch.device("cuda:0")
    plain = sed.train.eval_ranking(model, loader, dev_)
    got = sed.train.eval_ranking(model, loader, dev_, clip_pooling="att")
    assert got["clip"]["pooling"] == "att" and got["n_recordings"] == 3 and json.dumps(got["per_class"]) == json.dumps(plain["per_class"])
    lin = sed.train.eval_ranking(model, loader, dev_, clip_pooling="linear")
    assert lin["clip"]["pooling"] == "linear" and len(got["clip"]["per_class"]) == 3
    with pytest.raises(ValueError, match="attention head"):
        sed.train.eval_ranking(make_model(sed, "cnn", "fp32", attention=False), loader, dev_, clip_pooling="att")


# the launch labels of one eager bf16 train step of Cnn_AvgPooling(3, CFG) without the head, as the commit before the head recorded them
PLAIN_STEP = ["sed_pack_conv_weights_batch", "sed_conv3x3_c1_gram", "sed_bn_train_finalize_c1", "sed_conv3x3_fwd_c1",
              "sed_bn_train_finalize", "sed_bn_relu_pool_cnt_fwd", "sed_conv3x3_fwd", "sed_bn_train_finalize", "sed_conv3x3_fwd",
              "sed_bn_train_finalize", "sed_bn_relu_pool_fwd", "sed_head_fwd", "sed_bce_fwd_bwd", "sed_head_bwd",
              "sed_pool_relu_bwd_stats", "sed_bn_bwd_finalize", "sed_conv3x3_wgrad_fused", "sed_conv3x3_fwd", "sed_bn_bwd_finalize",
              "sed_conv3x3_wgrad_fused", "sed_conv3x3_dgrad_poolstats", "sed_pool_relu_bwd_stats_if", "sed_bn_bwd_finalize",
              "sed_conv3x3_bwd_fused_c1", "sed_c1_bwd_tail", "sed_adam_amsgrad_step"]


def step_labels(sed, attention, **kw):
    x, y = batch()
    mdl = make_model(sed, "cnn", "bf16", attention=attention)
    tr = sed.FusedTrainer(mdl, lr=1e-3, recall_factor=W, **kw)
    tr.train_step(x, y)             # (first step: allocations)
    mdl.engine.timer = sed.engine.KernelTimer()
    tr.train_step(x, y)
    torch.cuda.synchronize()
    return [lbl.split(":")[0] for lbl, _, _ in mdl.engine.timer.records]


def test_launch_lists(sed):
    plain = step_labels(sed, False)
    print("plain step:", plain)
    assert plain == PLAIN_STEP
    weak = step_labels(sed, False, weak_pooling="linear", weak_only=True)
    i = plain.index("sed_bce_fwd_bwd")
    assert weak == plain[:i] + ["sed_weak_bce_fwd_bwd"] + plain[i + 1:]
    # the head: one launch after the head forward; the strong step's backward gains nothing but att_fc's zero fill (a torch fill)
    h = plain.index("sed_head_fwd")
    assert step_labels(sed, True) == plain[:h + 1] + ["sed_att_logits_fwd"] + plain[h + 1:]
    att = step_labels(sed, True, weak_pooling="att", weak_only=True)
    b = plain.index("sed_head_bwd")
    assert att == plain[:h + 1] + ["sed_att_logits_fwd"] + plain[h + 1:i] + ["sed_att_loss_fwd_bwd"] + plain[i + 1:b] + \
        ["sed_att_bwd_pack", "sed_head_bwd", "sed_att_bwd_split"] + plain[b + 1:]
