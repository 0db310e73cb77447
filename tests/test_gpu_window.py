"""GPU: the local attention window through the C ABI (sed_mhsa_fwd_win / sed_mhsa_bwd_win / sed_mhsa_win_tiles, the WIN instantiations
of csrc/sed_mhsa.hip), per element against the float64 definition of tests/window_formula.py within the gates derived in that file's
docstring, SED_F32 and SED_BF16, B = 2, without dropout and at p in {0.1, 0.5}.

  cases      a chosen list over t in {1, 5, 33, 64, 65, 130, 257}, (H, dh) in {(1, 32), (4, 32), (2, 64)} and the windows (0, 0), (3, 0),
             (0, 3), (1, 1), (31, 0), (32, 32), (33, 31), (40, 7), (unbounded, 0), (0, unbounded), (t - 2, t - 2): the fully-masked first
             tile (left = 3 from t = 64 on), windows narrower and wider than a tile, edges on and next to tile (32) and workgroup (128)
             boundaries, windows wider than the clip; every case also checks sed_mhsa_win_tiles against the brute-force count
  loud key   one key per clip scores 120 against every query: queries with it in the window are near-one-hot, the others show no trace
             of it, forward and backward, and nothing is NaN or inf
  probe      q = k = 0 and V = rows of the identity read the window (and with p > 0 the mask) out of the fused forward
  bits       both sides >= t - 1 give sed_mhsa_fwd / _bwd bits (p = 0) and the _drop twins' (p > 0); repeats give the same bits;
             lse = NULL gives the same ctx bits
  memory     inputs between NaN regions, outputs between canaries; refusals leave the outputs untouched
Run with -s for the worst error / gate of every check.  Measured on the MI355X (worst over the cases): 0.97 in bf16 (dv, t = 257, window
(1, 1), p = 0.5: a sum of two or three terms nearly attains the 2^-8 operand bound, bf16's unit roundoff) and 0.07 in fp32 (dv, t = 257,
window (3, 0))."""
import importlib

import numpy as np
import pytest
import torch

import dropout_formula as DF
import mhsa_formula as MF
import window_formula as WF

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
GUARD = 1024
CANARY = -1024.0
F32, BF16 = 0, 1
SEED = (0x5EDD0001, 0x00C0FFEE)
UNB = 0x7FFFFFFF
T2 = "t-2"
# (t, (H, dh), (left, right), p of the dropped run)
CASES = [
    (1, (1, 32), (0, 0), 0.1), (5, (4, 32), (3, 0), 0.5), (5, (2, 64), (0, 3), 0.1), (5, (1, 32), (40, 7), 0.5),
    (33, (1, 32), (1, 1), 0.1), (33, (2, 64), (31, 0), 0.5), (33, (4, 32), (T2, T2), 0.1),
    (64, (4, 32), (32, 32), 0.5), (64, (2, 64), (3, 0), 0.1), (64, (1, 32), (0, UNB), 0.5),
    (65, (1, 32), (33, 31), 0.1), (65, (4, 32), (UNB, 0), 0.5), (65, (2, 64), (0, 0), 0.1),
    (130, (2, 64), (40, 7), 0.5), (130, (4, 32), (0, UNB), 0.1), (130, (1, 32), (T2, T2), 0.5), (130, (4, 32), (31, 0), 0.1),
    (130, (1, 32), (0, 3), 0.5),
    (257, (4, 32), (3, 0), 0.1), (257, (2, 64), (32, 32), 0.5), (257, (1, 32), (33, 31), 0.1), (257, (1, 32), (T2, T2), 0.5),
    (257, (4, 32), (UNB, 0), 0.1), (257, (2, 64), (1, 1), 0.5),
]


def case_id(c):
    t, (H, dh), (l, r), p = c
    f = lambda v: "inf" if v == UNB else str(v)
    return f"t{t}-H{H}dh{dh}-w{f(l)}_{f(r)}-p{p}"


def window_of(c):
    t, _, (l, r), _ = c
    return tuple(max(t - 2, 0) if v == T2 else v for v in (l, r))


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def state(step=3, seed=SEED):
    return np.array([seed[0], seed[1], step, 0], dtype=np.uint32)


def dev_state(st):
    return torch.from_numpy(np.asarray(st, dtype=np.uint32).view(np.int32).copy()).cuda()


class Bufs:
    def __init__(self):
        self.outs = []

    def out(self, *shape):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.float32, device="cuda")
        buf[GUARD:GUARD + n] = float("nan")
        self.outs.append((buf, n))
        return buf[GUARD:GUARD + n].view(shape)

    @staticmethod
    def inp(a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        buf = torch.full((a.size + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        buf[GUARD:GUARD + a.size] = torch.from_numpy(a.reshape(-1)).cuda()
        return buf[GUARD:GUARD + a.size].view(a.shape)

    def intact(self):
        torch.cuda.synchronize()
        for buf, n in self.outs:
            assert bool((buf[:GUARD] == CANARY).all()) and bool((buf[GUARD + n:] == CANARY).all()), "write outside an output buffer"


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def untouched(*tensors):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(t).all()) for t in tensors)


def ok(got, ref, gate, tag):
    good, worst = WF.check(got, ref, gate, tag)
    assert good, (tag, worst)


def operands(rng, dt, *shape, sigma=1.0):
    a = rng.normal(0.0, sigma, shape).astype(np.float32)
    return MF.round_bf16(a) if dt == BF16 else a


def run_core(L, dt, q, k, v, dctx, left, right, p, tag):
    """forward (with and without lse) and two backward runs of the windowed entries, every element inside its gate"""
    B, t, H, dh = q.shape
    C = H * dh
    lib, P = L.lib(), L.ptr
    st, sid = state(), DF.stream_id(1, 0)
    keep, s = (DF.keep_attn(st, sid, B, H, t, p), DF.thr_scale(p)[1]) if p else (None, 1.0)
    rng_d = dev_state(st) if p else None
    R = P(rng_d) if p else None
    mode = "bf16" if dt == BF16 else "f32"
    ref = WF.core(q, k, v, left, right, dctx, keep=keep, s=s)
    b = Bufs()
    qkv = b.inp(MF.join_qkv(q, k, v))
    ctx, lse, ctx2 = b.out(B * t, C), b.out(B, H, t), b.out(B * t, C)
    L.check(lib.sed_mhsa_fwd_win(dt, P(qkv), P(ctx), P(lse), B, t, H, dh, left, right, p, R, sid, stream()), "mhsa_fwd_win")
    L.check(lib.sed_mhsa_fwd_win(dt, P(qkv), P(ctx2), None, B, t, H, dh, left, right, p, R, sid, stream()), "mhsa_fwd_win")
    b.intact()
    assert np.array_equal(bits(ctx), bits(ctx2)), (tag, "lse = NULL changed ctx")
    # the backward is fed the reference's ctx and lse rounded to fp32 (teacher-forced reference and gates; ctx and lse keep their own
    # gates in that call, so one evaluation of the gates serves both halves)
    ctx_in, lse_in, dctx_in = b.inp(ref["ctx"].reshape(B * t, C)), b.inp(ref["lse"]), b.inp(dctx.reshape(B * t, C))
    ctx32, lse32 = ctx_in.cpu().numpy().reshape(B, t, H, dh), lse_in.cpu().numpy()
    refb = WF.core(q, k, v, left, right, dctx, keep=keep, s=s, lse=lse32, ctx=ctx32)
    gb = WF.core_gates(q, k, v, left, right, dctx, keep=keep, s=s, mode=mode, lse=lse32, ctx=ctx32)
    ok(ctx.cpu().numpy().reshape(B, t, H, dh), ref["ctx"], gb["ctx"], (tag, "ctx"))
    ok(lse.cpu().numpy(), ref["lse"], gb["lse"], (tag, "lse"))
    nws = lib.sed_mhsa_bwd_ws_floats(B, t, H, dh)
    outs = []
    for _ in range(2):
        dqkv, ws = b.out(B * t, 3 * C), b.out(nws)
        L.check(lib.sed_mhsa_bwd_win(dt, P(qkv), P(ctx_in), P(dctx_in), P(lse_in), P(dqkv), P(ws), B, t, H, dh, left, right, p, R, sid,
                                     stream()), "mhsa_bwd_win")
        outs.append(dqkv)
    b.intact()
    assert np.array_equal(bits(outs[0]), bits(outs[1])), (tag, "two backward runs differ")
    dq, dk, dv = MF.split_qkv(outs[0].cpu().numpy(), B, t, H, dh)
    for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        ok(got, refb[name], gb[name], (tag, name))
    return ctx, lse, outs[0], (qkv, ctx_in, dctx_in, lse_in)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_core_per_element(L, case, dt):
    t, (H, dh), _, p = case
    left, right = window_of(case)
    B = 2
    rng = np.random.default_rng(1000 + 7 * t + H + left % 97)
    q, k, v, dctx = (operands(rng, dt, B, t, H, dh, sigma=sg) for sg in (1.5, 1.5, 1.0, 1.0))
    mode = "bf16" if dt == BF16 else "f32"
    run_core(L, dt, q, k, v, dctx, left, right, 0.0, (case_id(case), mode, "p0"))
    run_core(L, dt, q, k, v, dctx, left, right, p, (case_id(case), mode, f"p{p}"))
    lib = L.lib()
    for which in (0, 1, 2):
        assert lib.sed_mhsa_win_tiles(t, left, right, which) == WF.tiles_brute(t, left, right, which), (case_id(case), which)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("tw", [(65, (3, 0)), (130, (40, 7)), (130, (0, 33))], ids=str)
def test_loud_key(L, tw, dt):
    """Key J of every clip has a scaled score of 120 against every query.  Queries with J in their window put (almost) all their weight
    on it; for the others an unmasked exp(120 - lse) would be inf: they must equal the run in which key J is an ordinary key, bit for
    bit, and dq of theirs and dk / dv of J must carry nothing of them."""
    t, (left, right) = tw
    B, H, dh = 2, 2, 32
    J = t // 2 + 1
    rng = np.random.default_rng(5)
    q, k, v, dctx = (operands(rng, dt, B, t, H, dh, sigma=sg) for sg in (0.25, 0.25, 1.0, 1.0))
    # q = (a, small...) with column 0 fixed at 4, k_J column 0 = 120 sqrt(dh) / 4 (bf16-exact: 169.75 -> rounded): score ~ 120
    q[..., 0] = 4.0
    k[..., 0] = 0.0
    kJ = float(MF.round_bf16(np.float32(120.0 * np.sqrt(dh) / 4.0)))
    kl = k.copy()
    kl[:, J, :, 0] = kJ
    ctx, lse, dqkv, _ = run_core(L, dt, q, kl, v, dctx, left, right, 0.0, ("loud", tw, dt))
    for a in (ctx, lse, dqkv):
        assert bool(torch.isfinite(a).all()), "NaN / inf"
    w = WF.in_window(t, left, right)
    sees = w[:, J]
    got = ctx.cpu().numpy().reshape(B, t, H, dh)
    assert np.allclose(got[:, sees], v[:, J][:, None], atol=1e-6 + 2.0 ** -8 * np.abs(v[:, J][:, None]).max()), "not one-hot on the loud key"
    # the same inputs with key J ordinary: rows that do not see J are the same bits in ctx and lse (J is outside every sum of theirs)
    ctx0, lse0, dqkv0, _ = run_core(L, dt, q, k, v, dctx, left, right, 0.0, ("quiet", tw, dt))
    assert np.array_equal(bits(ctx).reshape(B, t, -1)[:, ~sees], bits(ctx0).reshape(B, t, -1)[:, ~sees]), "a trace of the loud key in ctx"
    assert np.array_equal(bits(lse)[:, :, ~sees], bits(lse0)[:, :, ~sees]), "a trace of the loud key in lse"
    # backward: dq of those rows is the same bits (key J enters masked cells only)
    dq, dq0 = bits(dqkv).reshape(B, t, 3, -1)[:, :, 0], bits(dqkv0).reshape(B, t, 3, -1)[:, :, 0]
    assert np.array_equal(dq[:, ~sees], dq0[:, ~sees]), "a trace of the loud key in dq"


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("tw", [(5, (1, 0)), (33, (3, 0)), (64, (3, 0)), (64, (31, 33)), (64, (0, 40))], ids=str)
def test_window_read_out_of_the_fused_forward(L, tw, p, dt):
    """q = k = 0: p_ij = 1 / n_i inside the window; V = the first t rows of the identity (t <= dh = 64): ctx[i][j] = m_ij s / n_i on
    in-window kept cells and 0 everywhere else"""
    t, (left, right) = tw
    B, H, dh = 2, 2, 64
    C = H * dh
    lib, P = L.lib(), L.ptr
    q = np.zeros((B, t, H, dh), dtype=np.float32)
    v = np.zeros((B, t, H, dh), dtype=np.float32)
    for j in range(t):
        v[:, j, :, j] = 1.0
    st, sid = state(step=11), DF.stream_id(0, 0)
    b = Bufs()
    qkv, ctx = b.inp(MF.join_qkv(q, q, v)), b.out(B * t, C)
    rng_d = dev_state(st)
    L.check(lib.sed_mhsa_fwd_win(dt, P(qkv), P(ctx), None, B, t, H, dh, left, right, p, P(rng_d) if p else None, sid, stream()),
            "mhsa_fwd_win")
    b.intact()
    got = ctx.cpu().numpy().reshape(B, t, H, dh).transpose(0, 2, 1, 3)
    w = WF.in_window(t, left, right)
    keep = DF.keep_attn(st, sid, B, H, t, p) if p else np.ones((B, H, t, t), dtype=np.uint8)
    live = (keep != 0) & w[None, None]
    assert np.array_equal(got[..., :t] != 0, live), "the fused forward keeps other cells than the window and sed_dropout_mask name"
    assert not got[..., t:].any()
    s = float(DF.thr_scale(p)[1]) if p else 1.0
    assert np.allclose(got[..., :t], live * (s / w.sum(axis=1))[None, None, :, None], rtol=2.0 ** -7, atol=0)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("tlr", [(5, 4, 4), (65, 64, UNB), (130, UNB, 129), (130, 500, 129)], ids=str)
def test_unbounded_window_gives_the_plain_entries_bits(L, tlr, p, dt):
    t, left, right = tlr
    B, H, dh = 2, 2, 32
    C = H * dh
    lib, P = L.lib(), L.ptr
    rng = np.random.default_rng(9)
    q, k, v, dctx = (operands(rng, dt, B, t, H, dh) for _ in range(4))
    st, sid = state(), DF.stream_id(0, 0)
    rng_d = dev_state(st)
    b = Bufs()
    qkv, dctx_in = b.inp(MF.join_qkv(q, k, v)), b.inp(dctx.reshape(B * t, C))
    ctx_w, lse_w, ctx_p, lse_p = b.out(B * t, C), b.out(B, H, t), b.out(B * t, C), b.out(B, H, t)
    L.check(lib.sed_mhsa_fwd_win(dt, P(qkv), P(ctx_w), P(lse_w), B, t, H, dh, left, right, p, P(rng_d) if p else None, sid, stream()), "win")
    if p:
        L.check(lib.sed_mhsa_fwd_drop(dt, P(qkv), P(ctx_p), P(lse_p), B, t, H, dh, p, P(rng_d), sid, stream()), "drop")
    else:
        L.check(lib.sed_mhsa_fwd(dt, P(qkv), P(ctx_p), P(lse_p), B, t, H, dh, stream()), "plain")
    nws = lib.sed_mhsa_bwd_ws_floats(B, t, H, dh)
    d_w, d_p, ws = b.out(B * t, 3 * C), b.out(B * t, 3 * C), b.out(nws)
    L.check(lib.sed_mhsa_bwd_win(dt, P(qkv), P(ctx_p), P(dctx_in), P(lse_p), P(d_w), P(ws), B, t, H, dh, left, right, p,
                                 P(rng_d) if p else None, sid, stream()), "win")
    if p:
        L.check(lib.sed_mhsa_bwd_drop(dt, P(qkv), P(ctx_p), P(dctx_in), P(lse_p), P(d_p), P(ws), B, t, H, dh, p, P(rng_d), sid, stream()), "drop")
    else:
        L.check(lib.sed_mhsa_bwd(dt, P(qkv), P(ctx_p), P(dctx_in), P(lse_p), P(d_p), P(ws), B, t, H, dh, stream()), "plain")
    b.intact()
    for a, c in ((ctx_w, ctx_p), (lse_w, lse_p), (d_w, d_p)):
        assert np.array_equal(bits(a), bits(c))


def test_refusals_leave_the_outputs_untouched(L):
    lib, P = L.lib(), L.ptr
    B, t, H, dh = 2, 33, 2, 32
    C = H * dh
    b = Bufs()
    qkv = b.inp(np.zeros((B * t, 3 * C)))
    cin, din, lin = b.inp(np.zeros((B * t, C))), b.inp(np.zeros((B * t, C))), b.inp(np.zeros((B, H, t)))
    ctx, lse, dqkv, ws = b.out(B * t, C), b.out(B, H, t), b.out(B * t, 3 * C), b.out(lib.sed_mhsa_bwd_ws_floats(B, t, H, dh))
    rng_d = dev_state(state())
    R = P(rng_d)
    nan = float("nan")
    bad = [dict(left=-1), dict(right=-1), dict(p=-0.1), dict(p=1.0), dict(p=nan), dict(p=0.5, rng=None), dict(dt=7), dict(t=0), dict(dh=48),
           dict(B=0), dict(H=0)]
    for kw in bad:
        a = dict(dt=F32, B=B, t=t, H=H, dh=dh, left=4, right=2, p=0.0, rng=R)
        a.update(kw)
        rc = lib.sed_mhsa_fwd_win(a["dt"], P(qkv), P(ctx), P(lse), a["B"], a["t"], a["H"], a["dh"], a["left"], a["right"], a["p"], a["rng"], 0,
                                  stream())
        assert rc != 0, ("forward accepted", kw)
        rc = lib.sed_mhsa_bwd_win(a["dt"], P(qkv), P(cin), P(din), P(lin), P(dqkv), P(ws), a["B"], a["t"], a["H"], a["dh"], a["left"],
                                  a["right"], a["p"], a["rng"], 0, stream())
        assert rc != 0, ("backward accepted", kw)
    assert lib.sed_mhsa_fwd_win(F32, None, P(ctx), P(lse), B, t, H, dh, 4, 2, 0.0, None, 0, stream()) != 0
    assert lib.sed_mhsa_fwd_win(F32, P(qkv), None, P(lse), B, t, H, dh, 4, 2, 0.0, None, 0, stream()) != 0
    assert lib.sed_mhsa_fwd_win(F32, P(qkv[0, 1:]), P(ctx), P(lse), B, t, H, dh, 4, 2, 0.0, None, 0, stream()) != 0
    assert lib.sed_mhsa_bwd_win(F32, P(qkv), P(cin), P(din), None, P(dqkv), P(ws), B, t, H, dh, 4, 2, 0.0, None, 0, stream()) != 0
    assert lib.sed_mhsa_bwd_win(F32, P(qkv), P(cin), P(din), P(lin), P(dqkv), None, B, t, H, dh, 4, 2, 0.0, None, 0, stream()) != 0
    assert untouched(ctx, lse, dqkv, ws)
    b.intact()
    for args in ((0, 1, 1, 0), (-3, 1, 1, 0), (33, -1, 0, 0), (33, 0, -1, 1), (33, 1, 1, 3), (33, 1, 1, -1)):
        assert lib.sed_mhsa_win_tiles(*args) == -1, args
    # p = 0 with a state given is no dropout as well, and the whole clip in tiles when unbounded
    assert lib.sed_mhsa_win_tiles(130, UNB, UNB, 0) == 25 and lib.sed_mhsa_win_tiles(130, 0, 0, 1) == 5
