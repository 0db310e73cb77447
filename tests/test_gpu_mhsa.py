"""GPU: the self-attention core of csrc/sed_mhsa.hip and the residual LayerNorm of csrc/sed_layernorm.hip through the C ABI, per element against the float64
definition in tests/mhsa_formula.py, within the gates derived in that file's docstring (SED_F32 and SED_BF16).

Shapes: B = 2 different clips (leakage between clips shows), t on, under and over the tile edges of the kernels (a wave owns 32
queries or keys and walks the other index in tiles of 32; a workgroup is four waves = 128), (H, dh) in {(1, 32), (4, 32), (2, 64)}.
Every input lies between NaN regions (a read past the B*t rows poisons an output: NaN * 0 is NaN), every output in a NaN-filled
buffer between canary regions.  The backward is fed lse and ctx as the reference rounded to fp32 (the gates assume that).

Beyond those random cases (bf16-representable operands in bf16 mode, as the gates of the "bf16" paragraph assume):
  many tiles   B = 3 clips, t = 257 and 384: three workgroups per (clip, head) (bh = blockIdx.x / ntile with ntile = 3 and an odd B),
               nine key tiles with a last tile of one key / twelve through the two LDS buffers
  ramp         scores +-6 (key tile): the running maximum of an even query rises at every key tile (o and l rescaled by
               alpha = exp(-6) each time), that of an odd query stays where tile 0 put it
  raw operands fp32 q, k, v (and dctx) that are not bf16-representable -- what the engine's GEMMs hand the core -- give the bits of the
               same values rounded to nearest even beforehand, forward and backward (dv alone under a raw dctx: D is taken from the
               fp32 dctx by design); and a raw dctx against float64 within the raw_dctx gates
Run with -s for the worst error / gate of every check.  Measured on the MI355X (worst over the shapes of a family; ctx lse dq dk dv):
  random (test_core_against_formula)    f32 0.016 0.025 0.011 0.009 0.040     bf16 0.61 0.026 0.17 0.15 0.80
  near one-hot                          f32 0.003 0.011 0.002 0.004 0.017     bf16 0.44 0.011 0.094 0.22 0.85
  constant scores                       f32 0.004 0.026 0.002 0.004 0.015     bf16 0.000 0.020 0.041 0.070 0.031
  many tiles                            f32 0.009 0.016 0.006 0.006 0.022     bf16 0.24 0.016 0.20 0.10 0.35
  ramp                                  f32 0.002 0.009 0.001 0.002 0.009     bf16 0.001 0.009 0.15 0.043 0.40
  raw dctx (bf16 only)                                                        bf16 0.38 0.021 0.16 0.15 0.52
  raw operands: bit for bit.  (The ramp's bf16 ctx is nearly exact because the kernel's unnormalised weights exp(s - m) of the
  dominant tile are exactly 1.)
Tried against local edits of csrc/sed_mhsa.hip that were not committed: truncation in place of nearest-even where the bf16 forward
stages K in LDS fails only test_bf16_rounds_its_operands_to_nearest_even (all four cases), and so does truncation of dctx as the
operand of dP in the dq kernel (at the D = 0 comparison alone: dq differs, dk and dv do not); a third workgroup that takes the second's
tile fails test_core_many_tiles (all eight) and the ramp at t = 257, and no case with t <= 130; o left without its alpha rescale
fails every ramp case (and most others with more than four key tiles)."""
import importlib

import numpy as np
import pytest
import torch

import mhsa_formula as F

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
GUARD = 1024
CANARY = -1024.0
F32, BF16 = 0, 1
T_SIZES = [1, 5, 32, 33, 63, 64, 65, 97, 127, 128, 129, 130]
HEADS = [(1, 32), (4, 32), (2, 64)]


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


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


def ok(got, ref, gate, tag):
    good, worst = F.check(got, ref, gate, tag)
    assert good, (tag, worst)


def run_core(L, dt, q, k, v, dctx, tag, raw_dctx=False):
    """forward (with and without lse), backward, each twice; every element against the formula.  raw_dctx: dctx is not
    bf16-representable (the gates then carry its operand rounding)"""
    B, t, H, dh = q.shape
    C = H * dh
    lib, P = L.lib(), L.ptr
    ref = F.core(q, k, v, dctx)
    gates = F.core_gates(q, k, v, dctx, "bf16" if dt == BF16 else "f32", raw_dctx=raw_dctx)
    b = Bufs()
    qkv_h = F.join_qkv(q, k, v)
    qkv = b.inp(qkv_h)
    ctx, lse, ctx2, ctx3, lse3 = b.out(B * t, C), b.out(B, H, t), b.out(B * t, C), b.out(B * t, C), b.out(B, H, t)
    L.check(lib.sed_mhsa_fwd(dt, P(qkv), P(ctx), P(lse), B, t, H, dh, stream()), "mhsa_fwd")
    L.check(lib.sed_mhsa_fwd(dt, P(qkv), P(ctx2), None, B, t, H, dh, stream()), "mhsa_fwd")
    L.check(lib.sed_mhsa_fwd(dt, P(qkv), P(ctx3), P(lse3), B, t, H, dh, stream()), "mhsa_fwd")
    b.intact()
    assert np.array_equal(qkv.cpu().numpy(), qkv_h), "an input was modified"
    ok(ctx.cpu().numpy().reshape(B, t, H, dh), ref["ctx"], gates["ctx"], (tag, "ctx"))
    ok(lse.cpu().numpy(), ref["lse"], gates["lse"], (tag, "lse"))
    assert np.array_equal(bits(ctx), bits(ctx2)), (tag, "lse = NULL changed ctx")
    assert np.array_equal(bits(ctx), bits(ctx3)) and np.array_equal(bits(lse), bits(lse3)), (tag, "two forward runs differ")
    # backward on the reference's ctx and lse rounded to fp32
    ctx_in, lse_in, dctx_in = b.inp(ref["ctx"].reshape(B * t, C)), b.inp(ref["lse"]), b.inp(dctx.reshape(B * t, C))
    nws = lib.sed_mhsa_bwd_ws_floats(B, t, H, dh)
    assert nws >= 1
    outs = []
    for _ in range(2):
        dqkv, ws = b.out(B * t, 3 * C), b.out(nws)
        L.check(lib.sed_mhsa_bwd(dt, P(qkv), P(ctx_in), P(dctx_in), P(lse_in), P(dqkv), P(ws), B, t, H, dh, stream()), "mhsa_bwd")
        outs.append(dqkv)
    b.intact()
    assert np.array_equal(bits(outs[0]), bits(outs[1])), (tag, "two backward runs differ")
    dq, dk, dv = F.split_qkv(outs[0].cpu().numpy(), B, t, H, dh)
    for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        ok(got, ref[name], gates[name], (tag, name))


def operands(rng, dt, *shape, sigma=1.0):
    a = rng.normal(0.0, sigma, shape).astype(np.float32)
    return F.round_bf16(a) if dt == BF16 else a


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("hd", HEADS, ids=lambda v: f"H{v[0]}dh{v[1]}")
@pytest.mark.parametrize("t", T_SIZES)
def test_core_against_formula(L, t, hd, dt):
    H, dh = hd
    rng = np.random.default_rng(1000 * t + 10 * H + dt)
    q, k, v, d = (operands(rng, dt, 2, t, H, dh, sigma=s) for s in (1.0, 1.0, 1.0, 0.1))
    run_core(L, dt, q, k, v, d, (t, hd, dt))


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("hd", HEADS, ids=lambda v: f"H{v[0]}dh{v[1]}")
def test_near_one_hot_rows_and_constant_scores(L, hd, dt):
    H, dh = hd
    B, t = 2, 65
    rng = np.random.default_rng(7 + H + dt)
    # near one-hot: k rows of +-1, q_i = +-60/sqrt(dh) k_pi(i): the scaled score is +-60 at j = pi(i), 60 (k_pi . k_j)/dh elsewhere
    k = np.where(rng.random((B, t, H, dh)) > 0.5, 1.0, -1.0).astype(np.float32)
    pi = rng.integers(0, t, (B, t, H))
    sign = np.where(np.arange(t) % 3 == 0, -1.0, 1.0)[None, :, None, None]
    q = np.take_along_axis(k, pi[..., None], axis=1) * sign * (60.0 / np.sqrt(dh))
    q = F.round_bf16(q.astype(np.float32))
    v, d = operands(rng, dt, B, t, H, dh), operands(rng, dt, B, t, H, dh, sigma=0.1)
    s = F.core(q, k, v)["s"]
    assert 55.0 < s.max() < 65.0 and -65.0 < s.min() < -55.0 and F.core(q, k, v)["p"].max() > 0.999
    run_core(L, dt, q, k, v, d, ("one-hot", hd, dt))
    # constant scores: every key of a clip is the same vector -> uniform weights 1/t
    k = np.broadcast_to(operands(rng, dt, B, 1, H, dh), (B, t, H, dh)).copy()
    q = operands(rng, dt, B, t, H, dh)
    assert np.allclose(F.core(q, k, v)["p"], 1.0 / t, rtol=1e-12)
    run_core(L, dt, q, k, v, d, ("constant", hd, dt))


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("hd", [(4, 32), (2, 64)], ids=lambda v: f"H{v[0]}dh{v[1]}")
@pytest.mark.parametrize("t", [257, 384])
def test_core_many_tiles(L, t, hd, dt):
    """B = 3 (odd) clips and three workgroups per (clip, head): bh = blockIdx.x / ntile with ntile = 3.  t = 257: nine key tiles,
    the last of one key (and one query in the third workgroup); t = 384: three full workgroups, twelve key tiles through the two
    LDS buffers of the bf16 forward"""
    H, dh = hd
    assert (t + 127) // 128 == 3 and (t + 31) // 32 in (9, 12)
    rng = np.random.default_rng(1000 * t + 10 * H + dt)
    q, k, v, d = (operands(rng, dt, 3, t, H, dh, sigma=s) for s in (1.0, 1.0, 1.0, 0.1))
    run_core(L, dt, q, k, v, d, ("many tiles", t, hd, dt))


RAMP_STEP = 6.0


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("hd", HEADS, ids=lambda v: f"H{v[0]}dh{v[1]}")
@pytest.mark.parametrize("t", [130, 257])
def test_score_ramp_over_the_key_tiles(L, t, hd, dt):
    """k_j = w (j // 32), q_i = +-(step / sqrt(dh)) w with w a +-1 vector per (clip, head): the scaled score is about +-step (key tile).
    An even query's running maximum rises by step at EVERY key tile (o and l are rescaled by alpha = exp(-step) each time), an odd
    query's is fixed from tile 0 on (alpha = 1, every later weight tiny).  step (tiles - 1) <= 80 keeps every exp in fp32's normal
    range: the gates are relative and do not model underflow."""
    H, dh = hd
    B = 2
    tiles = (t + 31) // 32
    assert RAMP_STEP * (tiles - 1) <= 80.0
    rng = np.random.default_rng(50 * t + H + dt)
    w = np.where(rng.random((B, 1, H, dh)) > 0.5, 1.0, -1.0).astype(np.float32)
    k = (w * (np.arange(t) // 32).astype(np.float32)[None, :, None, None]).astype(np.float32)
    sigma = np.where(np.arange(t) % 2 == 0, 1.0, -1.0).astype(np.float32)[None, :, None, None]
    q = F.round_bf16((sigma * w * np.float32(RAMP_STEP / np.sqrt(dh))).astype(np.float32))
    assert np.array_equal(F.round_bf16(k), k)
    v, d = operands(rng, dt, B, t, H, dh), operands(rng, dt, B, t, H, dh, sigma=0.1)
    r = F.core(q, k, v)
    s, p = r["s"], r["p"]
    last = (tiles - 1) * 32
    assert np.allclose(s[:, :, 0::2, last:], RAMP_STEP * (tiles - 1), rtol=2e-2) and np.allclose(s[:, :, 1::2, last:], -RAMP_STEP * (tiles - 1), rtol=2e-2)
    assert (p[:, :, 0::2].argmax(axis=3) >= last).all(), "an even query's largest weight is not in the last key tile"
    assert (p[:, :, 1::2].argmax(axis=3) < 32).all() and (p[:, :, 1::2, :32].sum(axis=3) > 0.99).all()
    run_core(L, dt, q, k, v, d, ("ramp", t, hd, dt))


@pytest.mark.parametrize("hd", [(4, 32), (2, 64)], ids=lambda v: f"H{v[0]}dh{v[1]}")
@pytest.mark.parametrize("t", [33, 130])
def test_bf16_rounds_its_operands_to_nearest_even(L, t, hd):
    """SED_BF16 on fp32 values that are NOT bf16-representable (what the engine's GEMMs hand the core) gives the bits it gives for the
    same values rounded to nearest even beforehand: the LDS forward's staging, the register-fed fragments of forward and backward
    and the load_col operands all round the same way.  D is taken from the fp32 dctx by design, so under a raw dctx only dv (which
    does not depend on D) is compared -- and, with a ctx input of zeros (D = 0 for either dctx), the whole of dqkv."""
    H, dh = hd
    B, C = 2, H * dh
    lib, P = L.lib(), L.ptr
    rng = np.random.default_rng(900 + t + H)
    q, k, v = (rng.normal(0.0, 1.0, (B, t, H, dh)).astype(np.float32) for _ in range(3))
    d_raw = rng.normal(0.0, 0.1, (B, t, H, dh)).astype(np.float32)
    for a in (q, k, v, d_raw):
        assert (F.round_bf16(a) != a).mean() > 0.9, "rounding changes too few elements to show anything"
        trunc = (a.view(np.uint32) & 0xFFFF0000).view(np.float32)
        assert (F.round_bf16(a) != trunc).mean() > 0.4, "nearest-even and truncation agree too often to tell them apart"
    qr, kr, vr, d_rnd = (F.round_bf16(a) for a in (q, k, v, d_raw))
    ref = F.core(qr, kr, vr)
    b = Bufs()
    raw, rnd = b.inp(F.join_qkv(q, k, v)), b.inp(F.join_qkv(qr, kr, vr))
    fwd = {}
    for name, qkv in (("raw", raw), ("raw again", raw), ("rounded", rnd)):
        ctx, lse = b.out(B * t, C), b.out(B, H, t)
        L.check(lib.sed_mhsa_fwd(BF16, P(qkv), P(ctx), P(lse), B, t, H, dh, stream()), "mhsa_fwd")
        fwd[name] = (ctx, lse)
    b.intact()
    for i, what in enumerate(("ctx", "lse")):
        assert not bool(torch.isnan(fwd["raw"][i]).any()), what
        assert np.array_equal(bits(fwd["raw"][i]), bits(fwd["raw again"][i])), (what, "two forward runs differ")
        assert np.array_equal(bits(fwd["raw"][i]), bits(fwd["rounded"][i])), (what, "raw q, k, v are not rounded to nearest even in the forward")
    ctx_in, lse_in = b.inp(ref["ctx"].reshape(B * t, C)), b.inp(ref["lse"])
    nws = lib.sed_mhsa_bwd_ws_floats(B, t, H, dh)
    dd_rnd, dd_raw = b.inp(d_rnd.reshape(B * t, C)), b.inp(d_raw.reshape(B * t, C))
    bwd = {}
    zero_ctx = b.inp(np.zeros((B * t, C)))          # D = 0 whatever dctx is: dctx then enters dq and dk through the operand of dP alone
    for name, qkv, cc, dd in (("raw", raw, ctx_in, dd_rnd), ("raw again", raw, ctx_in, dd_rnd), ("rounded", rnd, ctx_in, dd_rnd),
                              ("raw dctx", rnd, ctx_in, dd_raw), ("D = 0", rnd, zero_ctx, dd_rnd), ("D = 0, raw dctx", rnd, zero_ctx, dd_raw)):
        dqkv, ws = b.out(B * t, 3 * C), b.out(nws)
        L.check(lib.sed_mhsa_bwd(BF16, P(qkv), P(cc), P(dd), P(lse_in), P(dqkv), P(ws), B, t, H, dh, stream()), "mhsa_bwd")
        bwd[name] = dqkv
    b.intact()
    assert not bool(torch.isnan(bwd["raw"]).any())
    assert np.array_equal(bits(bwd["raw"]), bits(bwd["raw again"])), "two backward runs differ"
    assert np.array_equal(bits(bwd["raw"]), bits(bwd["rounded"])), "raw q, k, v are not rounded to nearest even in the backward"
    dv = [F.split_qkv(bits(bwd[n]), B, t, H, dh)[2] for n in ("rounded", "raw dctx")]
    assert np.array_equal(dv[0], dv[1]), "a raw dctx is not rounded to nearest even as the operand of dV"
    dq = [F.split_qkv(bits(bwd[n]), B, t, H, dh)[0] for n in ("rounded", "raw dctx")]
    assert not np.array_equal(dq[0], dq[1]), "D is documented to come from the fp32 dctx: dq should see the raw values"
    assert not bool(torch.isnan(bwd["D = 0"]).any()) and not np.array_equal(bits(bwd["D = 0"]), bits(bwd["rounded"]))
    assert np.array_equal(bits(bwd["D = 0"]), bits(bwd["D = 0, raw dctx"])), "a raw dctx is not rounded to nearest even as the operand of dP"


@pytest.mark.parametrize("hd", HEADS, ids=lambda v: f"H{v[0]}dh{v[1]}")
@pytest.mark.parametrize("t", [65, 130])
def test_bf16_raw_dctx_against_formula(L, t, hd):
    """representable q, k, v and a raw fp32 dctx (sigma 0.1), against float64 on the raw dctx within the raw_dctx gates"""
    H, dh = hd
    rng = np.random.default_rng(77 * t + H)
    q, k, v = (operands(rng, BF16, 2, t, H, dh) for _ in range(3))
    d = rng.normal(0.0, 0.1, (2, t, H, dh)).astype(np.float32)
    assert (F.round_bf16(d) != d).mean() > 0.9
    run_core(L, BF16, q, k, v, d, ("raw dctx", t, hd), raw_dctx=True)


def test_refusals_launch_nothing(L):
    lib, P = L.lib(), L.ptr
    b = Bufs()
    B, t, H, dh = 2, 5, 1, 32
    C = H * dh
    qkv = b.inp(np.zeros((B * t, 3 * C)))
    ctx, lse, dqkv, ws = b.out(B * t + 1, C), b.out(B, H, t), b.out(B * t, 3 * C), b.out(B * t * H)
    st = stream()
    f32 = F32
    bad = [lib.sed_mhsa_fwd(f32, P(qkv), P(ctx), P(lse), 0, t, H, dh, st), lib.sed_mhsa_fwd(f32, P(qkv), P(ctx), P(lse), B, 0, H, dh, st),
           lib.sed_mhsa_fwd(f32, P(qkv), P(ctx), P(lse), B, t, 0, dh, st), lib.sed_mhsa_fwd(f32, P(qkv), P(ctx), P(lse), B, -1, H, dh, st),
           lib.sed_mhsa_fwd(f32, P(qkv), P(ctx), P(lse), B, t, H, 48, st), lib.sed_mhsa_fwd(f32, P(qkv), P(ctx), P(lse), B, t, H, 16, st),
           lib.sed_mhsa_fwd(f32, P(qkv), P(ctx), P(lse), B, t, H, 128, st), lib.sed_mhsa_fwd(2, P(qkv), P(ctx), P(lse), B, t, H, dh, st),
           lib.sed_mhsa_fwd(f32, None, P(ctx), P(lse), B, t, H, dh, st), lib.sed_mhsa_fwd(f32, P(qkv), None, P(lse), B, t, H, dh, st),
           lib.sed_mhsa_fwd(f32, P(qkv), ctx.data_ptr() + 4, P(lse), B, t, H, dh, st),
           lib.sed_mhsa_fwd(f32, P(qkv), P(ctx), P(lse), 1, 1 << 22, 2, 32, st),        # 2^22 * 192 * 4 bytes >= 2^31 inside a clip
           lib.sed_mhsa_bwd(f32, P(qkv), P(ctx), P(ctx), P(lse), P(dqkv), P(ws), B, t, H, 48, st),
           lib.sed_mhsa_bwd(f32, P(qkv), P(ctx), P(ctx), P(lse), P(dqkv), P(ws), B, 0, H, dh, st),
           lib.sed_mhsa_bwd(f32, P(qkv), P(ctx), P(ctx), None, P(dqkv), P(ws), B, t, H, dh, st),
           lib.sed_mhsa_bwd(f32, P(qkv), P(ctx), P(ctx), P(lse), None, P(ws), B, t, H, dh, st),
           lib.sed_mhsa_bwd(f32, P(qkv), P(ctx), P(ctx), P(lse), P(dqkv), None, B, t, H, dh, st),
           lib.sed_mhsa_bwd(f32, None, P(ctx), P(ctx), P(lse), P(dqkv), P(ws), B, t, H, dh, st),
           lib.sed_mhsa_bwd(f32, P(qkv), None, P(ctx), P(lse), P(dqkv), P(ws), B, t, H, dh, st),
           lib.sed_mhsa_bwd(f32, P(qkv), P(ctx), None, P(lse), P(dqkv), P(ws), B, t, H, dh, st),
           lib.sed_add_layernorm_fwd(P(qkv), P(qkv), P(qkv), P(qkv), P(ctx), None, 0, C, 1e-5, st),
           lib.sed_add_layernorm_fwd(P(qkv), P(qkv), P(qkv), P(qkv), P(ctx), None, 4, 0, 1e-5, st),
           lib.sed_add_layernorm_fwd(P(qkv), None, P(qkv), P(qkv), P(ctx), None, 4, C, 1e-5, st),
           lib.sed_add_layernorm_fwd(P(qkv), P(qkv), P(qkv), P(qkv), None, None, 4, C, 1e-5, st),
           lib.sed_add_layernorm_bwd(P(qkv), P(qkv), P(qkv), P(qkv), None, P(ctx), P(lse), P(lse), P(ws), 4, C, st),
           lib.sed_add_layernorm_bwd(P(qkv), P(qkv), P(qkv), P(qkv), P(qkv), P(ctx), P(lse), P(lse), None, 4, C, st),
           lib.sed_add_layernorm_bwd(P(qkv), P(qkv), P(qkv), P(qkv), P(qkv), P(ctx), P(lse), P(lse), P(ws), 0, C, st)]
    assert all(rc != 0 for rc in bad), bad
    assert lib.sed_last_error()
    b.intact()
    for o in (ctx, lse, dqkv, ws):
        assert bool(torch.isnan(o).all()), "a refused call wrote an output"
    assert lib.sed_mhsa_bwd_ws_floats(B, t, H, dh) == B * t * H and lib.sed_mhsa_bwd_ws_floats(0, t, H, dh) == 0
    assert lib.sed_add_layernorm_bwd_ws_floats(0, C) == 0 and lib.sed_add_layernorm_bwd_ws_floats(65, C) == 2 * 2 * C


@pytest.mark.parametrize("C", [32, 96, 128, 512])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 63, 64, 65, 129])
def test_add_layernorm_against_formula(L, rows, C):
    """rows around one forward workgroup's share (4) and one backward partial's (64)"""
    lib, P = L.lib(), L.ptr
    rng = np.random.default_rng(rows * 1000 + C)
    x = rng.normal(0.3, 1.0, (rows, C)).astype(np.float32)
    a = rng.normal(-0.1, 0.5, (rows, C)).astype(np.float32)
    gamma, beta = rng.normal(1.0, 0.3, C).astype(np.float32), rng.normal(0.0, 0.3, C).astype(np.float32)
    dy = rng.normal(0.0, 0.1, (rows, C)).astype(np.float32)
    ref = F.add_layernorm(x, a, gamma, beta, dy)
    gates = F.add_layernorm_gates(x, a, gamma, beta, dy)
    b = Bufs()
    dx, da, dg, db, ddy = (b.inp(v) for v in (x, a, gamma, beta, dy))
    y, stats, y2 = b.out(rows, C), b.out(rows, 2), b.out(rows, C)
    L.check(lib.sed_add_layernorm_fwd(P(dx), P(da), P(dg), P(db), P(y), P(stats), rows, C, 1e-5, stream()), "add_layernorm_fwd")
    L.check(lib.sed_add_layernorm_fwd(P(dx), P(da), P(dg), P(db), P(y2), None, rows, C, 1e-5, stream()), "add_layernorm_fwd")
    b.intact()
    tag = (rows, C)
    ok(y.cpu().numpy(), ref["y"], gates["y"], (tag, "y"))
    assert np.array_equal(bits(y), bits(y2)), "stats = NULL changed y"
    # the statistics: the mean is a C-term sum, rstd carries the error of the centred squares
    z = ref["z"]
    M = np.abs(z).mean(axis=1)
    d = np.abs(z - ref["mean"][:, None])
    k = (C + 8) * F.U
    st_h = stats.cpu().numpy()
    ok(st_h[:, 0], ref["mean"], k * M, (tag, "mean"))
    ok(st_h[:, 1], ref["rstd"], k * ref["rstd"] * (1.0 + ref["rstd"] ** 2 * (d * (np.abs(z) + M[:, None])).mean(axis=1)), (tag, "rstd"))
    stats_in = b.inp(np.stack([ref["mean"], ref["rstd"]], axis=1))
    nws = lib.sed_add_layernorm_bwd_ws_floats(rows, C)
    assert nws == (rows + 63) // 64 * 2 * C
    outs = []
    for _ in range(2):
        dres, dgam, dbet, ws = b.out(rows, C), b.out(C), b.out(C), b.out(nws)
        L.check(lib.sed_add_layernorm_bwd(P(ddy), P(dx), P(da), P(dg), P(stats_in), P(dres), P(dgam), P(dbet), P(ws), rows, C, stream()),
                "add_layernorm_bwd")
        outs.append((dres, dgam, dbet))
    b.intact()
    for u, w in zip(*outs):
        assert np.array_equal(bits(u), bits(w)), "two backward runs differ"
    for name, got in zip(("dres", "dgamma", "dbeta"), outs[0]):
        ok(got.cpu().numpy(), ref[name], gates[name], (tag, name))
    for dv, hv in ((dx, x), (da, a), (dg, gamma), (db, beta), (ddy, dy)):
        assert np.array_equal(dv.cpu().numpy(), hv), "an input was modified"
