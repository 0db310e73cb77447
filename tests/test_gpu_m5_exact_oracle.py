"""GPU: the raw-waveform M5 kernels of csrc/sed_m5.hip and csrc/sed_m5_mfma.hip -- the k = 79 / stride 4 first convolution in every
form (forward, statistics, fused BN + ReLU + MaxPool forward, the weight-gradient family), the MaxPool1d(4) kernels on a given z
and the mean-over-time + Linear head -- per element
against float64, through the C ABI.  (sed_m5_conv1_dgrad* has its own gate in tests/test_gpu_m5_input_grad.py.)

Reference: the same operation in float64 (torch) ON THE OPERANDS THE KERNEL READS: where a kernel rounds x, w, z or dy to bf16 on load
the reference rounds them too.  No kernel of this library serves as a reference (bit-identities the header promises between two entry
points are asserted on top, never instead).  Every output and workspace buffer starts as NaN and is followed (and preceded) by a NaN
guard region that must still be NaN after the launch; x is a pointer into a larger NaN-filled allocation, so a read before frame 0 or
past the last frame poisons the result.  No element is excluded from any comparison.  Every conv1 kernel runs at its default grid and
under SED_M5_BLOCKS = 3 and 7 (workgroups then own several tiles, unequal numbers of them, cross frames and the b >> 3 group
boundary); partial rows are summed here in float64 and every one of the sed_m5_conv1_nparts rows must have been written.

Gate, per element: |got - ref| <= c * S (+ the terms below), S = the same contraction over absolute values.  u = 2^-24 (one fp32
rounding), a bf16 rounding is the true half ulp of the value (2^-9 .. 2^-8 relative), SAFE = 4 multiplies every operation COUNT (not the bf16 half
ulps, which are hard bounds).  Nothing below was set from a measurement.  tpb = ceil(B * tiles / nparts) = tiles per workgroup.

  z              VALU form (SED_F32, and SED_BF16 under SED_M5_MFMA=0: fp32 operands): a serial chain of 79 fmas, c = SAFE * 79 u.
                 MFMA form: x and w rounded to bf16 (the reference rounds them), products exact in fp32, 80 accumulations in the
                 matrix pipe's order, c = SAFE * 80 u.  bf16 stores add half a bf16 ulp of (|ref| + the fp32 bound).
  z statistics   what is summed: the VALU kernel sums its fp32 ACCUMULATORS (also when it stores bf16), the MFMA kernels sum the
                 bf16-ROUNDED values as stored.  The reference sums exactly those values in float64 (the stored tensor; for the
                 VALU bf16 form the SED_F32 launch's z, whose rounding the bf16 z must equal bit for bit).  A thread adds 4 rows
                 per tile, the workgroup 32 threads per channel: c = SAFE * (4 tpb + 32) u of sum |v|, one more (the fma) for v^2.
  y              fused BN + ReLU + MaxPool: a maximum is 1-Lipschitz, so |y - yref| <= max over the window of |scale| * (z's gate)
                 + SAFE * u * (|scale z| + |shift|) (the fma), plus the bf16 store.  No arg-max decision enters.
  decisions      sed_m5_conv1_wgrad_fused_pool decides on the stored z; next to separated pre-activations it gets
                 inputs for which z and every pre-activation are exact in fp32 AND bf16 (integer x in [-8, 8], six taps of +-1 per
                 channel, scale = +-2^k, shift = (j + 1/2)/8; asserted on the CPU first), so ties and non-positive windows are
                 genuine and "first arg-max, maximum > 0" is applied exactly by the reference.
  weight grads   dW[k][c] = sum_{b,t} dz[b,t,c] x[b][4t+k-39], S = sum Dabs |x|.  VALU kernel (dz given, fp32 x): a chain of 128
                 fmas per tile, c = SAFE * 128 tpb u, Dabs = |dz|.  MFMA kernels (bf16 x): 32 tpb accumulations per wave + 3 adds
                 over the waves, and dz = fma(ca, g, fma(cb, z, cc)) is two fp32 roundings of Dabs = |ca g| + |cb z| + |cc| and ONE
                 bf16 rounding: gate = sum_t h(dz) |x| + SAFE * (32 tpb + 5) u * S, h(v) = the true half bf16 ulp of |v| (+ its fp32
                 slop): 2^-9 |v| only at the top of a binade, up to 2^-8 |v| at its bottom (bf16 has 8 significand bits), so a flat
                 2^-9 * S is NOT a bound -- the first version of this module assumed it and integer-valued data showed 1.36 x.
  tap row 79     unspecified (the VALU kernel leaves a contraction there, the MFMA kernels 0): consumers read rows 0..78.  The
                 tests never read it as dW and require it to be written.
  pool stats     (sum g, sum g*xhat): g is dy or 0 exactly; a thread adds 4 terms per window (the sed_maxpool4 kernels: n = 4 *
                 windows per thread + 256 / (Cp/8)), xhat = (z - mean) * invstd and the fma add 3.
  maxpool4       forward: one fma, c = SAFE * u of max over the window of |scale z| + |shift|, plus the bf16 store.  Backward: g bit
                 for bit (dy or +0; rows dropped by the floor +0).  pooled_stats: the float64 value of the kernel's own formula on
                 the y it is given; q = (rt - beta st) * (invstd / scale) costs the accumulation and 6 more roundings of
                 S = (sum |dy y| + |beta| sum |dy|) |invstd / scale|.
  head           m: H - 1 adds and the division, c = SAFE * H u.  pre: ceil(C/64) fmas, 6 shuffle levels, the bias: c = SAFE *
                 (ceil(C/64) + 7) u of sum |m w| + |b|, plus sum |w| (m's gate).  dfc_w: at most ceil(B/4) fmas and 10 adds on any
                 path; dfc_b: ceil(B/4) + 3.  dfeat: K fmas and the division by H, plus the bf16 store; the same bits for every h,
                 +0 in channels [C, Cp).

Measured max err / gate on the MI355X (printed per check at the end of the module with -s; head / tail / all agree to the digits shown):
  z              f32 0.020; bf16 VALU 0.991, bf16 MFMA 0.992 (the storage half ulp is the error and the gate); y 0.989
  z statistics   sum z 0.003 (VALU) / 0.0004 (MFMA), sum z^2 0.017: worst-case operation counts against errors that add like a random walk
  weight grads   VALU f32 / bf16 0.002 (a 128 tpb chain, tpb up to 27); fused 0.84, fused_pool 0.85 separated / 0.74 exact
                 (the bf16 rounding of dz is the error and the gate)
  maxpool4       forward f32 0.25 (one rounding = the count without SAFE; 0 on the exact data), bf16 0.9999; relu_bwd statistics 0.04;
                 pooled_stats sum g 0.06, sum g*xhat 0.04; g, dropped rows, zero rows, flags bit for bit
  head           m 0.20, pre 0.04, dfc_w 0.05, dfc_b 0.06, dfeat 0.24 (f32) / 0.9999 (bf16)
No kernel missed its gate.  The module runs in about 6 s.
"""
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
F32, BF16 = 0, 1
DT = {F32: torch.float32, BF16: torch.bfloat16}
NAME = {F32: "f32", BF16: "bf16"}
U = 2.0 ** -24
SAFE = 4.0
GUARD = 1024                    # NaN elements on each side of every output / workspace buffer (keeps 16-byte alignment)
XPAD = 256                      # NaN floats on each side of x
TT = 128                        # conv1 outputs per tile
LENGTHS = [13, 316, 505, 509, 513, 2045, 2049, 2050, 2051, 2053, 2057]
BLOCKS = [None, "3", "7"]
RATIOS = {}                     # (kernel, check) -> max err / gate


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)._lib


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if RATIOS:
        print("\nmax err / gate by kernel and check (1.0 = at the derived bound)")
        for k in sorted(RATIOS):
            print(f"  {k[0]:34s} {k[1]:28s} {RATIOS[k]:.3e}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def cdiv(a, b):
    return -(-a // b)


class Guards:
    """output / workspace buffers: NaN inside, a NaN guard region on both sides, checked by intact()"""

    def __init__(self):
        self.bufs = []

    def new(self, shape, dtype=torch.float32):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = math.prod(shape)
        buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
        self.bufs.append((buf, n))
        return buf[GUARD:GUARD + n].view(shape)

    def intact(self):
        torch.cuda.synchronize()
        for buf, n in self.bufs:
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), "write outside an output buffer"
        self.bufs = []


def guarded_x(x):
    """x [B][L] (CPU or GPU) as a view into a larger NaN-filled device allocation"""
    n = x.numel()
    buf = torch.full((n + 2 * XPAD,), float("nan"), device="cuda")
    buf[XPAD:XPAD + n] = x.reshape(-1).cuda()
    return buf[XPAD:XPAD + n].view(x.shape), buf


def bf16_half_ulp(v):
    """half a bf16 ulp of |v| (float64): |v| = m * 2^e with m in [0.5, 1) -> ulp 2^(e-8)"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.exp2(e.double() - 9.0)


def rbf(t):
    """round to bf16, back as float64"""
    return t.float().bfloat16().double()


def gate_check(kernel, check, got, ref, gate, regions=None):
    """|got - ref| <= gate for EVERY element; records max err / gate for the named regions (boolean masks) and the full tensor"""
    got = got.double()
    assert got.shape == ref.shape, (kernel, check, got.shape, ref.shape)
    assert not bool(torch.isnan(got).any()), f"{kernel} {check}: NaN in the output (an element not written, or a poisoned read)"
    gate = gate.expand_as(ref) if torch.is_tensor(gate) else torch.full_like(ref, gate)
    err = (got - ref).abs()
    ratio = torch.where(gate > 0, err / gate.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    for name, mask in list((regions or {}).items()) + [("all", None)]:
        r = ratio if mask is None else ratio[mask.expand_as(ratio)]
        if r.numel() == 0:
            continue
        key = (kernel, f"{check} {name}".strip())
        RATIOS[key] = max(RATIOS.get(key, 0.0), float(r.max()))
    if not bool((err <= gate).all()):
        i, idx = int(ratio.argmax()), ()
        for n in reversed(ratio.shape):
            idx = (i % n,) + idx
            i //= n
        i = int(ratio.argmax())
        raise AssertionError(f"{kernel} {check}: err/gate {float(ratio.reshape(-1)[i]):.3e} at {idx}: got {float(got[idx])!r} ref "
                             f"{float(ref[idx])!r} gate {float(gate[idx]):.3e}; {int((err > gate).sum())} of {err.numel()} elements miss")


def same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    assert torch.equal(a.contiguous().view(it), b.contiguous().view(it)), f"{what}: not the same bits"


# ---- layout and float64 references of conv_block1.0 ------------------------------------------------------------------------------
def to_eng(t):
    """(B, L1, C) -> engine layout [B/8][L1][8][C]"""
    B, L1, C = t.shape
    return t.reshape(B // 8, 8, L1, C).permute(0, 2, 1, 3).contiguous()


def from_eng(t):
    """engine layout [B/8][L1][8][C] -> (B, L1, C)"""
    N, L1, f, C = t.shape
    return t.permute(0, 2, 1, 3).reshape(N * f, L1, C)


def conv_len(Lx):
    return (Lx - 1) // 4 + 1


def patches(x64, L1):
    """P[b][t][k] = x[b][4t + k - 39] (0 outside the frame), float64 (B, L1, 79)"""
    return F.pad(x64, (39, 4 * L1 + 79)).unfold(1, 79, 4)[:, :L1]


def z_regions(Lx, L1, pooled=False):
    """head outputs (window reaches src < 0), tail outputs (src >= L) over the time axis of an engine-layout tensor"""
    t = torch.arange(L1, device="cuda")
    head, tail = 4 * t - 39 < 0, 4 * t + 39 >= Lx
    if pooled:
        Ho = L1 // 4
        head, tail = head[:4 * Ho].view(Ho, 4).any(1), tail[:4 * Ho].view(Ho, 4).any(1)
    return {"head": head.view(1, -1, 1, 1), "tail": tail.view(1, -1, 1, 1)}


def dw_regions(Lx, L1):
    """taps whose window reaches src < 0 at t = 0, and src >= L at t = L1 - 1, over a [79][64] weight gradient"""
    k = torch.arange(79, device="cuda")
    return {"head": (k - 39 < 0).view(-1, 1), "tail": (4 * (L1 - 1) + k - 39 >= Lx).view(-1, 1)}


def first_argmax_g(pre, dy64):
    """MaxPool1d(4) + ReLU backward on exact pre-activations [N][H][W][C]: dy at the FIRST arg-max of each window when that maximum is
    > 0, else 0; rows dropped by the floor 0.  Returns (g, number of windows with a tied positive maximum, windows with maximum <= 0)."""
    N, H, W, C = pre.shape
    Ho = H // 4
    win = pre[:, :4 * Ho].reshape(N, Ho, 4, W, C).clamp_min(0)
    best = win.amax(dim=2, keepdim=True)
    at = win == best
    first = at & (at.cumsum(2) == 1)                                 # the first position that attains the maximum
    g = torch.where(first & (best > 0), dy64.unsqueeze(2).expand_as(win), torch.zeros_like(win))       # (+0 elsewhere, never -0)
    out = torch.zeros_like(pre)
    out[:, :4 * Ho] = g.reshape(N, 4 * Ho, W, C)
    ties = int((((win == best).sum(2, keepdim=True) > 1) & (best > 0)).sum())
    return out, ties, int((best <= 0).sum())


class Env:
    """SED_M5_* knobs for one block of launches; the library caches them, sed_config_reload is the test hook"""

    def __init__(self, L, monkeypatch):
        self.L, self.mp = L, monkeypatch

    def set(self, **kv):
        for k, v in kv.items():
            if v is None:
                self.mp.delenv(k, raising=False)
            else:
                self.mp.setenv(k, v)
        self.L.lib().sed_config_reload()

    def restore(self):
        self.set(SED_M5_BLOCKS=None, SED_M5_MFMA=None)


def nparts_and_tpb(lib, B, Lx, blocks):
    L1 = lib.sed_m5_conv1_len(Lx)
    tiles = B * cdiv(L1, TT)
    npt = lib.sed_m5_conv1_nparts(B, Lx)
    assert npt == min(tiles, int(blocks) if blocks else 1024)
    return npt, cdiv(tiles, npt)


def sum_rows(part, what):
    """float64 sum of the partial rows; every row must have been written"""
    assert not bool(torch.isnan(part).any()), f"{what}: a partial row was not written"
    return part.double().sum(0)


# ---- 1. conv_block1 forward family ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [8, 16])
@pytest.mark.parametrize("Lx", LENGTHS)
def test_conv1_forward_family(L, monkeypatch, Lx, B):
    lib, P, st = L.lib(), L.ptr, _stream()
    gen = torch.Generator().manual_seed(100 + 7 * Lx + B)
    x = torch.randn(B, Lx, generator=gen) * 0.3
    w = (torch.randn(64, 79, generator=gen) * 0.1).cuda()
    scale = ((torch.rand(64, generator=gen) + 0.5) * (torch.randint(0, 2, (64,), generator=gen) * 2 - 1)).cuda()
    shift = (torch.randn(64, generator=gen) * 0.3).cuda()
    xg, xbuf = guarded_x(x)
    L1 = lib.sed_m5_conv1_len(Lx)
    assert L1 == conv_len(Lx) and L1 >= 4
    N, Ho = B // 8, L1 // 4
    reg, regy = z_regions(Lx, L1), z_regions(Lx, L1, pooled=True)
    # float64 references on the operands as read: fp32 (VALU) and bf16-rounded (MFMA)
    ref, S = {}, {}
    for form, (xr, wr) in {"valu": (xg.double(), w.double()), "mfma": (rbf(xg), rbf(w))}.items():
        Pm = patches(xr, L1)
        ref[form], S[form] = to_eng(Pm @ wr.t()), to_eng(Pm.abs() @ wr.abs().t())
    env, G = Env(L, monkeypatch), Guards()
    try:
        for blocks in BLOCKS:
            env.set(SED_M5_BLOCKS=blocks, SED_M5_MFMA=None)
            npt, tpb = nparts_and_tpb(lib, B, Lx, blocks)
            cs = SAFE * (4 * tpb + 32) * U

            def stats_check(kernel, part, v):
                tot = sum_rows(part, kernel)
                v = v.double()
                gate_check(kernel, "sum z", tot[0], v.sum((0, 1, 2)), cs * v.abs().sum((0, 1, 2)))
                gate_check(kernel, "sum z^2", tot[1], (v * v).sum((0, 1, 2)), (cs + SAFE * U) * (v * v).sum((0, 1, 2)))

            # fp32 VALU
            z32, p32 = G.new((N, L1, 8, 64)), G.new((npt, 2, 64))
            L.check(lib.sed_m5_conv1_fwd(F32, P(xg), P(w), P(z32), P(p32), B, Lx, st), "sed_m5_conv1_fwd f32")
            G.intact()
            g32 = SAFE * 79 * U * S["valu"]
            gate_check("conv1_fwd f32", "z", z32, ref["valu"], g32, reg)
            stats_check("conv1_fwd f32", p32, z32)
            # bf16 store, VALU form (fp32 operands): its statistics are those of the fp32 accumulators
            env.set(SED_M5_MFMA="0")
            zv, pv = G.new((N, L1, 8, 64), torch.bfloat16), G.new((npt, 2, 64))
            L.check(lib.sed_m5_conv1_fwd(BF16, P(xg), P(w), P(zv), P(pv), B, Lx, st), "sed_m5_conv1_fwd bf16 valu")
            G.intact()
            env.set(SED_M5_MFMA=None)
            gate_check("conv1_fwd bf16 valu", "z", zv, ref["valu"], g32 + bf16_half_ulp(ref["valu"].abs() + g32), reg)
            same_bits(zv, z32.bfloat16(), "VALU bf16 z against the rounding of the fp32 launch's accumulators")
            stats_check("conv1_fwd bf16 valu", pv, z32)
            # bf16 MFMA (the default form): statistics of the values as stored
            zm, pm = G.new((N, L1, 8, 64), torch.bfloat16), G.new((npt, 2, 64))
            L.check(lib.sed_m5_conv1_fwd(BF16, P(xg), P(w), P(zm), P(pm), B, Lx, st), "sed_m5_conv1_fwd bf16")
            G.intact()
            gm = SAFE * 80 * U * S["mfma"]
            gzm = gm + bf16_half_ulp(ref["mfma"].abs() + gm)
            gate_check("conv1_fwd bf16 mfma", "z", zm, ref["mfma"], gzm, reg)
            stats_check("conv1_fwd bf16 mfma", pm, zm)
            # the statistics-only launch: the same bits as the forward's stats_partial
            ps = G.new((npt, 2, 64))
            L.check(lib.sed_m5_conv1_stats(BF16, P(xg), P(w), P(ps), B, Lx, st), "sed_m5_conv1_stats")
            G.intact()
            sum_rows(ps, "conv1_stats")
            same_bits(ps, pm, "sed_m5_conv1_stats against sed_m5_conv1_fwd's stats_partial")
            # conv + BN + ReLU + MaxPool in one launch, with and without z_out
            ya, za, yb = G.new((N, Ho, 8, 64), torch.bfloat16), G.new((N, L1, 8, 64), torch.bfloat16), G.new((N, Ho, 8, 64), torch.bfloat16)
            L.check(lib.sed_m5_conv1_bn_relu_pool_fwd(BF16, P(xg), P(w), P(scale), P(shift), P(ya), P(za), B, Lx, st), "pool_fwd z_out")
            L.check(lib.sed_m5_conv1_bn_relu_pool_fwd(BF16, P(xg), P(w), P(scale), P(shift), P(yb), None, B, Lx, st), "pool_fwd")
            yk = G.new((N, Ho, 8, 64), torch.bfloat16)
            L.check(lib.sed_bn_relu_maxpool4_fwd(BF16, P(zm), P(scale), P(shift), P(yk), N, L1, 8, 64, st), "sed_bn_relu_maxpool4_fwd")
            G.intact()
            same_bits(za, zm, "z_out against sed_m5_conv1_fwd's z")
            same_bits(ya, yb, "y with and without z_out")
            same_bits(ya, yk, "y against sed_bn_relu_maxpool4_fwd of the stored z")
            sc, sh = scale.double(), shift.double()
            pre = ref["mfma"] * sc + sh
            yref = pre[:, :4 * Ho].reshape(N, Ho, 4, 8, 64).clamp_min(0).amax(2)
            gpre = sc.abs() * gzm + SAFE * U * ((ref["mfma"].abs() + gzm) * sc.abs() + sh.abs())
            gy = gpre[:, :4 * Ho].reshape(N, Ho, 4, 8, 64).amax(2)
            gate_check("conv1_bn_relu_pool_fwd", "y", ya, yref, gy + bf16_half_ulp(yref + gy), regy)
    finally:
        env.restore()
    assert not bool(torch.isnan(xbuf[XPAD:-XPAD]).any()) and bool(torch.isnan(xbuf[:XPAD]).all()) and bool(torch.isnan(xbuf[-XPAD:]).all())


# ---- inputs of the pooled weight gradient ------------------------------------------------------------------------------------------
def exact_case(B, Lx, gen):
    """x, w, scale, shift for which z = conv1(x, w) and every pre-activation scale*z + shift are exact in fp32 and z in bf16: ties and
    non-positive windows are genuine.  Returns CPU tensors (x [B][L], w [64][79], z [B][L1][64] float64, scale, shift)."""
    L1 = conv_len(Lx)
    x = torch.randint(-8, 9, (B, Lx), generator=gen).float()
    pos = torch.rand(64, 77, generator=gen).argsort(1)[:, :6] + 1            # six distinct taps of 1..77 per channel ...
    pos[0, 0] = 0; pos[1, 0] = 78; pos[2, 0] = 0; pos[2, 1] = 78; pos[3::8, 0] = 0; pos[5::8, 0] = 78     # ... and the end taps
    w = torch.zeros(64, 79)
    w.scatter_(1, pos, (torch.randint(0, 2, (64, 6), generator=gen) * 2 - 1).float())
    assert int((w != 0).sum()) == 6 * 64
    scale = torch.exp2(torch.randint(-2, 2, (64,), generator=gen).float()) * (torch.randint(0, 2, (64,), generator=gen) * 2 - 1)
    shift = (torch.randint(-6, 6, (64,), generator=gen).float() + 0.5) / 8
    z = patches(x.double(), L1) @ w.double().t()
    assert float(z.abs().max()) <= 48 and torch.equal(rbf(z), z), "z is not exact in bf16"
    pre = z * scale.double() + shift.double()
    assert torch.equal(pre.float().double(), pre) and float(pre.abs().min()) > 0, "a pre-activation is not exact in fp32"
    return x, w, z, scale, shift


def pool_case(B, L1, gen):
    """z (bf16-exact), scale, shift such that inside every pooling window the four pre-activations scale*z + shift are pairwise at
    least |scale|/8 apart and none is closer to zero than |scale|/16 (the construction of tests/test_gpu_m5_input_grad.py): the
    arg-max / ReLU decisions cannot depend on fp32 against float64 rounding.  z in engine layout [B/8][L1][8][64]."""
    N, Ho = B // 8, L1 // 4
    scale = (torch.rand(64, generator=gen) + 0.5) * (torch.randint(0, 2, (64,), generator=gen) * 2 - 1).float()
    shift = scale * (torch.randint(-6, 6, (64,), generator=gen).float() + 0.5) / 8
    z = torch.randint(-24, 25, (N, L1, 8, 64), generator=gen).float() / 8
    base = torch.randint(-20, 9, (N, Ho, 1, 8, 64), generator=gen)
    perm = torch.rand(N, Ho, 4, 8, 64, generator=gen).argsort(dim=2)
    k = base + 3 * perm + torch.randint(0, 3, (N, Ho, 4, 8, 64), generator=gen)
    z[:, :4 * Ho] = (k.float() / 8).reshape(N, 4 * Ho, 8, 64)
    assert torch.equal(z.bfloat16().float(), z)
    pre = z.double() * scale.double() + shift.double()
    win = pre[:, :4 * Ho].reshape(N, Ho, 4, 8, 64)
    margin = 1e-3                                                       # the fp32 fma error here is < 4 * 2^-24
    assert float(pre.abs().min()) > margin, "a pre-activation within rounding of zero"
    srt = win.sort(dim=2).values
    assert float((srt[:, :, 1:] - srt[:, :, :-1]).min()) > margin, "two pre-activations of a pooling window tie"
    return z, scale, shift


def run_pooled_family(L, env, tag, Lx, B, x, z_eng, scale, shift, gen, exact):
    """sed_m5_conv1_wgrad_fused_pool, which rebuilds g (and dz) from the pooled gradient, at every grid.  z_eng: the stored z
    (bf16-exact, engine layout, CPU).  exact: the inputs of exact_case, which hold genuine ties and non-positive windows."""
    lib, P, st = L.lib(), L.ptr, _stream()
    L1 = conv_len(Lx)
    N, Ho = B // 8, L1 // 4
    dy = torch.randn(N, Ho, 8, 64, generator=gen).bfloat16().cuda()
    ca = (torch.rand(64, generator=gen) + 0.5).cuda()
    cb, cc = (torch.randn(64, generator=gen) * 0.1).cuda(), (torch.randn(64, generator=gen) * 0.1).cuda()
    torch.randn(64, generator=gen), torch.rand(64, generator=gen)      # (two draws the removed statistics checks took: dy .. cc keep their values)
    xg, xbuf = guarded_x(x)
    zb = z_eng.bfloat16().cuda()
    scale, shift = scale.cuda(), shift.cuda()
    z64 = zb.double()
    g64, ties, nonpos = first_argmax_g(z64 * scale.double() + shift.double(), dy.double())
    if exact:
        assert ties >= 4 and nonpos >= 4, (ties, nonpos)           # the data really hold tied maxima and windows without a positive one
    else:
        assert ties == 0
    Pm = patches(rbf(xg), L1)                                       # the matrix-pipe kernels round x to bf16
    Pa = Pm.abs()
    gb, zf = from_eng(g64), from_eng(z64)
    terms = (ca.double() * gb, cb.double() * zf, cc.double().expand_as(zf))
    dz64, dabs = terms[0] + terms[1] + terms[2], terms[0].abs() + terms[1].abs() + terms[2].abs()
    dw_ref, dw_S = torch.einsum("btk,btc->kc", Pm, dz64), torch.einsum("btk,btc->kc", Pa, dabs)
    dw_H = torch.einsum("btk,btc->kc", Pa, bf16_half_ulp(dz64.abs() + 2 * U * dabs))       # the one bf16 rounding of dz
    regw = dw_regions(Lx, L1)
    G = Guards()
    for blocks in BLOCKS:
        env.set(SED_M5_BLOCKS=blocks)
        npt, tpb = nparts_and_tpb(lib, B, Lx, blocks)
        g_dw = dw_H + SAFE * (32 * tpb + 5) * U * dw_S

        def dw_of(part, what):
            assert part.shape == (npt, 80, 64)
            return sum_rows(part, what)[:79]                        # tap row 79 is written (no NaN) and never read as dW

        ws = G.new((npt, 80, 64))
        L.check(lib.sed_m5_conv1_wgrad_fused_pool(BF16, P(xg), P(dy), P(zb), P(scale), P(shift), P(ca), P(cb), P(cc), P(ws), B, Lx, st),
                "sed_m5_conv1_wgrad_fused_pool")
        G.intact()
        gate_check("conv1_wgrad_fused_pool", tag, dw_of(ws, "wgrad_fused_pool"), dw_ref, g_dw, regw)
    assert bool(torch.isnan(xbuf[:XPAD]).all()) and bool(torch.isnan(xbuf[-XPAD:]).all())


# ---- 2. the pooled weight gradient deciding on exact data: genuine ties and non-positive windows -------------------------------------
@pytest.mark.parametrize("B", [8, 16])
@pytest.mark.parametrize("Lx", LENGTHS)
def test_conv1_decisions_on_exact_z(L, monkeypatch, Lx, B):
    gen = torch.Generator().manual_seed(200 + 7 * Lx + B)
    x, _, z, scale, shift = exact_case(B, Lx, gen)
    env = Env(L, monkeypatch)
    try:
        run_pooled_family(L, env, "exact", Lx, B, x, to_eng(z), scale, shift, gen, exact=True)
    finally:
        env.restore()


# ---- 3. weight-gradient family -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [8, 16])
@pytest.mark.parametrize("Lx", LENGTHS)
def test_conv1_weight_gradients(L, monkeypatch, Lx, B):
    lib, P, st = L.lib(), L.ptr, _stream()
    gen = torch.Generator().manual_seed(300 + 7 * Lx + B)
    L1 = conv_len(Lx)
    N = B // 8
    x = torch.randn(B, Lx, generator=gen) * 0.3
    xg, xbuf = guarded_x(x)
    dz = torch.randn(N, L1, 8, 64, generator=gen).cuda()
    gg, zz = torch.randn(N, L1, 8, 64, generator=gen).bfloat16().cuda(), torch.randn(N, L1, 8, 64, generator=gen).bfloat16().cuda()
    ca = (torch.rand(64, generator=gen) + 0.5).cuda()
    cb, cc = (torch.randn(64, generator=gen) * 0.2).cuda(), (torch.randn(64, generator=gen) * 0.1).cuda()
    regw = dw_regions(Lx, L1)
    P32, Pbf = patches(xg.double(), L1), patches(rbf(xg), L1)
    refs = {}
    for dt in (F32, BF16):                                           # the VALU kernel: fp32 x, dz in the mode's type
        d = from_eng(dz.to(DT[dt]).double())
        refs[dt] = torch.einsum("btk,btc->kc", P32, d), torch.einsum("btk,btc->kc", P32.abs(), d.abs())
    terms = (ca.double() * from_eng(gg.double()), cb.double() * from_eng(zz.double()), cc.double().expand(B, L1, 64))
    fz_ref = torch.einsum("btk,btc->kc", Pbf, terms[0] + terms[1] + terms[2])
    fz_abs = terms[0].abs() + terms[1].abs() + terms[2].abs()
    fz_S = torch.einsum("btk,btc->kc", Pbf.abs(), fz_abs)
    fz_H = torch.einsum("btk,btc->kc", Pbf.abs(), bf16_half_ulp((terms[0] + terms[1] + terms[2]).abs() + 2 * U * fz_abs))
    env, G = Env(L, monkeypatch), Guards()
    try:
        for blocks in BLOCKS:
            env.set(SED_M5_BLOCKS=blocks)
            npt, tpb = nparts_and_tpb(lib, B, Lx, blocks)
            for dt in (F32, BF16):
                ws, dzt = G.new((npt, 80, 64)), dz.to(DT[dt])
                L.check(lib.sed_m5_conv1_wgrad(dt, P(xg), P(dzt), P(ws), B, Lx, st), "sed_m5_conv1_wgrad")
                G.intact()
                gate_check(f"conv1_wgrad {NAME[dt]}", "dW", sum_rows(ws, "wgrad")[:79], refs[dt][0], SAFE * 128 * tpb * U * refs[dt][1], regw)
            ws = G.new((npt, 80, 64))
            L.check(lib.sed_m5_conv1_wgrad_fused(BF16, P(xg), P(gg), P(zz), P(ca), P(cb), P(cc), P(ws), B, Lx, st), "sed_m5_conv1_wgrad_fused")
            G.intact()
            gate_check("conv1_wgrad_fused", "dW", sum_rows(ws, "wgrad_fused")[:79], fz_ref, fz_H + SAFE * (32 * tpb + 5) * U * fz_S, regw)
        assert bool(torch.isnan(xbuf[:XPAD]).all()) and bool(torch.isnan(xbuf[-XPAD:]).all())
        # the stored-z pooled forms on separated pre-activations (no decision within rounding of a tie or of zero)
        z, scale, shift = pool_case(B, L1, gen)
        run_pooled_family(L, env, "separated", Lx, B, x, z, scale, shift, gen, exact=False)
    finally:
        env.restore()


# ---- 4. MaxPool1d(4) kernels on a given z ----------------------------------------------------------------------------------------
def maxpool_case(N, H, Cp, gen):
    """exact data: z = k/8, scale = +-2^k, shift = (j + 1/2)/8 on even channels and j/8 on odd ones (a pre-activation of exactly 0 can
    occur there); one planted window with a tied positive maximum and one whose maximum pre-activation is exactly 0."""
    z = torch.randint(-24, 25, (N, H, 8, Cp), generator=gen).float() / 8
    scale = torch.exp2(torch.randint(-1, 2, (Cp,), generator=gen).float()) * (torch.randint(0, 2, (Cp,), generator=gen) * 2 - 1)
    j = torch.randint(-6, 6, (Cp,), generator=gen).float()
    shift = torch.where(torch.arange(Cp) % 2 == 0, (j + 0.5) / 8, j / 8)
    z[0, 0:4, 0, 0] = (torch.tensor([1.0, 2.0, 2.0, 0.0]) - shift[0] + 0.0625) / scale[0]       # pre = 1, 2, 2, 0 (+ 1/16): tie
    z[0, 0:4, 0, 1] = (torch.tensor([-1.0, 0.0, -2.0, 0.0]) - shift[1]) / scale[1]              # pre = -1, 0, -2, 0: maximum exactly 0
    assert torch.equal(z.bfloat16().float(), z)
    pre = z.double() * scale.double() + shift.double()
    assert torch.equal(pre.float().double(), pre)
    assert float(pre[0, 0:4, 0, 1].max()) == 0.0 and float(pre[0, 1, 0, 0]) == float(pre[0, 2, 0, 0]) > 0
    return z, scale, shift


@pytest.mark.parametrize("Cp", [8, 24, 64, 128, 256, 512])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_maxpool4_kernels(L, dt, Cp):
    lib, P, st = L.lib(), L.ptr, _stream()
    tdt, Gd = DT[dt], Guards()
    for N in (1, 3):
        for H in (4, 5, 7, 8, 9, 130):
            gen = torch.Generator().manual_seed(500 + 1000 * N + 10 * H + Cp)
            Ho, W = H // 4, 8
            z, scale, shift = maxpool_case(N, H, Cp, gen)
            dy = torch.randn(N, Ho, W, Cp, generator=gen).to(tdt).cuda()
            mean, invstd = (torch.randn(Cp, generator=gen) * 0.3).cuda(), (torch.rand(Cp, generator=gen) + 0.5).cuda()
            zt, scale, shift = z.to(tdt).cuda(), scale.cuda(), shift.cuda()
            pre = zt.double() * scale.double() + shift.double()
            # forward, also on free-form (inexact) data: one fma of the exact value
            for tag, zin, sc, sh in (("exact", zt, scale, shift),
                                     ("random", torch.randn(N, H, W, Cp, generator=gen).to(tdt).cuda(),
                                      (torch.randn(Cp, generator=gen)).cuda(), (torch.randn(Cp, generator=gen) * 0.3).cuda())):
                y = Gd.new((N, Ho, W, Cp), tdt)
                L.check(lib.sed_bn_relu_maxpool4_fwd(dt, P(zin), P(sc), P(sh), P(y), N, H, W, Cp, st), "sed_bn_relu_maxpool4_fwd")
                Gd.intact()
                pr = zin.double() * sc.double() + sh.double()
                yref = pr[:, :4 * Ho].reshape(N, Ho, 4, W, Cp).clamp_min(0).amax(2)
                gy = SAFE * U * ((zin.double() * sc.double()).abs() + sh.double().abs())[:, :4 * Ho].reshape(N, Ho, 4, W, Cp).amax(2)
                gate_check(f"bn_relu_maxpool4_fwd {NAME[dt]}", tag, y, yref, gy + bf16_half_ulp(yref + gy) if dt == BF16 else gy)
            if 256 % (Cp // 8) != 0 or Cp < 64:
                continue
            g_ref, ties, nonpos = first_argmax_g(pre, dy.double())
            assert ties >= 1 and nonpos >= 1
            xhat = (zt.double() - mean.double()) * invstd.double()
            st_ref = torch.stack([g_ref.sum((0, 1, 2)), (g_ref * xhat).sum((0, 1, 2))])
            st_S = torch.stack([g_ref.abs().sum((0, 1, 2)), (g_ref * xhat).abs().sum((0, 1, 2))])
            npp = lib.sed_maxpool4_bwd_nparts(N, H, W, Cp)
            Gc = Cp // 8
            n_acc = 4 * cdiv(N * (Ho + 1) * W * Gc, npp * 256) + 256 // Gc
            c_st = torch.tensor([SAFE * n_acc * U, SAFE * (n_acc + 3) * U], device="cuda", dtype=torch.float64).view(2, 1)
            g, pa, pb = Gd.new((N, H, W, Cp), tdt), Gd.new((npp, 2, Cp)), Gd.new((npp, 2, Cp))
            L.check(lib.sed_maxpool4_relu_bwd(dt, P(dy), P(zt), P(scale), P(shift), P(mean), P(invstd), P(g), P(pa), N, H, W, Cp, st), "relu_bwd")
            L.check(lib.sed_maxpool4_relu_bwd(dt, P(dy), P(zt), P(scale), P(shift), P(mean), P(invstd), None, P(pb), N, H, W, Cp, st), "relu_bwd g=NULL")
            Gd.intact()
            same_bits(g, g_ref.to(tdt), f"g (dy or +0, dropped rows +0) N={N} H={H}")
            same_bits(pa, pb, "the statistics with and without g stored")
            gate_check(f"maxpool4_relu_bwd {NAME[dt]}", "stats", sum_rows(pa, "relu_bwd"), st_ref, c_st * st_S)
            # the pooled-tensor statistics: the kernel's own formula on the y it is given, in float64
            y = pre[:, :4 * Ho].reshape(N, Ho, 4, W, Cp).clamp_min(0).amax(2).to(tdt)
            flag = torch.tensor([0, 0x5A5A5A5A, 7, 0x5A5A5A5A], dtype=torch.int32, device="cuda")     # [flag, canary, flag_clear, canary]
            pp = Gd.new((npp, 2, Cp))
            L.check(lib.sed_maxpool4_pooled_stats(dt, P(dy), P(y), P(scale), P(shift), P(mean), P(invstd), P(pp), P(flag), P(flag[2:]),
                                                  N, H, W, Cp, st), "sed_maxpool4_pooled_stats")
            Gd.intact()
            assert flag.tolist() == [0, 0x5A5A5A5A, 0, 0x5A5A5A5A]           # well-conditioned channels only; flag_clear reset
            items = N * Ho * W * Gc
            grid = min(max(cdiv(items, 256), 1), 2048, npp)
            assert bool((pp[grid:] == 0).all()), "rows past pooled_stats' own grid must be zero"
            act = (y.double() > 0) * dy.double()
            st_, rt_ = act.sum((0, 1, 2)), (act * y.double()).sum((0, 1, 2))
            beta = mean.double() * scale.double() + shift.double()
            r = invstd.double() / scale.double()
            q_ref = (rt_ - beta * st_) * r
            q_S = ((act * y.double()).abs().sum((0, 1, 2)) + beta.abs() * act.abs().sum((0, 1, 2))) * r.abs()
            n_p = cdiv(items, grid * 256) + 256 // Gc
            tot = sum_rows(pp, "pooled_stats")
            gate_check(f"maxpool4_pooled_stats {NAME[dt]}", "sum g", tot[0], st_, SAFE * n_p * U * act.abs().sum((0, 1, 2)))
            gate_check(f"maxpool4_pooled_stats {NAME[dt]}", "sum g*xhat", tot[1], q_ref, SAFE * (n_p + 6) * U * q_S)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_maxpool4_pooled_stats_flag(L, dt):
    """raised by an ill-conditioned channel (|beta| > 8 |gamma|) with an active window and by scale = 0, not by an ill channel whose
    windows are all inactive; sed_maxpool4_relu_bwd_if is a no-op while it is 0, else recomputes from z and resets it"""
    lib, P, st = L.lib(), L.ptr, _stream()
    tdt, Gd = DT[dt], Guards()
    N, H, W, Cp = 3, 9, 8, 64
    Ho = H // 4
    gen = torch.Generator().manual_seed(600 + dt)
    z, scale, shift = maxpool_case(N, H, Cp, gen)
    dy = torch.randn(N, Ho, W, Cp, generator=gen).to(tdt).cuda()
    invstd = (torch.rand(Cp, generator=gen) + 0.5).cuda()
    zt, scale, shift = z.to(tdt).cuda(), scale.cuda(), shift.cuda()
    y = (zt.double() * scale.double() + shift.double())[:, :4 * Ho].reshape(N, Ho, 4, W, Cp).clamp_min(0).amax(2).to(tdt)
    assert bool((y[..., 5] > 0).any()) and bool((y[..., 6] > 0).any())
    npp = lib.sed_maxpool4_bwd_nparts(N, H, W, Cp)

    def launch(mean, sc, yy):
        flag = torch.tensor([0, 0x5A5A5A5A], dtype=torch.int32, device="cuda")
        pp = Gd.new((npp, 2, Cp))
        L.check(lib.sed_maxpool4_pooled_stats(dt, P(dy), P(yy), P(sc), P(shift), P(mean), P(invstd), P(pp), P(flag), None, N, H, W, Cp, st),
                "sed_maxpool4_pooled_stats")
        Gd.intact()
        assert int(flag[1]) == 0x5A5A5A5A
        return flag, pp

    mean0 = torch.zeros(Cp, device="cuda")                           # beta = shift, |shift| < 1 <= 8 |scale| * ... : well conditioned
    assert bool((shift.abs() * invstd <= 8 * scale.abs()).all())
    assert int(launch(mean0, scale, y)[0][0]) == 0
    ill = mean0.clone()
    ill[5] = 1000.0                                                  # |beta| >> 8 |gamma| in channel 5
    y_off = y.clone()
    y_off[..., 5] = 0
    assert int(launch(ill, scale, y_off)[0][0]) == 0, "an ill channel without an active window raised the flag"
    sc0 = scale.clone()
    sc0[6] = 0.0
    assert int(launch(mean0, sc0, y)[0][0]) == 1, "scale = 0 with an active window did not raise the flag"
    flag, pp = launch(ill, scale, y)
    assert int(flag[0]) == 1, "an ill channel with an active window did not raise the flag"
    # the conditional z pass: a no-op on a zero flag, the statistics of sed_maxpool4_relu_bwd(g = NULL) and a reset flag otherwise
    want = Gd.new((npp, 2, Cp))
    L.check(lib.sed_maxpool4_relu_bwd(dt, P(dy), P(zt), P(scale), P(shift), P(ill), P(invstd), None, P(want), N, H, W, Cp, st), "relu_bwd")
    keep = pp.clone()
    zero = torch.zeros(2, dtype=torch.int32, device="cuda")
    L.check(lib.sed_maxpool4_relu_bwd_if(P(zero), dt, P(dy), P(zt), P(scale), P(shift), P(ill), P(invstd), P(pp), N, H, W, Cp, st), "relu_bwd_if 0")
    Gd.intact()
    same_bits(pp, keep, "sed_maxpool4_relu_bwd_if with a zero flag must not write")
    L.check(lib.sed_maxpool4_relu_bwd_if(P(flag), dt, P(dy), P(zt), P(scale), P(shift), P(ill), P(invstd), P(pp), N, H, W, Cp, st), "relu_bwd_if 1")
    torch.cuda.synchronize()
    same_bits(pp, want, "sed_maxpool4_relu_bwd_if against sed_maxpool4_relu_bwd(g = NULL)")
    assert flag.tolist() == [0, 0x5A5A5A5A], "the flag is reset after the conditional pass"


# ---- 5. head -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,Cp", [(256, 256), (40, 64), (300, 304), (512, 512)])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_head(L, dt, C, Cp):
    lib, P, st = L.lib(), L.ptr, _stream()
    tdt, Gd = DT[dt], Guards()
    for B in (8, 32, 40, 72):
        for H in (1, 3, 31):
            for K in (1, 3, 4, 5, 11):
                gen = torch.Generator().manual_seed(700 + 100 * B + 10 * H + K + C)
                feat = torch.randn(B // 8, H, 8, Cp, generator=gen).to(tdt).cuda()
                feat[..., C:] = float("nan")                          # padded channels are not read
                fcw, fcb = (torch.randn(K, C, generator=gen) * 0.1).cuda(), torch.randn(K, generator=gen).cuda()
                m, pre = Gd.new((B, C)), Gd.new((B, K))
                L.check(lib.sed_m5_head_fwd(dt, P(feat), P(fcw), P(fcb), P(m), P(pre), B, H, C, Cp, K, st), "sed_m5_head_fwd")
                Gd.intact()
                f64 = feat[..., :C].double().permute(0, 2, 1, 3).reshape(B, H, C)
                m_ref, g_m = f64.mean(1), SAFE * H * U * f64.abs().mean(1)
                gate_check(f"m5_head_fwd {NAME[dt]}", "m", m, m_ref, g_m)
                w64 = fcw.double()
                g_pre = SAFE * (cdiv(C, 64) + 7) * U * (m_ref.abs() @ w64.abs().t() + fcb.double().abs()) + g_m @ w64.abs().t()
                gate_check(f"m5_head_fwd {NAME[dt]}", "pre", pre, m_ref @ w64.t() + fcb.double(), g_pre)
                dpre, min_ = torch.randn(B, K, generator=gen).cuda(), torch.randn(B, C, generator=gen).cuda()
                dw, db, df = Gd.new((K, C)), Gd.new((K,)), Gd.new((B // 8, H, 8, Cp), tdt)
                L.check(lib.sed_m5_head_bwd(dt, P(dpre), P(min_), P(fcw), P(dw), P(db), P(df), B, H, C, Cp, K, st), "sed_m5_head_bwd")
                Gd.intact()
                d64 = dpre.double()
                gate_check(f"m5_head_bwd {NAME[dt]}", "dfc_w", dw, d64.t() @ min_.double(),
                           SAFE * (cdiv(B, 4) + 10) * U * (d64.abs().t() @ min_.double().abs()))
                gate_check(f"m5_head_bwd {NAME[dt]}", "dfc_b", db, d64.sum(0), SAFE * (cdiv(B, 4) + 3) * U * d64.abs().sum(0))
                assert not bool(torch.isnan(df).any())
                assert bool((df[..., C:] == 0).all()) and not bool(torch.signbit(df[..., C:].float()).any()), "channels [C, Cp) of dfeat must be +0"
                for h in range(1, H):
                    same_bits(df[:, h], df[:, 0], "dfeat differs between time steps")
                df_ref = (d64 @ w64) / H
                g_df = SAFE * (K + 1) * U * (d64.abs() @ w64.abs()) / H
                got = df[:, 0, :, :C].reshape(B, C)
                gate_check(f"m5_head_bwd {NAME[dt]}", "dfeat", got, df_ref, g_df + bf16_half_ulp(df_ref.abs() + g_df) if dt == BF16 else g_df)
