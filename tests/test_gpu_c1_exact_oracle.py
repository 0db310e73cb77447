"""GPU: the Cin = 1 first-layer kernels of csrc/sed_c1.hip -- the direct forward with its statistics, the plain and the fused weight
gradient, the Gram statistics of the 3x3 input patches, the BatchNorm finalizers that work from them, the backward's scalar kernels
and the composed first-layer gradient -- per element against float64, through the C ABI.  (sed_conv3x3_c1_dgrad and the eval
finalizers have their gate in tests/test_gpu_input_grad.py, the matrix-pipe C1-mode kernels in tests/test_gpu_kernels_oracle.py.)

Reference: the same operation in float64 (torch) ON THE OPERANDS THE KERNEL READS (fp32 x / mean / std / w, g and z as stored).  No
kernel of this library serves as a reference; bit identities the header promises between two entry points are asserted on top,
never instead.  Every output and workspace buffer starts as NaN between two NaN guard regions that must be intact after the launch;
x is a view into a larger NaN-filled allocation, so a read before row 0 or past the last row poisons the result.  No element is
excluded from any comparison.  Partial rows are summed here in float64 and every row must have been written.

Notation: xn = (x - mean) / std in float64 from the fp32 x, mean, std (x itself when they are NULL); xp[t], t = 3 di + dj, its
zero-padded 3x3 patch (xp[t] at pixel (h, w) = xn[h + di - 1][w + dj - 1]); N = B H W; u = 2^-24 (one fp32 rounding); SAFE = 4
multiplies every operation COUNT; a bf16 store adds the true half bf16 ulp of the value.  Nothing below was set from a measurement.
Geometry (c1_geometry, sed_conv_c1_nparts, sed_conv_c1_gram_nparts): bands = B ceil(H/8) bands of 8 rows; forward / weight gradient:
grid = min(B H, 768) workgroups, PPB = 256 / (Coutp / 8) pixel lanes, a thread's chain n_t = ceil(W / PPB) * 8 * ceil(bands / grid);
Gram: grid = min(bands, 2048), n_t = ceil(8 W / 256) * ceil(bands / grid).

  z              (sed_conv3x3_c1_fwd) a chain of 9 fmas on z-scored values that carry 2 roundings (the subtraction, the division):
                 gate = SAFE (9 + 2) u S, S = sum_t |xp[t]| |w[t]|; the bf16 store adds half a bf16 ulp of (|ref| + that gate).
                 Channels [Cout, Coutp) are +0 in z and in both partial rows.  stats_partial = NULL: the same z bits.
  z statistics   the kernel sums its fp32 ACCUMULATORS (also when it stores bf16); the reference is the float64 sum of the float64 z
                 and z^2.  z's fp32 gate g propagates as sum g, and as sum (2 |z| g + g^2) for z^2; the summation adds
                 SAFE (n_t + PPB) u sum |z| (n_t adds in the thread, PPB over the lanes) and SAFE (n_t + PPB + 1) u sum z^2 (the fma).
                 Rows of workgroups that own no band (row >= bands) are exactly 0.
  weight grads   (sed_conv3x3_c1_wgrad, _fused) dW[k][c] = sum dz xp[k]: n_t fmas, PPB adds over the lanes, the 2 roundings of the
                 z-scored operand: gate = SAFE (n_t + PPB + 2) u sum |dz| |xp[k]|.  Fused: dz = fma(ca, g, fma(cb, z, cc)) is two
                 fp32 roundings of |ca g| + |cb z| + |cc|: + 2 u sum (|ca g| + |cb z| + |cc|) |xp[k]|; g and z as stored.
  Gram           (sed_conv3x3_c1_gram) G[j][k] = sum xp[j] xp[k] (j <= k, row-major upper triangle), then sx[k] = sum xp[k].  The kernel
                 z-scores as (v - mean) * (1 / std): three roundings per operand; two operands and the fma make 7; n_t fmas in the
                 thread; six shuffle levels and three adds over the waves make 9: gate(G) = SAFE (7 + n_t + 9) u sum |xp[j]| |xp[k]|,
                 gate(sx) = SAFE (3 + n_t + 9) u sum |xp[k]|.  mean / std NULL: the operand roundings drop out, the gate is kept.
  finalize       (sed_bn_train_finalize_c1, _g) fed with the Gram kernel's own partial rows.  Reference: mean and biased variance
                 directly over the float64 z1 = conv1(xn), NOT through the Gram identity.  The kernel forms mean = w.sx / N and
                 var = w'Gw / N - mean^2 in double, so only the Gram gates propagate (with absolute values):
                   g_mean = sum |w_k| gate(sx_k) / N + u |mean|                         (the fp32 store)
                   g_var  = sum |w_j| |w_k| gate(G_jk) / N + 2 |mean| g_mean + g_mean^2
                   g_invstd = invstd g_var / (2 (var + eps - g_var)) + SAFE u invstd     (1/sqrt is convex: the exact difference is
                              g_var / ((sqrt(a) + sqrt(a - g_var)) sqrt(a) sqrt(a - g_var)), a = var + eps, which is smaller)
                   scale  = fl(gamma invstd):            |gamma| g_invstd + SAFE u |scale|
                   shift  = fl(beta - fl(mean) scale):   |mean| g_scale + |scale| g_mean + g_mean g_scale + SAFE 2 u (|beta| + |mean scale|)
                   running mean = fl(fl(1 - m) rm + m fl(mean)):     m g_mean + SAFE 3 u (|(1 - m) rm| + |m mean|)
                   running var  = the same with fl(unbiased):        m g_var N/(N-1) + SAFE 4 u (|(1 - m) rv| + m unbiased)
                 Condition (on the reference, asserted before any comparison): g_var <= (var + eps) / 4 in every tested channel.
                 gram_sum of _g equals the float64 sum of the partial rows to 2^-50 relative and satisfies the Gram gates; the two entry
                 points agree bit for bit.  Exact: a channel of zero weights has invstd = fl(1 / sqrt(eps)), mean 0, shift = beta;
                 N = 1 leaves the unbiased factor at 1; channels [C, Cp) are 0 in scale, shift, mean, invstd and untouched in the
                 running statistics.
  scalar kernels (sed_bn_bwd_finalize_c1, sed_conv3x3_c1_wgrad_combine / _u, sed_c1_bwd_tail) compute in double from fp32 operands
                 and round once; the reference evaluates the header's formulas in float64 on the same operands.  Gate: one fp32
                 rounding, u |ref|, plus 2^-45 of the magnitudes that are combined: sum |w| |A| and |mu| |sg| (scaled by the factors
                 that multiply them) for dgamma, cb, cc; |ca A| + |cb| sum |w| |G| + |cc sx| for dW (|G| = the sum of |partial rows|).
                 sed_c1_bwd_tail: a_sum is gated first (a fixed-order double sum, one rounding: u |ref| + 2^-45 sum |rows|); that
                 rounding, and then those of ca / cb / cc, are propagated through the coefficient and dW1 formulas with absolute values
                 (|xy - x'y'| <= |x| e_y + |y| e_x + e_x e_y); the kernel's own a_sum is never the reference.  dw (torch layout) equals
                 dwpack bit for bit, padded channels are 0, and the tail agrees with the three-kernel route bit for bit whenever both
                 hold the same fp32 a_sum (asserted for every such case; a_nparts = 1 always is one).  Half of the channels get a mean
                 with mean sg = (w.A) (1 + 2^-10): the ill-conditioned direction of dgamma.
  composed       Gram -> finalize -> plain weight gradient of a given g -> sed_sum_partials -> sed_bn_bwd_finalize_c1 -> combine, and
                 the same through sed_c1_bwd_tail (Coutp = 32).  Reference: the float64 dW1 of BatchNorm-1's backward over the
                 float64 z1 (dz1 = ca g + cb z1 + cc from float64 statistics).  Gate: the component gates (A: the weight-gradient
                 gate + u |A| of sed_sum_partials; G, sx, mean, invstd as above; sum g: u |sum g|, it is handed over in fp32)
                 propagated with absolute values through q = invstd (w.A - mean sg), ca, cb, cc (each + u, the fp32 store) and
                 dW1 = ca A + cb (w.G) + cc sx, i.e. |ca| gate(A) + |cb| sum |w_j| gate(G_jk) + |cc| gate(sx_k) + the coefficient
                 errors times |A|, |w.G|, |sx| + SAFE u (|ca A| + |cb| sum |w| |G| + |cc sx|).
  exact family   integer x in [-8, 8], mean integer, std a power of two, weights +-1: every product and partial sum is exact in fp32, so
                 G, sx, mean and sum z must equal float64 exactly (an indexing error is a whole-number difference).

Input families (each with and without mean / std): white noise with random weights; a smooth field (AR(1) along both axes, rho =
0.97) as raw features -40 + 10 field with zero-sum (difference) weights, z-scored by mean / std or, the worst-conditioned case, with
mean / std NULL; the field itself with NULL; the exact integer family.

Measured max err / gate on the MI355X (printed per check at the end of the module with -s):
  z              f32 0.098 (border pixels 0.082); bf16 0.9993 (the storage half ulp is the error and the gate)
  z statistics   sum z 0.0072, sum z^2 0.015 (either storage type: the same fp32 accumulators)
  weight grads   plain 0.015 (f32) / 0.014 (bf16); fused 0.024 (f32) / 0.014 (bf16); the eight border taps no worse than the centre
  Gram           G 0.026, sx 0.017; gram_sum the same; the exact family bit for bit
  finalize       channels with weights: mean 0.017, invstd 0.12 (white; 0.005 smooth), scale 0.12, shift 0.021,
                 running mean 0.095, running var 0.089; the zero-weight channel's invstd 0.175 (one rounding of 1 / sqrt(eps) under SAFE u)
  scalar kernels bn_bwd_finalize_c1 dgamma 0.86, dbeta 0.94, ca 0.97, cb 0.93, cc 0.95; combine dW 0.996; tail a_sum 0.992, dbeta 0.991,
                 dgamma 0.60, ca 0.88, cb 0.49, cc 0.75, dW 0.50 (one fp32 rounding is the error and the gate; the cancelling channels
                 no worse); a_sum was bit-equal to sed_sum_partials in all seven cases, and so was every output of the two routes
  composed       three kernels: white 0.0091, smooth 0.0023, field 0.0016, integer 0.0008; tail: white 0.0040, smooth 0.0005 (bf16 g
                 about the same): the gate is a sum of worst cases over absolute values, the error of the identity is far inside it
No kernel missed its gate.  Dropping one border pixel of 8640 from the float64 Gram sum moves G by 21 to 196 gates.  The module runs
in about 4 s.
"""
import functools
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
XPAD = 1024                     # NaN floats on each side of x (more than a line of SED_ANYW_MAX_W + 2)
TR = 8                          # rows per band (C1_TR)
EPS = float(torch.tensor(1e-5, dtype=torch.float32))
MOM = float(torch.tensor(0.1, dtype=torch.float32))
RATIOS = {}                     # (kernel, check) -> max err / gate

# (B, H, W, Cout, Coutp, family, z-scored): every width, height, channel pair and family of the issue, each for one reason
CASES = [
    (1, 1, 1, 32, 32, "white", False),          # count = 1 (|x| <= 1/4: var = 0 there, so the finalize condition is g_var <= eps / 4)
    (2, 7, 2, 20, 32, "white", False),
    (3, 8, 5, 64, 64, "smooth", True),
    (1, 9, 64, 40, 64, "field", False),
    (2, 23, 100, 128, 128, "smooth", False),    # last width of the 4-value staging; raw features, the worst-conditioned case
    (1, 23, 101, 32, 32, "smooth", True),       # first width of the 11-value staging
    (1, 9, 256, 20, 32, "white", True),         # SED_ANYW_MAX_W
    (2, 9, 101, 32, 32, "integer", True),
    (3, 7, 64, 32, 32, "integer", False),
    (2, 23, 64, 32, 32, "smooth", False),       # the flagship width, raw features
    (1, 8, 256, 64, 64, "smooth", False),
    (3, 1, 100, 40, 64, "white", False),
    (2, 8, 1, 128, 128, "white", True),
]
# workgroups that own more than one band; the prefetch of band + gridDim crosses an image boundary
STRIDE_FWD = [(3, 2051, 5, 32, 32, "white", True), (3, 2051, 64, 32, 32, "white", False)]        # 771 bands on 768 workgroups
STRIDE_GRAM = [(8, 2049, 5, 32, 32, "white", True), (8, 2049, 64, 32, 32, "white", False)]       # 2056 bands on 2048


def case_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-{c[3]}of{c[4]}-{c[5]}{'-zs' if c[6] else ''}"


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
            print(f"  {k[0]:26s} {k[1]:44s} {RATIOS[k]:.3e}")


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


def bf16_half_ulp(v):
    """half a bf16 ulp of |v| (float64): |v| = m * 2^e with m in [0.5, 1) -> ulp 2^(e-8)"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.exp2(e.double() - 9.0)


def gate_check(kernel, check, got, ref, gate, regions=None):
    """|got - ref| <= gate for EVERY element; records max err / gate for the named regions (boolean masks) and the full tensor"""
    got = got.double()
    assert got.shape == ref.shape, (kernel, check, got.shape, ref.shape)
    assert not bool(torch.isnan(got).any()), f"{kernel} {check}: NaN in the output (an element not written, or a poisoned read)"
    assert not bool(torch.isnan(ref).any()) and not bool(torch.isnan(gate).any() if torch.is_tensor(gate) else math.isnan(gate))
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
    it = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[a.dtype]
    assert torch.equal(a.contiguous().view(it), b.contiguous().view(it)), f"{what}: not the same bits"


def plus_zero(t, what):
    it = torch.int16 if t.dtype == torch.bfloat16 else torch.int32
    assert bool((t.contiguous().view(it) == 0).all()), f"{what}: not +0"


def sum_rows(part, what):
    """float64 sum of the partial rows; every row must have been written"""
    assert not bool(torch.isnan(part).any()), f"{what}: a partial row was not written"
    return part.double().sum(0)


# ---- inputs and float64 references ---------------------------------------------------------------------------------------------------
def ar1_field(B, H, W, gen, rho=0.97):
    """unit-variance AR(1) field along both axes"""
    f = torch.randn(B, H, W, generator=gen, dtype=torch.float64)
    s = math.sqrt(1.0 - rho * rho)
    for h in range(1, H):
        f[:, h] = rho * f[:, h - 1] + s * f[:, h]
    for w in range(1, W):
        f[:, :, w] = rho * f[:, :, w - 1] + s * f[:, :, w]
    return f


def make_inputs(case):
    """x [B][H][W], mean / std [W] or None, w [Cout][1][3][3]: fp32 on the CPU"""
    B, H, W, C, Cp, family, zs = case
    gen = torch.Generator().manual_seed(1000 * B + 37 * H + 7 * W + C + (500 if zs else 0))
    mean = std = None
    if family == "white":
        x = torch.randn(B, H, W, generator=gen)
        if B * H * W == 1:
            x = x.clamp(-0.25, 0.25)
        w = torch.randn(C, 9, generator=gen) / 3.0
        if zs:
            mean, std = 0.1 * torch.randn(W, generator=gen), 0.5 + torch.rand(W, generator=gen)
    elif family in ("smooth", "field"):
        f = ar1_field(B, H, W, gen)
        x = f.float() if family == "field" else (-40.0 + 10.0 * f).float()
        w = torch.randn(C, 9, generator=gen) / 3.0
        w = w - w.mean(1, keepdim=True)                              # zero-sum (difference) filters
        if zs:
            mean, std = -40.0 + 0.5 * torch.randn(W, generator=gen), 10.0 * (0.8 + 0.4 * torch.rand(W, generator=gen))
    elif family == "integer":
        x = torch.randint(-8, 9, (B, H, W), generator=gen).float()
        w = (torch.randint(0, 2, (C, 9), generator=gen) * 2 - 1).float()
        if zs:
            mean, std = torch.randint(-2, 3, (W,), generator=gen).float(), torch.exp2(torch.randint(-1, 2, (W,), generator=gen).float())
    else:
        raise ValueError(family)
    return x.contiguous(), mean, std, w.view(C, 1, 3, 3).contiguous()


def patches(xn):
    """xp [B][H][W][9] of xn [B][H][W] (float64), tap t = 3 di + dj <-> xn[h + di - 1][w + dj - 1], 0 outside the image"""
    B, H, W = xn.shape
    p = F.pad(xn, (1, 1, 1, 1))
    return torch.stack([p[:, di:di + H, dj:dj + W] for di in range(3) for dj in range(3)], dim=-1)


class Data:
    pass


@functools.lru_cache(maxsize=3)
def data(case):
    """device operands and the float64 patch tensor of a case, computed once and shared (never modified)"""
    B, H, W, C, Cp, family, zs = case
    x, mean, std, w = make_inputs(case)
    d = Data()
    n = x.numel()
    d.xbuf = torch.full((n + 2 * XPAD,), float("nan"), device="cuda")
    d.xbuf[XPAD:XPAD + n] = x.reshape(-1).cuda()
    d.x = d.xbuf[XPAD:XPAD + n].view(B, H, W)
    d.mean, d.std = (None, None) if mean is None else (mean.cuda(), std.cuda())
    d.w = w.cuda()
    d.w64 = d.w.double().view(C, 9)
    xn = d.x.double() if mean is None else (d.x.double() - d.mean.double()) / d.std.double()
    d.P = patches(xn)                                                # [B][H][W][9]
    d.Pm = d.P.reshape(-1, 9)
    d.N = B * H * W
    hh, ww = torch.arange(H, device="cuda").view(1, H, 1, 1), torch.arange(W, device="cuda").view(1, 1, W, 1)
    d.border = ((hh == 0) | (hh == H - 1) | (ww == 0) | (ww == W - 1)).expand(B, H, W, 1)
    return d


def x_guard_intact(d):
    assert bool(torch.isnan(d.xbuf[:XPAD]).all()) and bool(torch.isnan(d.xbuf[-XPAD:]).all())


def fwd_geometry(lib, case):
    B, H, W, C, Cp = case[:5]
    npt = lib.sed_conv_c1_nparts(B, H, W)
    assert npt == min(B * H, 768)
    bands, PPB = B * cdiv(H, TR), 256 // (Cp // 8)
    return npt, bands, PPB, cdiv(W, PPB) * TR * cdiv(bands, npt)


def gram_geometry(lib, case):
    B, H, W = case[:3]
    bands = B * cdiv(H, TR)
    ng = lib.sed_conv_c1_gram_nparts(B, H, W)
    assert ng == min(bands, 2048)
    return ng, cdiv(TR * W, 256) * cdiv(bands, ng)


IU = torch.triu_indices(9, 9)                                        # row-major upper triangle: the kernel's order of the 45 products


def gram_reference(d, n_t):
    """(G [45], sx [9]) in float64 and their gates"""
    Pa = d.Pm.abs()
    Gf, Sf = d.Pm.t() @ d.Pm, Pa.t() @ Pa
    return (Gf[IU[0], IU[1]], d.Pm.sum(0), SAFE * (7 + n_t + 9) * U * Sf[IU[0], IU[1]], SAFE * (3 + n_t + 9) * U * Pa.sum(0))


def full9(tri):
    """[45] upper triangle -> symmetric [9][9]"""
    M = torch.zeros(9, 9, dtype=tri.dtype, device=tri.device)
    M[IU[0], IU[1]] = tri
    M[IU[1], IU[0]] = tri
    return M


def run_gram(L, d, case, G):
    lib, P = L.lib(), L.ptr
    B, H, W = case[:3]
    ng, n_t = gram_geometry(lib, case)
    gp = G.new((ng, 54))
    L.check(lib.sed_conv3x3_c1_gram(P(d.x), P(d.mean), P(d.std), P(gp), B, H, W, _stream()), "sed_conv3x3_c1_gram")
    G.intact()
    return gp, ng, n_t


# ---- 1. forward and its statistics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES + STRIDE_FWD, ids=case_id)
def test_c1_forward_and_statistics(L, case, dt):
    lib, P, st = L.lib(), L.ptr, _stream()
    B, H, W, C, Cp, family, zs = case
    d, G = data(case), Guards()
    npt, bands, PPB, n_t = fwd_geometry(lib, case)
    zref, S = d.P @ d.w64.t(), d.P.abs() @ d.w64.abs().t()           # [B][H][W][C]
    g32 = SAFE * (9 + 2) * U * S
    z, part = G.new((B, H, W, Cp), DT[dt]), G.new((npt, 2, Cp))
    L.check(lib.sed_conv3x3_c1_fwd(dt, P(d.x), P(d.mean), P(d.std), P(d.w), P(z), P(part), B, H, W, C, Cp, st), "sed_conv3x3_c1_fwd")
    G.intact()
    name = f"c1_fwd {NAME[dt]}"
    gate_check(name, "z", z[..., :C], zref, g32 + bf16_half_ulp(zref.abs() + g32) if dt == BF16 else g32, {"border": d.border})
    tot = sum_rows(part, name)
    if Cp > C:
        assert not bool(torch.isnan(z.float()).any())
        plus_zero(z[..., C:], f"{name}: padded channels of z")
        plus_zero(part[:, :, C:], f"{name}: padded channels of the partial rows")
    a1, a2 = zref.abs().sum((0, 1, 2)), (zref * zref).sum((0, 1, 2))
    gate_check(name, "sum z", tot[0, :C], zref.sum((0, 1, 2)), g32.sum((0, 1, 2)) + SAFE * (n_t + PPB) * U * a1)
    gate_check(name, "sum z^2", tot[1, :C], a2, (2 * zref.abs() * g32 + g32 * g32).sum((0, 1, 2)) + SAFE * (n_t + PPB + 1) * U * a2)
    if bands < npt:
        assert bool((part[bands:] == 0).all()), f"{name}: the rows of workgroups without a band are not 0"
    if family == "integer":
        assert torch.equal(tot[0, :C], zref.sum((0, 1, 2))), f"{name}: sum z of the exact family"
        if dt == F32:
            assert torch.equal(z[..., :C].double(), zref), f"{name}: z of the exact family"
    z2 = G.new((B, H, W, Cp), DT[dt])
    L.check(lib.sed_conv3x3_c1_fwd(dt, P(d.x), P(d.mean), P(d.std), P(d.w), P(z2), None, B, H, W, C, Cp, st), "sed_conv3x3_c1_fwd (no statistics)")
    G.intact()
    same_bits(z2, z, f"{name}: z without statistics")
    x_guard_intact(d)


# ---- 2. weight gradient, plain and fused ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES + STRIDE_FWD, ids=case_id)
def test_c1_weight_gradients(L, case, dt):
    lib, P, st = L.lib(), L.ptr, _stream()
    B, H, W, C, Cp, family, zs = case
    d, G = data(case), Guards()
    npt, bands, PPB, n_t = fwd_geometry(lib, case)
    gen = torch.Generator(device="cuda").manual_seed(2000 + 7 * W + H + Cp + dt)
    g = torch.randn(B, H, W, Cp, device="cuda", generator=gen).to(DT[dt])
    zz = torch.randn(B, H, W, Cp, device="cuda", generator=gen).to(DT[dt])
    ca = torch.rand(Cp, device="cuda", generator=gen) + 0.5
    cb, cc = torch.randn(Cp, device="cuda", generator=gen) * 0.2, torch.randn(Cp, device="cuda", generator=gen) * 0.1
    Pa, c = d.Pm.abs(), SAFE * (n_t + PPB + 2) * U
    reg = {"border taps": torch.tensor([t != 4 for t in range(9)], device="cuda").view(9, 1)}
    # plain
    g64 = g.double().view(-1, Cp)
    part = G.new((npt, 9, Cp))
    L.check(lib.sed_conv3x3_c1_wgrad(dt, P(d.x), P(d.mean), P(d.std), P(g), P(part), B, H, W, Cp, st), "sed_conv3x3_c1_wgrad")
    G.intact()
    gate_check(f"c1_wgrad {NAME[dt]}", "dW", sum_rows(part, "c1_wgrad"), d.Pm.t() @ g64, c * (Pa.t() @ g64.abs()), reg)
    # fused: dz = ca g + cb z + cc, never stored
    t0, t1, t2 = ca.double() * g64, cb.double() * zz.double().view(-1, Cp), cc.double().expand(d.N, Cp)
    dz, mag = t0 + t1 + t2, t0.abs() + t1.abs() + t2.abs()
    part = G.new((npt, 9, Cp))
    L.check(lib.sed_conv3x3_c1_wgrad_fused(dt, P(d.x), P(d.mean), P(d.std), P(g), P(zz), P(ca), P(cb), P(cc), P(part), B, H, W, Cp, st),
            "sed_conv3x3_c1_wgrad_fused")
    G.intact()
    gate_check(f"c1_wgrad_fused {NAME[dt]}", "dW", sum_rows(part, "c1_wgrad_fused"), d.Pm.t() @ dz,
               c * (Pa.t() @ dz.abs()) + 2 * U * (Pa.t() @ mag), reg)
    x_guard_intact(d)


# ---- 3. Gram statistics, every entry -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + STRIDE_GRAM, ids=case_id)
def test_c1_gram_every_entry(L, case):
    d, G = data(case), Guards()
    gp, ng, n_t = run_gram(L, d, case, G)
    tot = sum_rows(gp, "c1_gram")
    G_ref, sx_ref, gG, gsx = gram_reference(d, n_t)
    diag = {"diagonal": (IU[0] == IU[1]).cuda()}
    gate_check("c1_gram", "G", tot[:45], G_ref, gG, diag)
    gate_check("c1_gram", "sx", tot[45:], sx_ref, gsx)
    if case[5] == "integer":
        assert torch.equal(tot[:45], G_ref) and torch.equal(tot[45:], sx_ref), "c1_gram: the exact family"
    x_guard_intact(d)


# ---- 4. BatchNorm-1 statistics from the Gram kernel's rows ---------------------------------------------------------------------------
def finalize_reference(d, case, w64, n_t, gamma, beta, rm0, rv0):
    """float64 statistics of z1 = conv1(xn) and the gates of every finalize output (module docstring)"""
    N = d.N
    _, _, gG, gsx = gram_reference(d, n_t)
    z1 = d.Pm @ w64.t()
    r = Data()
    r.mean = z1.mean(0)
    r.var = ((z1 - r.mean) ** 2).mean(0)
    aw = w64.abs()
    r.g_mean = aw @ gsx / N + U * r.mean.abs()
    r.g_var = torch.einsum("cj,jk,ck->c", aw, full9(gG), aw) / N + 2 * r.mean.abs() * r.g_mean + r.g_mean ** 2
    a = r.var + EPS
    assert bool((r.g_var <= a / 4).all()), f"condition g_var <= (var + eps) / 4 fails: {float((r.g_var / a).max()):.3e}"
    r.invstd = a.rsqrt()
    r.g_invstd = r.invstd * r.g_var / (2 * (a - r.g_var)) + SAFE * U * r.invstd
    ga, be = gamma.double(), beta.double()
    r.scale = ga * r.invstd
    r.g_scale = ga.abs() * r.g_invstd + SAFE * U * r.scale.abs()
    r.shift = be - r.mean * r.scale
    r.g_shift = r.mean.abs() * r.g_scale + r.scale.abs() * r.g_mean + r.g_mean * r.g_scale + SAFE * 2 * U * (be.abs() + (r.mean * r.scale).abs())
    fac = N / (N - 1.0) if N > 1 else 1.0
    r.rm = (1 - MOM) * rm0.double() + MOM * r.mean
    r.g_rm = MOM * r.g_mean + SAFE * 3 * U * (((1 - MOM) * rm0.double()).abs() + (MOM * r.mean).abs())
    r.rv = (1 - MOM) * rv0.double() + MOM * r.var * fac
    r.g_rv = MOM * r.g_var * fac + SAFE * 4 * U * (((1 - MOM) * rv0.double()).abs() + MOM * r.var * fac)
    return r


def bn_operands(C, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    gamma = (torch.rand(C, device="cuda", generator=gen) + 0.5) * (torch.randint(0, 2, (C,), device="cuda", generator=gen) * 2 - 1).float()
    beta = torch.randn(C, device="cuda", generator=gen) * 0.2
    return gamma, beta, torch.randn(C, device="cuda", generator=gen) * 0.3, torch.rand(C, device="cuda", generator=gen) + 0.5


def run_finalize(L, G, gp, ng, N, w, gamma, beta, rm0, rv0, C, Cp, with_g):
    lib, P = L.lib(), L.ptr
    o = Data()
    o.scale, o.shift, o.mean, o.invstd, o.rm, o.rv = (G.new(Cp) for _ in range(6))
    o.rm[:C], o.rv[:C] = rm0, rv0                                    # [C, Cp) stays NaN: the kernel must not touch it
    if with_g:
        o.gsum = G.new(54, torch.float64)
        L.check(lib.sed_bn_train_finalize_c1_g(P(gp), ng, float(N), P(w), P(gamma), P(beta), P(o.rm), P(o.rv), MOM, EPS, P(o.scale), P(o.shift),
                                               P(o.mean), P(o.invstd), C, Cp, P(o.gsum), _stream()), "sed_bn_train_finalize_c1_g")
    else:
        L.check(lib.sed_bn_train_finalize_c1(P(gp), ng, float(N), P(w), P(gamma), P(beta), P(o.rm), P(o.rv), MOM, EPS, P(o.scale), P(o.shift),
                                             P(o.mean), P(o.invstd), C, Cp, _stream()), "sed_bn_train_finalize_c1")
    G.intact()
    return o


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_c1_bn_finalize_from_gram(L, case):
    B, H, W, C, Cp, family, zs = case
    d, G = data(case), Guards()
    gp, ng, n_t = run_gram(L, d, case, G)
    w = d.w.clone()
    if C > 1:
        w[C - 1] = 0                                                 # a channel of zero weights: var = 0 exactly
    w64 = w.double().view(C, 9)
    gamma, beta, rm0, rv0 = bn_operands(C, 3000 + 7 * W + H + C)
    r = finalize_reference(d, case, w64, n_t, gamma, beta, rm0, rv0)
    o, og = (run_finalize(L, G, gp, ng, d.N, w, gamma, beta, rm0, rv0, C, Cp, with_g) for with_g in (False, True))
    for n_ in ("scale", "shift", "mean", "invstd", "rm", "rv"):
        a, b = getattr(o, n_), getattr(og, n_)
        assert not bool(torch.isnan(a[:C]).any())
        same_bits(a[:C], b[:C], f"finalize_c1 against _g: {n_}")
    for n_, ref, gate in (("mean", r.mean, r.g_mean), ("invstd", r.invstd, r.g_invstd), ("scale", r.scale, r.g_scale), ("shift", r.shift, r.g_shift),
                          ("running mean", r.rm, r.g_rm), ("running var", r.rv, r.g_rv)):
        got = {"running mean": og.rm, "running var": og.rv}.get(n_)
        got = getattr(og, n_) if got is None else got
        gate_check("bn_train_finalize_c1", f"{n_} {family}", got[:C], ref, gate, {"non-zero weights": (w64 != 0).any(1)})
    if Cp > C:
        for n_ in ("scale", "shift", "mean", "invstd"):
            plus_zero(getattr(og, n_)[C:], f"finalize_c1 {n_}: padded channels")
            plus_zero(getattr(o, n_)[C:], f"finalize_c1 {n_}: padded channels")
        assert bool(torch.isnan(og.rm[C:]).all()) and bool(torch.isnan(og.rv[C:]).all()), "running statistics of a padded channel written"
    # the reduced Gram statistics
    tot = sum_rows(gp, "c1_gram")
    assert bool(((og.gsum - tot).abs() <= 2.0 ** -50 * tot.abs()).all()), "gram_sum against the float64 sum of the partial rows"
    G_ref, sx_ref, gG, gsx = gram_reference(d, n_t)
    gate_check("bn_train_finalize_c1_g", "gram_sum G", og.gsum[:45], G_ref, gG)
    gate_check("bn_train_finalize_c1_g", "gram_sum sx", og.gsum[45:], sx_ref, gsx)
    # exact cases
    if C > 1:
        c = C - 1
        assert float(og.mean[c]) == 0.0 and float(og.invstd[c]) == float(torch.tensor(1.0 / math.sqrt(EPS), dtype=torch.float32))
        same_bits(og.shift[c:c + 1], beta[c:c + 1], "shift of a zero-weight channel")
        same_bits(og.scale[c:c + 1], gamma[c:c + 1] * og.invstd[c:c + 1], "scale of a zero-weight channel")
    if d.N == 1:
        assert float(r.var.abs().max()) == 0.0                       # one pixel: the unbiased factor stays 1, running var decays only
    if family == "integer":
        assert torch.equal(og.mean[:C].double(), r.mean.float().double()), "mean of the exact family"


# ---- 5. the backward's scalar kernels ------------------------------------------------------------------------------------------------
class V:
    """a float64 value with a bound on its error; products and sums propagate the bounds with absolute values"""

    def __init__(self, v, e=None):
        self.v = v.double() if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64, device="cuda")
        self.e = torch.zeros_like(self.v) if e is None else e.double().expand_as(self.v).clone()

    @staticmethod
    def of(o):
        return o if isinstance(o, V) else V(o)

    def __add__(self, o):
        o = V.of(o)
        return V(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = V.of(o)
        return V(self.v - o.v, self.e + o.e)

    def __neg__(self):
        return V(-self.v, self.e)

    def __mul__(self, o):
        o = V.of(o)
        return V(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    def mag(self):
        return self.v.abs() + self.e

    def rounded(self, extra=None):
        """one fp32 rounding of the value (+ `extra`: 2^-45 of the magnitudes combined in double)"""
        return V(self.v, self.e + U * self.mag() + (0 if extra is None else 2.0 ** -45 * extra))

    def sum0(self):
        return V(self.v.sum(0), self.e.sum(0))


def bwd_reference(sg, A, w64, gamma, mean, invstd, N):
    """header formulas of sed_bn_bwd_finalize_c1 on V operands: sg [C], A [9][C], mean / invstd [C] (V), w64 [C][9], gamma [C]"""
    wt = w64.t()                                                     # [9][C]
    sgz = (A * wt).sum0()
    m_sgz = (A.mag() * wt.abs()).sum(0)
    ga = gamma.double()
    inner = sgz - mean * sg
    m_inner = m_sgz + mean.mag() * sg.mag()
    q = invstd * inner
    m_q = invstd.mag() * m_inner
    r = {"dbeta": sg, "dgamma": q.rounded(m_q), "ca": (invstd * ga).rounded(invstd.mag() * ga.abs())}
    gi = invstd * ga
    mgx = q * (1.0 / N)
    r["cb"] = (-(gi * invstd * mgx)).rounded(gi.mag() * invstd.mag() * m_q / N)
    r["cc"] = (-(gi * (sg * (1.0 / N) - mean * invstd * mgx))).rounded(gi.mag() * (sg.mag() / N + mean.mag() * invstd.mag() * m_q / N))
    return r


def combine_reference(ca, cb, cc, A, w64, Gsum, Gabs):
    """dW[k][c] = ca A[k][c] + cb sum_j w[c][j] G[j][k] + cc sx[k] on V operands; Gsum: V [54], Gabs [54] magnitudes"""
    Gf = V(full9(Gsum.v[:45]), full9(Gsum.e[:45]))
    wG = V(Gf.v @ w64.t(), Gf.e @ w64.abs().t())                     # [9][C]
    m_wG = full9(Gabs[:45]) @ w64.abs().t()
    sx = V(Gsum.v[45:].view(9, 1), Gsum.e[45:].view(9, 1))
    t = A * ca + wG * cb + sx * cc
    return t, A.mag() * ca.mag() + m_wG * cb.mag() + Gabs[45:].view(9, 1) * cc.mag()


def cancelling_mean(w64, A, sg, C, gen):
    """fp32 mean [C]: random, and in every second channel mean sg = (w . A)(1 + 2^-10): the two terms of dgamma cancel to 2^-10"""
    mean = torch.randn(C, device="cuda", generator=gen) * 0.5
    sgz = (w64.t() * A.double()[:, :C]).sum(0)
    tight = (sgz / sg.double()[:C] * (1 + 2.0 ** -10)).float()
    mean[::2] = tight[::2]
    return mean


def scalar_operands(C, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randn(C, 1, 3, 3, device="cuda", generator=gen) * 0.4
    gamma = (torch.rand(C, device="cuda", generator=gen) + 0.5) * (torch.randint(0, 2, (C,), device="cuda", generator=gen) * 2 - 1).float()
    invstd = torch.rand(C, device="cuda", generator=gen) * 3 + 0.2
    return gen, w, gamma, invstd


GRAM_FOR_SCALARS = CASES[9]                                           # the Gram rows of a real input: raw smooth features at W = 64


def assert_dw_layouts(dw, dwp, C, Cp, what):
    same_bits(dw.view(C, 9).t().contiguous(), dwp.view(9, Cp)[:, :C].contiguous(), f"{what}: dw (torch layout) against dwpack")
    if Cp > C:
        plus_zero(dwp.view(9, Cp)[:, C:], f"{what}: padded channels of dwpack")


@pytest.mark.parametrize("nparts,C,Cp", [(1, 32, 32), (5, 20, 32), (300, 40, 64), (257, 128, 128), (2, 64, 64)])
def test_c1_bn_backward_finalize_and_combine(L, nparts, C, Cp):
    lib, P, st = L.lib(), L.ptr, _stream()
    G, d = Guards(), data(GRAM_FOR_SCALARS)
    gp, ng, _ = run_gram(L, d, GRAM_FOR_SCALARS, G)
    Gsum, Gabs = V(sum_rows(gp, "gram")), gp.double().abs().sum(0)
    N = float(d.N)
    gen, w, gamma, invstd = scalar_operands(C, 5000 + nparts + C)
    w64 = w.double().view(C, 9)
    part = torch.randn(nparts, 2, Cp, device="cuda", generator=gen)
    part[:, 1] = float("nan")                                        # row 1 is not an operand of the C1 form
    A = torch.randn(9, Cp, device="cuda", generator=gen) * 3
    sg = part[:, 0].double().sum(0)
    mean = cancelling_mean(w64, A, sg.float(), C, gen)
    o = {n_: G.new(Cp) for n_ in ("dgamma", "dbeta", "ca", "cb", "cc")}
    L.check(lib.sed_bn_bwd_finalize_c1(P(part), nparts, N, P(A), P(w), P(gamma), P(mean), P(invstd), P(o["dgamma"]), P(o["dbeta"]), P(o["ca"]),
                                       P(o["cb"]), P(o["cc"]), C, Cp, st), "sed_bn_bwd_finalize_c1")
    G.intact()
    r = bwd_reference(V(sg[:C]), V(A[:, :C]), w64, gamma, V(mean), V(invstd), N)
    r["dbeta"] = r["dbeta"].rounded(part[:, 0, :C].double().abs().sum(0))
    for n_, ref in r.items():
        gate_check("bn_bwd_finalize_c1", n_, o[n_][:C], ref.v, ref.e, {"cancelling": (torch.arange(C, device="cuda") % 2 == 0)})
    if Cp > C:
        for n_ in ("ca", "cb", "cc"):
            plus_zero(o[n_][C:], f"bn_bwd_finalize_c1 {n_}: padded channels")
    # the combine, with the kernel's fp32 coefficients as operands
    ca, cb, cc = o["ca"].clone(), o["cb"].clone(), o["cc"].clone()
    ref, m = combine_reference(V(ca[:C]), V(cb[:C]), V(cc[:C]), V(A[:, :C]), w64, Gsum, Gabs)
    ref = ref.rounded(m)
    dwp, dwp_u, dw = G.new(9 * Cp), G.new(9 * Cp), G.new((C, 1, 3, 3))
    L.check(lib.sed_conv3x3_c1_wgrad_combine(P(A), P(gp), ng, P(w), P(ca), P(cb), P(cc), P(dwp), C, Cp, st), "sed_conv3x3_c1_wgrad_combine")
    L.check(lib.sed_conv3x3_c1_wgrad_combine_u(P(A), P(gp), ng, P(w), P(ca), P(cb), P(cc), P(dwp_u), C, Cp, P(dw), st), "sed_conv3x3_c1_wgrad_combine_u")
    G.intact()
    gate_check("c1_wgrad_combine", "dW", dwp.view(9, Cp)[:, :C], ref.v, ref.e)
    same_bits(dwp, dwp_u, "combine against combine_u")
    assert_dw_layouts(dw, dwp_u, C, Cp, "combine_u")


@pytest.mark.parametrize("a_nparts,C", [(1, 32), (2, 32), (3, 20), (7, 32), (25, 17), (256, 32), (1000, 20)])
def test_c1_backward_tail(L, a_nparts, C):
    lib, P, st = L.lib(), L.ptr, _stream()
    Cp = 32
    G, d = Guards(), data(GRAM_FOR_SCALARS)
    gp, ng, _ = run_gram(L, d, GRAM_FOR_SCALARS, G)
    N = float(d.N)
    gen, w, gamma, invstd = scalar_operands(C, 6000 + a_nparts + C)
    w64 = w.double().view(C, 9)
    a_part = torch.randn(a_nparts, 10, Cp, device="cuda", generator=gen) * 2
    a64 = a_part.double().sum(0)
    mean = cancelling_mean(w64, a64[:9].float(), a64[9].float(), C, gen)
    # gram_sum as the forward hands it over: sed_bn_train_finalize_c1_g's own reduction of the rows
    f = run_finalize(L, G, gp, ng, d.N, w, gamma, gamma, gamma * 0, gamma * 0 + 1, C, Cp, True)
    tot = sum_rows(gp, "gram")
    assert bool(((f.gsum - tot).abs() <= 2.0 ** -50 * tot.abs()).all())
    gsum = f.gsum.clone()
    Gsum, Gabs = V(gsum), gp.double().abs().sum(0)
    o = {n_: G.new(Cp) for n_ in ("dgamma", "dbeta", "ca", "cb", "cc")}
    a_sum, dwp, dw = G.new((10, Cp)), G.new(9 * Cp), G.new((C, 1, 3, 3))
    L.check(lib.sed_c1_bwd_tail(P(a_part), a_nparts, P(gsum), N, P(w), P(gamma), P(mean), P(invstd), P(o["dgamma"]), P(o["dbeta"]), P(o["ca"]),
                                P(o["cb"]), P(o["cc"]), P(a_sum), P(dwp), C, Cp, P(dw), st), "sed_c1_bwd_tail")
    G.intact()
    As = V(a64).rounded(a_part.double().abs().sum(0))                # a fixed-order double sum, one rounding
    gate_check("c1_bwd_tail", "a_sum", a_sum, As.v, As.e)
    Ac = V(As.v[:9, :C], As.e[:9, :C])
    r = bwd_reference(V(As.v[9, :C], As.e[9, :C]), Ac, w64, gamma, V(mean), V(invstd), N)
    for n_, ref in r.items():
        gate_check("c1_bwd_tail", n_, o[n_][:C], ref.v, ref.e, {"cancelling": (torch.arange(C, device="cuda") % 2 == 0)})
    ref, m = combine_reference(r["ca"], r["cb"], r["cc"], Ac, w64, Gsum, Gabs)
    ref = ref.rounded(m)
    gate_check("c1_bwd_tail", "dW", dwp.view(9, Cp)[:, :C], ref.v, ref.e)
    assert_dw_layouts(dw, dwp, C, Cp, "c1_bwd_tail")
    if Cp > C:
        for n_ in ("ca", "cb", "cc"):
            plus_zero(o[n_][C:], f"c1_bwd_tail {n_}: padded channels")
    # the three-kernel route: bit for bit wherever both hold the same fp32 a_sum
    a3 = G.new((10, Cp))
    L.check(lib.sed_sum_partials(P(a_part), a_nparts, 10 * Cp, P(a3), st), "sed_sum_partials")
    o3 = {n_: G.new(Cp) for n_ in ("dgamma", "dbeta", "ca", "cb", "cc")}
    L.check(lib.sed_bn_bwd_finalize_c1(P(a3[9]), 1, N, P(a3), P(w), P(gamma), P(mean), P(invstd), P(o3["dgamma"]), P(o3["dbeta"]), P(o3["ca"]),
                                       P(o3["cb"]), P(o3["cc"]), C, Cp, st), "sed_bn_bwd_finalize_c1")
    dwp3, dw3 = G.new(9 * Cp), G.new((C, 1, 3, 3))
    L.check(lib.sed_conv3x3_c1_wgrad_combine_u(P(a3), P(gp), ng, P(w), P(o3["ca"]), P(o3["cb"]), P(o3["cc"]), P(dwp3), C, Cp, P(dw3), st),
            "sed_conv3x3_c1_wgrad_combine_u")
    G.intact()
    same = torch.equal(a3.view(torch.int32), a_sum.view(torch.int32))
    if a_nparts == 1:
        assert same, "one partial row: both routes hold the row itself"
    if same:
        for n_ in o:
            lim = Cp if n_ in ("ca", "cb", "cc") else C
            same_bits(o[n_][:lim], o3[n_][:lim], f"tail against the three kernels: {n_}")
        same_bits(dwp, dwp3, "tail against the three kernels: dwpack")
        same_bits(dw, dw3, "tail against the three kernels: dw")
    print(f"c1_bwd_tail a_nparts {a_nparts}: a_sum {'bit-equal to' if same else 'differs from'} sed_sum_partials")


# ---- 6. the composed first-layer gradient --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_c1_composed_first_layer_gradient(L, case):
    lib, P, st = L.lib(), L.ptr, _stream()
    B, H, W, C, Cp, family, zs = case
    d, G = data(case), Guards()
    N = d.N
    gp, ng, n_tg = run_gram(L, d, case, G)
    w, w64 = d.w, d.w64
    gamma, beta, rm0, rv0 = bn_operands(C, 7000 + 7 * W + H + C)
    r = finalize_reference(d, case, w64, n_tg, gamma, beta, rm0, rv0)
    f = run_finalize(L, G, gp, ng, N, w, gamma, beta, rm0, rv0, C, Cp, True)
    G_ref, sx_ref, gG, gsx = gram_reference(d, n_tg)
    Gv = V(torch.cat([G_ref, sx_ref]), torch.cat([gG, gsx]))
    Pa = d.Pm.abs()
    Gabs = torch.cat([(Pa.t() @ Pa)[IU[0], IU[1]], Pa.sum(0)])
    npt, bands, PPB, n_t = fwd_geometry(lib, case)
    z1 = d.Pm @ w64.t()                                              # [N][C]
    xhat = (z1 - r.mean) * r.invstd
    for dt in (F32, BF16):
        gen = torch.Generator(device="cuda").manual_seed(7100 + 7 * W + H + dt)
        g = (torch.randn(B, H, W, Cp, device="cuda", generator=gen) / N).to(DT[dt])
        g64 = g.double().view(-1, Cp)[:, :C]
        sg64 = g64.sum(0)
        # float64 reference: BatchNorm-1's backward over z1, then conv1's weight gradient of dz1
        dz1 = gamma.double() * r.invstd * (g64 - sg64 / N - xhat * (g64 * xhat).sum(0) / N)
        dW_ref = d.Pm.t() @ dz1                                      # [9][C]
        # the kernels
        part = G.new((npt, 9, Cp))
        L.check(lib.sed_conv3x3_c1_wgrad(dt, P(d.x), P(d.mean), P(d.std), P(g), P(part), B, H, W, Cp, st), "sed_conv3x3_c1_wgrad")
        A = G.new((9, Cp))
        L.check(lib.sed_sum_partials(P(part), npt, 9 * Cp, P(A), st), "sed_sum_partials")
        sgp = torch.zeros(1, 2, Cp, device="cuda")
        sgp[0, 0, :C] = sg64.float()
        o = {n_: G.new(Cp) for n_ in ("dgamma", "dbeta", "ca", "cb", "cc")}
        L.check(lib.sed_bn_bwd_finalize_c1(P(sgp), 1, float(N), P(A), P(w), P(gamma), P(f.mean), P(f.invstd), P(o["dgamma"]), P(o["dbeta"]),
                                           P(o["ca"]), P(o["cb"]), P(o["cc"]), C, Cp, st), "sed_bn_bwd_finalize_c1")
        dwp, dw = G.new(9 * Cp), G.new((C, 1, 3, 3))
        L.check(lib.sed_conv3x3_c1_wgrad_combine_u(P(A), P(gp), ng, P(w), P(o["ca"]), P(o["cb"]), P(o["cc"]), P(dwp), C, Cp, P(dw), st),
                "sed_conv3x3_c1_wgrad_combine_u")
        G.intact()
        # the gate: component gates propagated through the formulas
        A_ref = d.Pm.t() @ g64
        Av = V(A_ref, SAFE * (n_t + PPB + 2) * U * (Pa.t() @ g64.abs())).rounded()
        sgv = V(sg64, U * sg64.abs())
        co = bwd_reference(sgv, Av, w64, gamma, V(r.mean, r.g_mean), V(r.invstd, r.g_invstd), float(N))
        t, m = combine_reference(co["ca"], co["cb"], co["cc"], Av, w64, Gv, Gabs)
        gate = t.e + SAFE * U * m
        name = f"composed dW1 {NAME[dt]}"
        gate_check(name, f"three kernels {family}", dwp.view(9, Cp)[:, :C], dW_ref, gate)
        assert_dw_layouts(dw, dwp, C, Cp, name)
        if Cp == 32:
            a_part = G.new((npt, 10, Cp))
            a_part[:, :9] = part
            a_part[:, 9] = 0
            a_part[0, 9, :C] = sg64.float()
            o2 = {n_: G.new(Cp) for n_ in ("dgamma", "dbeta", "ca", "cb", "cc")}
            a_sum, dwp2, dw2 = G.new((10, Cp)), G.new(9 * Cp), G.new((C, 1, 3, 3))
            gsum = f.gsum.clone()
            L.check(lib.sed_c1_bwd_tail(P(a_part), npt, P(gsum), float(N), P(w), P(gamma), P(f.mean), P(f.invstd), P(o2["dgamma"]), P(o2["dbeta"]),
                                        P(o2["ca"]), P(o2["cb"]), P(o2["cc"]), P(a_sum), P(dwp2), C, Cp, P(dw2), st), "sed_c1_bwd_tail")
            G.intact()
            gate_check(name, f"tail {family}", dwp2.view(9, Cp)[:, :C], dW_ref, gate)
            assert_dw_layouts(dw2, dwp2, C, Cp, name + " tail")
    x_guard_intact(d)
