"""float64 references, operand draws, gates and mutants for the bf16 3x3 convolution family (dtype SED_BF16).

Imports neither the package nor the GPU library; every function works on CPU or device tensors.  Used by
tests/test_conv_bf16_formula_host.py (CPU: the references against torch's conv2d / autograd, the mutants against the gates) and
tests/test_gpu_conv_bf16_exact_oracle.py (the kernels against the references).

Two operand families (draw_conv / draw_c1, always drawn on the CPU generator so that the host test sees the values the GPU test uses):

  exact   small integers (x, dz, g, z, weights in {-m..m}, m <= 2; BN prologue scale in {1, 2}, shift in {-2..2}; ca, cb, cc in
          {-m..m}; pool-2 dy in multiples of 4; mean integer, invstd a power of two; block 0: fmean = 0, fstd a power of two, x1 a
          multiple of fstd, w1 in {-1, 0, 1}, sc1 in {1, 2}, sh1 integer).  Nothing is sparse.  Every product and partial sum is an
          integer (or a multiple of 1/4 / of a power of two) below 2^24 in magnitude, so a correct kernel's fp32 accumulator holds the
          float64 result whatever its summation order, tile order or strip split.  Gates: eq_f32 (the fp32 output equals the
          float64 reference converted to fp32) and eq_bf16 (the stored bf16 output equals ref.to(bfloat16): integers above 256 are not
          all representable, so this pins the store's round-to-nearest-even).  exact_ok() is the < 2^24 condition.

  random  bf16-rounded Gaussians.  Per-element gates, derived (not measured):
            fp32 results            |got - ref| <= C*S, S = the same contraction over absolute values, C = 2^-16: bf16 x bf16 products
                                    are exact in fp32; accumulation in three levels (MFMA chain, tiles of a strip, strip slabs) as in
                                    tests/test_gpu_conv_exact_oracle.py, whose constant this is.
            stored bf16 results     |got - ref| <= half_ulp(|ref| + C*S) + C*S: half a bf16 ulp of the accumulator plus the
                                    accumulator's own gate.  No absolute floor, no share of elements left out; S = 0 demands exactly 0.
                                    Half an ulp is taken from the format, 2^(floor(log2 v) - 8): bf16 has 8 significant bits, so
                                    it is 2^-9 * v only at the top of a binade and 2^-8 * v at its bottom -- a flat 2^-9 * v
                                    rejects correctly rounded stores in the lower half of every binade (the host test shows one).
            dz_out                  half_ulp(|ref| + 2^-21 * M) + 2^-21 * M, M = |ca*g| + |cb*z| + |cc|.
            operands rounded in the kernel (dz kept in LDS, activations rebuilt by a BN+ReLU prologue)
                                    the reference rounds the float64 value to bf16; an element whose float64 value lies within
                                    2^-21 * M of a bf16 rounding boundary may round the other way in fp32: it contributes
                                    |other operand| * ulp_bf16(value) to the results it enters (flip_allowance).
            ReLU gates              an element whose gate argument fma(z, es, et) lies within 2^-22 * (|z*es| + |et|) of zero may match
                                    either branch (relu_either); a condition on the operands, not a measurement; its share must stay
                                    <= EITHER_SHARE per tensor.
            summed statistics       the element gate propagated through the sum plus 2^-20 of the sum of magnitudes.
"""
import torch
import torch.nn.functional as F

BF = torch.bfloat16
F64 = torch.float64
C = 2.0 ** -16              # fp32 accumulation of exact products, relative to the contraction over absolute values
SUM_ULPS = 2.0 ** -20       # fp32 summation of a statistics row, relative to the sum of magnitudes
DZ_ULPS = 2.0 ** -21        # dz = ca*g + cb*z + cc in fp32, relative to M = |ca*g| + |cb*z| + |cc|
RELU_EPS = 2.0 ** -22       # fp32 gate argument fma(z, es, et), relative to |z*es| + |et|
EITHER_SHARE = 1e-3         # largest share of either-branch elements a random case may hold
LIMIT = 2.0 ** 24           # integers below this are exact in fp32

# ---- the shape lists (B, H, W, Cin, Cout) ------------------------------------------------------------------------------------
RAGGED = [(2, 37, 64, 32, 32), (1, 9, 64, 32, 32), (3, 50, 32, 64, 64), (2, 33, 32, 32, 64), (2, 41, 16, 128, 128),
          (2, 29, 16, 64, 128), (2, 45, 8, 128, 128)]
TILE_EDGE = [(1, 5, 16, 128, 128), (3, 16, 16, 128, 128)]                      # shorter than a tile; ends on a tile boundary
FROM_L2 = [(2, 41, 16, 96, 128), (1, 23, 32, 128, 256), (2, 19, 8, 256, 128)]  # weights-from-L2 mode of the producer/consumer kernel
BENCH_GRID = [(160, 9, 32, 64, 64), (300, 20, 16, 128, 128)]
EDGES = [(1, 1, 64, 32, 32), (2, 1, 8, 128, 128), (2, 2, 16, 64, 64), (3, 2, 32, 32, 64), (2, 13, 16, 20, 17), (2, 11, 32, 40, 100)]
CONV_SHAPES = RAGGED + TILE_EDGE + FROM_L2 + BENCH_GRID + EDGES
# the wide weight-gradient kernel: one shape per width and workgroup form ((128 x 64) / (64 x 128) channels), then many short images
WIDE = [(3, 16, 16, 128, 64), (2, 29, 16, 64, 128), (2, 33, 8, 128, 64), (1, 7, 8, 64, 128), (2, 4, 32, 128, 64), (1, 9, 32, 64, 128),
        (40, 11, 16, 128, 128), (70, 19, 8, 64, 128)]
WGRAD_SHAPES = CONV_SHAPES + [s for s in WIDE if s not in CONV_SHAPES]
ANYW_WIDTHS = [1, 5, 40, 100, 255, 256]                                         # 255 / 256: aw_wg_rows falls to one row
ANYW_SHAPES = [(2, 7, 1, 32, 64), (2, 9, 5, 64, 32), (2, 5, 40, 32, 32), (1, 4, 100, 32, 64), (1, 3, 255, 32, 32), (1, 3, 256, 32, 32)]
COL_SHAPES = [(2, 45, 8, 64, 64), (3, 33, 8, 64, 128), (1, 30, 8, 256, 256)]    # sed_conv3x3_fwd_col: W = 8, zero side columns
POOLSTATS_SHAPES = [(2, 37, 32, 64, 32), (3, 50, 16, 128, 64), (2, 45, 8, 128, 128), (1, 9, 16, 64, 64), (1, 1, 16, 64, 64)]   # B, H, W, Cd, C
FUSED_CASES = [(1, 1, None), (1, 3, None), (1, 4, None), (2, 8, None), (5, 7, 1), (3, 50, 2), (192, 13, None)]   # B, H, workgroups
GEOM_C1 = [(32, 32, 64)]                                                        # W, Cin, Cout
GEOM_C2 = [(32, 64, 64, 2)]                                                     # W, C, C, pool
BLOCK0 = [(1, 1), (1, 6), (2, 37), (3, 41), (2, 64)]                            # B, H at W = 64, 1 -> 32 -> 32 channels


def pad32(c):
    return -(-c // 32) * 32


# ---- bf16 in float64 ---------------------------------------------------------------------------------------------------------
def rne(t):
    """round to nearest-even bf16 (through fp32: exact for every value used here), back in float64"""
    return t.to(torch.float32).to(BF).to(F64)


def rtz(t):
    """bf16 by truncation (round toward zero): the rounding mutant"""
    i = t.to(torch.float32).contiguous().view(torch.int32) & -65536
    return i.view(torch.float32).to(F64)


def ulp_bf16(t):
    """spacing of bf16 at |t| (normal range)"""
    e = torch.frexp(t.abs().clamp_min(2.0 ** -120)).exponent              # |t| = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(t), e - 8)


def boundary_distance(t):
    """distance of t to the nearest bf16 rounding boundary (the midpoint of the two bf16 neighbours of t)"""
    a = t.abs()
    u = ulp_bf16(a)
    lo = torch.floor(a / u) * u
    return (a - (lo + 0.5 * u)).abs()


def flip_mask(t, margin):
    """elements whose fp32 evaluation (within `margin` of the float64 value t) may round to the other bf16 neighbour"""
    return boundary_distance(t) <= margin


# ---- float64 references (NHWC) -----------------------------------------------------------------------------------------------
def conv_ref(a, w):
    """a [B][H][W][Ci], w [Co][Ci][3][3] -> [B][H][W][Co]: 3x3 convolution, stride 1, zero padding 1 (nine shifted GEMMs)"""
    B, H, W, _ = a.shape
    ap = F.pad(a, (0, 0, 1, 1, 1, 1))
    z = None
    for i in range(3):
        for j in range(3):
            t = ap[:, i:i + H, j:j + W, :] @ w[:, :, i, j].t()
            z = t if z is None else z + t
    return z


def dgrad_w(w):
    """the data gradient as a forward convolution: W'[c][o][i][j] = W[o][c][2-i][2-j]"""
    return w.permute(1, 0, 2, 3).flip(2, 3).contiguous()


def wgrad_ref(a, dz):
    """dw [Co][Ci][3][3] = sum over pixels of a[b][h+i-1][w+j-1][ci] * dz[b][h][w][co]"""
    B, H, W, Ci = a.shape
    ap = F.pad(a, (0, 0, 1, 1, 1, 1))
    d2 = dz.reshape(-1, dz.shape[-1])
    dw = torch.empty(dz.shape[-1], Ci, 3, 3, dtype=a.dtype, device=a.device)
    for i in range(3):
        for j in range(3):
            dw[:, :, i, j] = (ap[:, i:i + H, j:j + W, :].reshape(-1, Ci).t() @ d2).t()
    return dw


def bn_relu(x, sc, sh):
    """the BN+ReLU prologue relu(scale*x + shift), unrounded"""
    return torch.relu(x.to(F64) * sc.to(F64) + sh.to(F64))


def gate_arg(z, es, et):
    """(the ReLU gate argument z*es + et, its fp32 error scale |z*es| + |et|)"""
    t = z.to(F64) * es.to(F64)
    return t + et.to(F64), t.abs() + et.to(F64).abs()


def relu_either(z, es, et):
    """elements whose fp32 gate decision fma(z, es, et) > 0 is not determined by the float64 value"""
    v, m = gate_arg(z, es, et)
    return v.abs() <= RELU_EPS * m


def upsample_pool(gsrc, pool, H, W):
    """avg-pool backward: up(gsrc) / pool^2; rows / columns dropped by the pooling floor get 0"""
    g = gsrc.to(F64)
    if pool == 1:
        return g
    out = torch.zeros(g.shape[0], H, W, g.shape[-1], dtype=F64, device=g.device)
    up = g.repeat_interleave(pool, 1).repeat_interleave(pool, 2) / float(pool * pool)
    out[:, :up.shape[1], :up.shape[2]] = up
    return out


def dz_ref(gsrc, z, ca, cb, cc, pool=1, sc=None, sh=None):
    """(dz, M): dz = ca*g + cb*z + cc with g = gsrc (BN backward, sc None) or up(gsrc)/pool^2 * [sc*z + sh > 0] (BN / ReLU / avg-pool
    backward); M = |ca*g| + |cb*z| + |cc|, the scale of the fp32 evaluation's error"""
    z = z.to(F64)
    g = upsample_pool(gsrc, pool, z.shape[1], z.shape[2])
    if sc is not None:
        g = g * (gate_arg(z, sc, sh)[0] > 0)
    ca, cb, cc = ca.to(F64), cb.to(F64), cc.to(F64)
    return ca * g + cb * z + cc, (ca * g).abs() + (cb * z).abs() + cc.abs().expand_as(z)


def avgpool_fwd(a, pool=2):
    """floor avg-pool of an NHWC tensor"""
    B, H, W, Cc = a.shape
    h, w = H // pool, W // pool
    return a[:, :h * pool, :w * pool].reshape(B, h, pool, w, pool, Cc).mean(dim=(2, 4))


def c1_activation(x1, fmean, fstd, w1, sc1, sh1):
    """relu(bn1(conv1(x))) as the C1-mode kernels rebuild it (csrc/conv_common.h: c1mma_init / c1mma_block): z-score in fp32, operands
    bf16(scale*w1) and bf16(xz), shift as bf16 hi + lo, one fp32 MFMA chain.  Returns float64 NHWC (a1 rounded to bf16, the
    pre-activation, S = the same contraction over absolute values, the bf16 z-score xz [B][H][W])"""
    xz = rne((x1 - fmean) * (1.0 / fstd))                                  # fp32 arithmetic as in the loader waves
    wf = rne(w1 * sc1[:, None, None, None])                                # [32][1][3][3]
    hi = rne(sh1)
    lo = rne(sh1.to(F64) - hi)
    pre = conv_ref(xz[..., None], wf) + hi + lo
    S = conv_ref(xz[..., None].abs(), wf.abs()) + hi.abs() + lo.abs()
    return rne(torch.relu(pre)), pre, S, xz


def c1_a_rows(g, xz):
    """rows 0..8 = A[tap][c] = sum_px g[px][c] * xz[px + tap], row 9 = sum_px g[px][c]; g [B][H][W][C], xz [B][H][W] (float64)"""
    B, H, W, Cc = g.shape
    xp = F.pad(xz, (1, 1, 1, 1))
    rows = [(g * xp[:, i:i + H, j:j + W, None]).sum(dim=(0, 1, 2)) for i in range(3) for j in range(3)]
    return torch.stack(rows + [g.sum(dim=(0, 1, 2))])


def to_pack_layout(dw, Cinp, Coutp):
    """dw [Co][Ci][3][3] -> dwpack [9][Cinp][Coutp], zero padded"""
    Co, Ci = dw.shape[:2]
    out = torch.zeros(9, Cinp, Coutp, dtype=dw.dtype, device=dw.device)
    out[:, :Ci, :Co] = dw.permute(2, 3, 1, 0).reshape(9, Ci, Co)
    return out


# ---- gates: each returns a bool tensor, True where the element passes -------------------------------------------------------------
def eq_f32(got, ref):
    """exact family, fp32 output: equal to the float64 reference converted to fp32"""
    return got.to(torch.float32) == ref.to(torch.float32)


def eq_bf16(got, ref):
    """exact family, stored bf16 output: equal to ref.to(bfloat16) (round-to-nearest-even)"""
    return got.to(F64) == rne(ref)


def exact_ok(*bounds):
    """the exact family's condition: every given bound on a sum of magnitudes stays below 2^24"""
    return all(float(b) < LIMIT for b in bounds)


def bound_f32(S, allow=None):
    b = C * S
    return b if allow is None else b + allow


def half_ulp(v):
    """half a bf16 ulp at magnitude v: 2^(floor(log2 v) - 8), i.e. between 2^-9 * v (top of a binade) and 2^-8 * v (its bottom)"""
    return 0.5 * ulp_bf16(v)


def bound_bf16(ref, S, allow=None):
    acc = bound_f32(S, allow)
    return half_ulp(ref.abs() + acc) + acc


def bound_dz(ref, M):
    return half_ulp(ref.abs() + DZ_ULPS * M) + DZ_ULPS * M


def within(got, ref, bound):
    """|got - ref| <= bound per element (NaN fails; a zero bound demands equality)"""
    return (got.to(F64) - ref).abs() <= bound


def within_either(got, ref_on, bound_on, either):
    """the ReLU-gated output: the gated reference, or on `either` elements the other branch as well (gated reference 0 <-> the
    ungated value ref_on)"""
    g = got.to(F64)
    return torch.where(either, ((g - ref_on).abs() <= bound_on) | (g == 0), torch.ones_like(either))


def sum_bound(elem_bound, mags, px=(0, 1, 2)):
    """a statistics row: the element gate propagated through the sum + the fp32 summation"""
    return elem_bound.sum(px) + SUM_ULPS * mags.sum(px)


def square_bound(ref, e):
    """|got^2 - ref^2| for |got - ref| <= e"""
    return (2.0 * ref.abs() + e) * e


def flip_allowance_wgrad(a_abs, dz_flip_ulp):
    """per dW entry: sum over pixels of |a| * ulp_bf16(dz) on the pixels whose dz may round the other way"""
    return wgrad_ref(a_abs, dz_flip_ulp)


# ---- operand draws (CPU generator; move with .to(device)) ----------------------------------------------------------------------------
def _ints(g, shape, m):
    return torch.randint(-m, m + 1, shape, generator=g).to(torch.float32)


def _chan(v, n, npad):
    out = torch.zeros(npad)
    out[:n] = v[:n]
    return out


def conv_seed(shape):
    B, H, W, Ci, Co = shape
    return B * 1000003 + H * 1009 + W * 31 + Ci * 7 + Co


def draw_conv(shape, family, m=2):
    """operands of one layer; activations NHWC with padded channels exactly 0, per-channel coefficients 0 on the padded channels.
    Activation tensors hold bf16-representable fp32 values (the caller stores them as bf16); w is bf16-representable too."""
    B, H, W, Ci, Co = shape
    Cip, Cop = pad32(Ci), pad32(Co)
    g = torch.Generator().manual_seed(conv_seed(shape) + (0 if family == "exact" else 1))
    ex = family == "exact"

    def act(Cn, Cp, h=H, w=W, mult=1):
        t = torch.zeros(B, h, w, Cp)
        t[..., :Cn] = _ints(g, (B, h, w, Cn), m) * mult if ex else torch.randn(B, h, w, Cn, generator=g).to(BF).float()
        return t

    def coef(Cn, Cp, kind):
        if ex:
            v = {"scale": torch.randint(1, 3, (Cn,), generator=g).float(), "shift": _ints(g, (Cn,), 2), "int": _ints(g, (Cn,), m),
                 "mean": _ints(g, (Cn,), 1), "invstd": torch.exp2(torch.randint(-1, 2, (Cn,), generator=g).float())}[kind]
        else:
            v = {"scale": torch.rand(Cn, generator=g) + 0.5, "shift": torch.randn(Cn, generator=g) * 0.3,
                 "int": torch.randn(Cn, generator=g) * (1.0 if kind == "int" else 0.1), "mean": torch.randn(Cn, generator=g) * 0.1,
                 "invstd": torch.rand(Cn, generator=g) + 0.5}[kind]
        return _chan(v, Cn, Cp)

    o = {"shape": shape, "family": family, "m": m, "Cip": Cip, "Cop": Cop}
    o["x"] = act(Ci, Cip)
    o["sc_i"], o["sh_i"] = coef(Ci, Cip, "scale"), coef(Ci, Cip, "shift")
    o["w"] = _ints(g, (Co, Ci, 3, 3), m) if ex else (torch.randn(Co, Ci, 3, 3, generator=g) * 0.05).to(BF).float()
    o["dz"] = act(Co, Cop)
    o["zref"] = act(Ci, Cip)
    o["mean_i"], o["invstd_i"] = coef(Ci, Cip, "mean"), coef(Ci, Cip, "invstd")
    o["z"] = act(Co, Cop)
    o["sc_o"], o["sh_o"] = coef(Co, Cop, "scale"), coef(Co, Cop, "shift")
    o["ca"] = coef(Co, Cop, "int")
    o["cb"], o["cc"] = (coef(Co, Cop, "int") * (1.0 if ex else 0.1) for _ in range(2))
    o["g"] = act(Co, Cop)
    o["g2"] = act(Co, Cop, H // 2, W // 2, mult=4)
    return o


def draw_pool_z(shape, family):
    """the full-resolution z [B][2H+1][2W][C] whose pooled activation sed_conv3x3_dgrad_poolstats reads (the odd row is dropped by the
    pooling floor); shape = (B, H, W, C, Cd) of the pooled layer"""
    B, H, W, Cc = shape[:4]
    g = torch.Generator().manual_seed(conv_seed(shape) + 99)
    if family == "exact":
        return _ints(g, (B, 2 * H + 1, 2 * W, Cc), 2)
    return torch.randn(B, 2 * H + 1, 2 * W, Cc, generator=g).to(BF).float()


def draw_c1(B, H, family, m=1, seed=0):
    """block 0 in C1 mode (W = 64, 1 -> 32 -> 32 channels): the Cin = 1 layer's operands, conv2's weights and the operands of conv2's
    backward.  exact: fmean = 0, fstd a power of two, x1 = fstd * integer in {-1..1} (so the z-score is that integer)."""
    W, Cc = 64, 32
    g = torch.Generator().manual_seed(7919 * B + 31 * H + seed + (0 if family == "exact" else 1))
    ex = family == "exact"
    o = {"shape": (B, H, W, Cc, Cc), "family": family, "m": m, "Cip": Cc, "Cop": Cc}
    if ex:
        o["fmean"] = torch.zeros(W)
        o["fstd"] = torch.exp2(torch.randint(-1, 2, (W,), generator=g).float())
        o["x1"] = _ints(g, (B, H, W), 1) * o["fstd"]
        o["w1"] = _ints(g, (Cc, 1, 3, 3), 1)
        o["sc1"], o["sh1"] = torch.randint(1, 3, (Cc,), generator=g).float(), _ints(g, (Cc,), 2)
        o["w2"] = _ints(g, (Cc, Cc, 3, 3), m)
        o["z2"], o["dz"] = _ints(g, (B, H, W, Cc), m), _ints(g, (B, H, W, Cc), m)
        o["dy"] = _ints(g, (B, H // 2, W // 2, Cc), m) * 4
        o["sc2"], o["sh2"] = torch.randint(1, 3, (Cc,), generator=g).float(), _ints(g, (Cc,), 2)
        o["ca"], o["cb"], o["cc"] = (_ints(g, (Cc,), m) for _ in range(3))
    else:
        o["x1"] = torch.randn(B, H, W, generator=g) * 3.0 + 1.0
        o["fmean"], o["fstd"] = torch.randn(W, generator=g), torch.rand(W, generator=g) + 0.5
        o["w1"] = torch.randn(Cc, 1, 3, 3, generator=g) * 0.4
        o["sc1"], o["sh1"] = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
        o["w2"] = (torch.randn(Cc, Cc, 3, 3, generator=g) * 0.05).to(BF).float()
        o["z2"], o["dz"] = (torch.randn(B, H, W, Cc, generator=g).to(BF).float() for _ in range(2))
        o["dy"] = torch.randn(B, H // 2, W // 2, Cc, generator=g).to(BF).float()
        o["sc2"], o["sh2"] = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
        o["ca"], o["cb"], o["cc"] = (torch.randn(Cc, generator=g) * s for s in (1.0, 0.1, 0.1))
    return o


# ---- the exact family's < 2^24 conditions from K * max|a| * max|b| (no full-size convolution needed) --------------------------------
def exact_bounds_conv(shape, m=2, pro_max=None):
    """upper bounds on the sums of magnitudes of one conv layer's exact-family contractions: forward (with the BN+ReLU prologue,
    |a| <= 2m + 2), data gradient, weight gradient with dz <= m*m + m*m + m, and the fused kernels' data gradient from that dz"""
    B, H, W, Ci, Co = shape
    amax = 2 * m + 2 if pro_max is None else pro_max
    dzmax = 2 * m * m + m
    return {"fwd": 9 * Ci * amax * m, "dgrad": 9 * Co * m * m, "wgrad": B * H * W * amax * dzmax, "dgrad_of_dz": 9 * Co * dzmax * m}


def exact_bounds_c1(B, H, m=1):
    """block 0: conv1's pre-activation, conv2's forward on a1 <= 9*2 + 2, dW2, g = conv2^T(dz) with |dz| <= 2 m^2 + m, the A rows"""
    px = B * H * 64
    a1 = 9 * 2 + 2
    dzmax = 2 * m * m + m
    gmax = 9 * 32 * dzmax * m
    return {"pre": a1, "fwd": 9 * 32 * a1 * m, "wgrad": px * a1 * dzmax, "g": gmax, "A": px * gmax * 1, "g_given": 9 * 32 * m * m,
            "A_given": px * 9 * 32 * m * m}


# ---- mutants: each returns a mutated COPY of a reference output --------------------------------------------------------------------
def mutant_corner_product(z, a, w):
    """forward: one product dropped at an image corner (pixel (0, 0) of the last image, output channel 0, centre tap, input 0)"""
    out = z.clone()
    out[-1, 0, 0, 0] -= a[-1, 0, 0, 0] * w[0, 0, 1, 1]
    return out


def mutant_halo_row(a, w):
    """forward: the halo row above image 1 taken from the last row of image 0 instead of the zero padding; returns the mutated z of
    image 1's first row [W][Co] computed directly"""
    row = a[0, -1]                                                          # [W][Ci]
    rp = F.pad(row, (0, 0, 1, 1))
    Wd = row.shape[0]
    return sum(rp[j:j + Wd] @ w[:, :, 0, j].t() for j in range(3))          # the extra contribution to z[1, 0]


def mutant_tap_zeroed(z, a, w, co=0, tap=(0, 2)):
    """forward: one tap's weights zeroed for one output channel"""
    B, H, W, _ = a.shape
    ap = F.pad(a, (0, 0, 1, 1, 1, 1))
    i, j = tap
    out = z.clone()
    out[..., co] -= ap[:, i:i + H, j:j + W, :] @ w[co, :, i, j]
    return out


def pixel_dw(a, dz, b, h, w_):
    """the contribution of pixel (b, h, w_) to dw [Co][Ci][3][3], computed from that pixel's operands alone"""
    B, H, W, Ci = a.shape
    out = torch.zeros(dz.shape[-1], Ci, 3, 3, dtype=a.dtype, device=a.device)
    for i in range(3):
        for j in range(3):
            hh, ww = h + i - 1, w_ + j - 1
            if 0 <= hh < H and 0 <= ww < W:
                out[:, :, i, j] = torch.outer(dz[b, h, w_], a[b, hh, ww])
    return out


def mutant_strip_pixel_twice(dw, a, dz, b, h):
    """dW: the last pixel of a strip (row h of image b, last column) counted twice"""
    return dw + pixel_dw(a, dz, b, h, a.shape[2] - 1)


def mutant_stat_missing_pixel(row, z, b, h, w_):
    """a statistics row (sum over pixels of z) missing one pixel"""
    return row - z[b, h, w_]
