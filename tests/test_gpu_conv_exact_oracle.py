"""GPU: the reference-exact 3x3 conv kernels (dtype SED_F32 = fp32 MFMA, csrc/sed_conv.hip and csrc/sed_conv_wgrad.hip; SED_F32H3 / SED_F32X3 = split operands,
csrc/sed_conv_x3.hip and csrc/sed_wgrad_x3.hip) against float64, through the C ABI, at the specialised widths W in {8, 16, 32, 64}.

Reference: the same contraction in float64 on the device (nine shifted float64 GEMMs over NHWC tensors), on the fp32 operands the
kernel reads.  Each shape's references are computed once and shared by every dtype and kernel form (module cache, one shape at a time).

Gate, per element: |got - ref| <= c * S, S = the same contraction over absolute values (|x| * |w|, |dz| * |w^T|, |a| (x) |dz|) in
float64; an output with S = 0 must be exactly 0.  The constants are derived, not measured:
  - SED_F32 has exact products; SED_F32H3 rounds each operand to hi + lo/2^11 (fp16 pieces) and drops lo.lo: <= 3 * 2^-22 of each
    product.  fp32 accumulation over K <= 4608 terms adds ~sqrt(K) * 2^-24 <= 2^-18 of S for independent rounding errors.  Sum:
    <= 2^-18.5 of S; c = 2^-16 keeps a factor > 4 of margin.
  - SED_F32X3 (bf16 pieces): <= 3 * 2^-18 of each product -> 2^-16.4 of S plus accumulation; c = 2^-13 keeps a factor > 8.
  - The weight gradient contracts over pixels (K = B*H*W, up to 655360 here), but in three levels, each with its own fp32
    accumulator: the MFMA chain of one 128-pixel tile (64 steps), the tiles of one strip (<= 5 here), then the reduction of <= 1024
    strip slabs.  ~sqrt(64 + 5 + 1024) * 2^-24 ~ 2^-19 of S, a few times more where the terms do not cancel (BN+ReLU prologue:
    a >= 0 against dz's per-channel constant cc) -- the same c holds, with the smallest margin of the file (measured ~2^-17 on the
    longest strips, identical for SED_F32 and SED_F32H3: summation, not the split).
Sums (BatchNorm statistics partial rows, summed here in float64) take the gate propagated through the sum plus 2^-20 of the sum of
magnitudes for the fp32 summation itself.  The measured max err/S of every check is printed (run with -s) and summarised at the end
of the module.  A sensitivity case runs SED_BF16 on the same operands and requires it to FAIL the fp32 gate.
"""
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32, BF16, X3, H3 = 0, 1, 2, 3
NAME = {F32: "f32", BF16: "bf16", X3: "bf16x3", H3: "f16x3"}
C_GATE = {F32: 2.0 ** -16, H3: 2.0 ** -16, X3: 2.0 ** -13}
SUM_ULPS = 2.0 ** -20          # fp32 summation inside the partial rows, relative to the sum of magnitudes
DZ_ULPS = 2.0 ** -21           # dz = ca*g + cb*z + cc in fp32 (a few roundings), relative to |ca*g| + |cb*z| + |cc|
DZ_GIVEN, DZ_POOL, DZ_BN = 0, 1, 2
MAX_PARTS = 1024               # sed_conv_nparts' cap (kMaxParts, csrc/sed_conv.hip)

# B, H, W, Cin, Cout
MAIN = [(2, 37, 64, 32, 32), (3, 19, 32, 32, 64), (2, 41, 32, 64, 64), (2, 29, 16, 64, 128), (2, 33, 16, 128, 128), (3, 17, 8, 128, 128)]
DEFAULT_NET = [(2, 23, 64, 64, 64), (2, 21, 32, 64, 128), (2, 19, 16, 128, 256), (2, 13, 16, 256, 256), (2, 11, 8, 256, 512),
               (1, 9, 8, 512, 512)]
EDGES = [(1, 1, 64, 32, 32), (2, 1, 8, 128, 128),          # one row
         (2, 2, 16, 64, 64), (3, 2, 32, 32, 64),           # two rows, pool 2
         (2, 13, 16, 20, 17), (2, 11, 32, 40, 100)]        # padded channels (Cinp 32 / 64, Coutp 32 / 128)
# long strips: the partial-row cap gives several 128-pixel tiles per strip (value: the count the shape is here for)
LONG = {(3, 1801, 64, 32, 32): 3, (2, 6001, 32, 64, 64): 3, (1, 10240, 64, 32, 32): 5, (160, 9, 32, 64, 64): 2,
        (300, 20, 16, 128, 128): 2}
SHAPES = MAIN + DEFAULT_NET + EDGES + list(LONG)

# A/B knobs of the split-operand kernels; "" = the default route
FWD_FORMS = {"form2": {"SED_X3_FORM": "2"}, "form1": {"SED_X3_FORM": "1"}, "pair0": {"SED_X3_PAIR": "0"}}
WG_FORMS = {"wg_a": {"SED_X3_WGRAD": "a"},                 # the all-waves weight-gradient kernel under f16x3 too
            "wg_p": {"SED_X3_WGRAD": "p"},                 # the producer/consumer one at W = 64, Coutp % 64 != 0
            "wgwn2": {"SED_X3_WGWN": "2", "SED_X3_WGRAD": "a"}}   # the wide all-waves form (f16x3 reaches it past the p/c kernel)
FORMS = {"": {}, **FWD_FORMS, **WG_FORMS}
FWD_FORM_SHAPES = [(2, 37, 64, 32, 32), (2, 41, 32, 64, 64), (2, 29, 16, 64, 128), (3, 17, 8, 128, 128), (2, 11, 32, 40, 100),
                   (2, 6001, 32, 64, 64)]
WG_FORM_SHAPES = {"wg_a": [(2, 41, 32, 64, 64), (3, 17, 8, 128, 128), (2, 13, 16, 20, 17), (2, 6001, 32, 64, 64)],
                  "wg_p": [(2, 37, 64, 32, 32), (1, 1, 64, 32, 32), (3, 1801, 64, 32, 32)],
                  "wgwn2": [(2, 41, 32, 64, 64), (2, 19, 16, 128, 256), (2, 11, 32, 40, 100)]}


def _cases():
    out = []
    for s in SHAPES:                     # shape-major: the reference cache holds one shape at a time
        out += [(s, kind, dt, "") for kind in ("fwd", "dgrad", "wgrad") for dt in (F32, H3, X3)]
        if s in FWD_FORM_SHAPES:
            out += [(s, kind, dt, form) for form in FWD_FORMS for kind in ("fwd", "dgrad") for dt in (H3, X3)]
        for form, shapes in WG_FORM_SHAPES.items():
            if s in shapes:
                out += [(s, "wgrad", dt, form) for dt in ((H3,) if form == "wg_p" else (H3, X3))]
    return out


CASES = _cases()
RATIOS = {}                              # (dtype, form, check) -> max err/S measured


def _id(c):
    (B, H, W, Ci, Co), kind, dt, form = c
    return f"{B}x{H}x{W}_{Ci}-{Co}-{kind}-{NAME[dt]}" + (f"-{form}" if form else "")


def cdiv(a, b):
    return -(-a // b)


def pad32(c):
    return cdiv(c, 32) * 32


def x3_tiles_per_strip(B, H, W):
    """(tiles per strip, strips) of the default split-operand forward: 128-pixel tiles (TH = 128 / W rows), one strip per
    partial-statistics row, sed_conv_nparts() = min(B * cdiv(H*W, 256), 1024) of them (launch_x3, csrc/sed_conv_x3.hip)"""
    nparts = min(B * cdiv(H * W, 256), MAX_PARTS)
    return cdiv(B * cdiv(H, 128 // W), nparts), nparts


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module("soundeventdetection-pytorch_amd")._lib


@pytest.fixture(scope="module")
def engine(L):
    pkg = importlib.import_module("soundeventdetection-pytorch_amd")
    return pkg.CnnEngine(1, [(32, 2)], precision="f16x3")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if RATIOS:
        print("\nmax err/S by dtype, form and check (gate c: f32 / f16x3 2^-16 = 1.53e-05, bf16x3 2^-13 = 1.22e-04)")
        for k in sorted(RATIOS):
            print(f"  {k[0]:7s} {k[1] or 'default':7s} {k[2]:40s} {RATIOS[k]:.3e}")
    _CACHE.clear()


def _grad_exp(engine, B, H, W):
    """the pre-scale exponent the engine gives this layer's backward launches (bits 8..15 of their dtype argument)"""
    dt = engine._grad_dtype(B, H, W)
    assert dt & 0xff == H3
    e = (dt >> 8) & 0xff
    return e - 256 if e >= 128 else e


def _with_exp(dt, e):
    return dt | ((e & 0xff) << 8) if dt == H3 else dt


# ---- float64 references (NHWC, on the device) ----------------------------------------------------------------------------------
def conv_ref(a, w):
    """a [B][H][W][Ci], w [Co][Ci][3][3] (float64) -> [B][H][W][Co]: 3x3 conv, stride 1, zero padding 1"""
    B, H, W, _ = a.shape
    ap = F.pad(a, (0, 0, 1, 1, 1, 1))
    z = None
    for i in range(3):
        for j in range(3):
            t = ap[:, i:i + H, j:j + W, :] @ w[:, :, i, j].t()
            z = t if z is None else z + t
    return z


def wgrad_ref(a, dz):
    """dw [Co][Ci][3][3] = sum over pixels of a[h+i-1][w+j-1][ci] * dz[h][w][co] (float64)"""
    B, H, W, Ci = a.shape
    ap = F.pad(a, (0, 0, 1, 1, 1, 1))
    d2 = dz.reshape(-1, dz.shape[-1])
    dw = torch.empty(dz.shape[-1], Ci, 3, 3, dtype=torch.float64, device=a.device)
    for i in range(3):
        for j in range(3):
            dw[:, :, i, j] = (ap[:, i:i + H, j:j + W, :].reshape(-1, Ci).t() @ d2).t()
    return dw


def dgrad_w(w):
    """the data gradient as a forward conv: W'[c][o][i][j] = W[o][c][2-i][2-j]"""
    return w.permute(1, 0, 2, 3).flip(2, 3)


def to_pack_layout(dw, Cinp, Coutp):
    """dw [Co][Ci][3][3] -> dwpack [9][Cinp][Coutp], zero padded"""
    Co, Ci = dw.shape[:2]
    out = torch.zeros(9, Cinp, Coutp, dtype=dw.dtype, device=dw.device)
    out[:, :Ci, :Co] = dw.permute(2, 3, 1, 0).reshape(9, Ci, Co)
    return out


def record(dt, form, what, got, ref, S):
    err = (got.double() - ref).abs()
    pos = S > 0
    r = float((err[pos] / S[pos]).max()) if bool(pos.any()) else 0.0
    if not math.isfinite(r) or bool(torch.isnan(got).any()):
        r = math.inf
    key = (NAME[dt], form, what)
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    return err, r


def assert_gate(dt, form, what, got, ref, S):
    c = C_GATE[dt]
    err, r = record(dt, form, what, got, ref, S)
    ok = err <= c * S                          # NaN fails; S = 0 demands an exact 0
    nbad = int((~ok).sum())
    print(f"  {NAME[dt]:7s} {form or 'default':7s} {what:40s} max err/S {r:.3e}")
    assert nbad == 0, f"{what}: {nbad} of {ok.numel()} elements over the gate, max err/S {r:.3e} > c = {c:.3e}"


def assert_sum(what, got, ref, bound):
    d = (got.double() - ref).abs()
    assert bool((d <= bound).all()), f"{what}: max excess over the bound {float((d - bound).max()):.3e} (max |err| {float(d.max()):.3e})"


# ---- operands and cached references ------------------------------------------------------------------------------------------
_CACHE = {}


def _away_from_zero(z, sc, sh, C):
    """move every element whose BN value sc*z+sh lies within 2e-3 of 0 (real channels) to sc*z+sh ~ 0.01: the kernels' fp32 ReLU
    decisions then agree with float64 exactly"""
    t = z[..., :C] * sc[:C] + sh[:C]
    fix = ((0.01 - sh[:C]) / sc[:C]).expand_as(t)
    z[..., :C] = torch.where(t.abs() < 2e-3, fix, z[..., :C])
    t = z[..., :C].double() * sc[:C].double() + sh[:C].double()
    assert float(t.abs().min()) >= 1e-3
    return z


def operands(shape):
    """deterministic fp32 operands of one shape; padded channels exactly 0 and their per-channel coefficients 0 (the engine's
    convention).  Gradients at unit scale: the tests multiply them by exact powers of two."""
    if shape in _CACHE:
        return _CACHE[shape]
    _CACHE.clear()
    torch.cuda.empty_cache()
    B, H, W, Ci, Co = shape
    Cip, Cop = pad32(Ci), pad32(Co)
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(B * 1000003 + H * 1009 + W * 31 + Ci * 7 + Co)

    def chan(n, npad, lo, scale, uniform=False):
        v = torch.zeros(npad, device=dev)
        v[:n] = (torch.rand(n, device=dev, generator=g) if uniform else torch.randn(n, device=dev, generator=g)) * scale + lo
        return v

    def act(C, Cp, h=H, w=W):
        t = torch.zeros(B, h, w, Cp, device=dev)
        t[..., :C] = torch.randn(B, h, w, C, device=dev, generator=g)
        return t

    o = {"Cip": Cip, "Cop": Cop, "refs": {}}
    o["x"] = act(Ci, Cip)
    o["sc_i"], o["sh_i"] = chan(Ci, Cip, 0.5, 1.0, True), chan(Ci, Cip, 0.0, 0.3)
    o["w"] = torch.randn(Co, Ci, 3, 3, device=dev, generator=g) * 0.05
    o["wd"] = torch.zeros(Cop, Cip, 3, 3, dtype=torch.float64, device=dev)
    o["wd"][:Co, :Ci] = o["w"].double()
    # data gradient: conv^T of a Co-channel gradient into the Ci channels, ReLU / BN1 epilogue on those
    o["dz"] = act(Co, Cop)
    o["mean"], o["invstd"] = chan(Ci, Cip, 0.0, 0.1), chan(Ci, Cip, 0.5, 1.0, True)
    o["zref"] = _away_from_zero(act(Ci, Cip), o["sc_i"], o["sh_i"], Ci)
    # weight gradient: dz produced from (gsrc, z) over the Co channels
    o["sc_o"], o["sh_o"] = chan(Co, Cop, 0.5, 1.0, True), chan(Co, Cop, 0.0, 0.3)
    o["z"] = _away_from_zero(act(Co, Cop), o["sc_o"], o["sh_o"], Co)
    o["ca"], o["cb"], o["cc"] = chan(Co, Cop, 0.5, 1.0, True), chan(Co, Cop, 0.0, 0.1), chan(Co, Cop, 0.0, 0.1)
    o["g"] = act(Co, Cop)
    if H >= 2:
        o["g2"] = act(Co, Cop, H // 2, W // 2)
    _CACHE[shape] = o
    return o


def cached(o, key, fn):
    if key not in o["refs"]:
        o["refs"][key] = fn()
    return o["refs"][key]


def prologue(o, pro):
    """the conv input as the loader forms it (relu(scale*x + shift) in fp32), in float64"""
    x = o["x"]
    return (torch.relu(x * o["sc_i"] + o["sh_i"]) if pro else x).double()


def pack(L, dt, w, Cip, Cop, tf):
    Co, Ci = w.shape[:2]
    wp = torch.full((9 * Cip * Cop,), float("nan"), device="cuda", dtype=torch.bfloat16 if dt == BF16 else torch.float32)
    L.check(L.lib().sed_pack_conv_weight(dt, L.ptr(w), L.ptr(wp), Co, Ci, Cop, Cip, tf, torch.cuda.current_stream().cuda_stream))
    return wp


def dz_unit(o, H, dzmode, pool):
    """(gsrc, float64 dz, float64 error scale |ca*g| + |cb*z| + |cc|) of one dz mode at unit gradient scale"""
    if dzmode == DZ_GIVEN:
        return o["g"], o["g"].double(), None
    z = o["z"].double()
    gsrc = o["g2"] if (dzmode == DZ_POOL and pool == 2) else o["g"]
    if dzmode == DZ_POOL and pool == 2:            # floor pooling: an odd last row gets no gradient (avgpool_bwd)
        gfull = torch.zeros_like(z)
        up = gsrc.double().repeat_interleave(2, 1).repeat_interleave(2, 2) / 4.0
        gfull[:, :up.shape[1], :up.shape[2]] = up
    else:
        gfull = gsrc.double()
    if dzmode == DZ_POOL:
        gfull = gfull * ((z * o["sc_o"].double() + o["sh_o"].double()) > 0)
    ca, cb, cc = o["ca"].double(), o["cb"].double(), o["cc"].double()
    return gsrc, ca * gfull + cb * z + cc, (ca * gfull).abs() + (cb * z).abs() + cc.abs()


# ---- the three entry points --------------------------------------------------------------------------------------------------
def check_fwd(L, shape, dt, form, o):
    B, H, W, Ci, Co = shape
    Cip, Cop = o["Cip"], o["Cop"]
    lib, P = L.lib(), L.ptr
    st = torch.cuda.current_stream().cuda_stream
    nparts = lib.sed_conv_nparts(B, H, W)
    assert nparts == x3_tiles_per_strip(B, H, W)[1]
    wp = pack(L, dt, o["w"], Cip, Cop, 0)
    c = C_GATE[dt]
    for pro in (0, 1):
        zr, S = cached(o, ("fwd", pro), lambda: (conv_ref(prologue(o, pro), o["wd"]), conv_ref(prologue(o, pro).abs(), o["wd"].abs())))
        for epi in (0, 1):
            z = torch.full((B, H, W, Cop), float("nan"), device="cuda")
            part = torch.full((nparts, 2, Cop), float("nan"), device="cuda")
            L.check(lib.sed_conv3x3_fwd(dt, pro, epi, P(o["x"]), P(o["sc_i"]) if pro else None, P(o["sh_i"]) if pro else None,
                                        P(wp), P(z), None, None, None, None, None, P(part) if epi else None, B, H, W, Cip, Cop, st))
            torch.cuda.synchronize()
            assert_gate(dt, form, f"fwd pro={pro} epi={epi}", z, zr, S)
            if epi:
                s = part.double().sum(0)
                az, px = zr.abs(), (0, 1, 2)
                assert_sum("sum z", s[0], zr.sum(px), c * S.sum(px) + SUM_ULPS * az.sum(px))
                assert_sum("sum z^2", s[1], (zr * zr).sum(px), 2 * c * (az * S).sum(px) + SUM_ULPS * (zr * zr).sum(px))


def run_dgrad(L, shape, dt, o, e, dz):
    B, H, W = shape[:3]
    Cip, Cop = o["Cip"], o["Cop"]
    lib, P = L.lib(), L.ptr
    nparts = lib.sed_conv_nparts(B, H, W)
    wpt = pack(L, dt, o["w"], Cip, Cop, 1)
    out = torch.full((B, H, W, Cip), float("nan"), device="cuda")
    part = torch.full((nparts, 2, Cip), float("nan"), device="cuda")
    L.check(lib.sed_conv3x3_fwd(_with_exp(dt, e), 0, 2, P(dz), None, None, P(wpt), P(out), P(o["zref"]), P(o["sc_i"]), P(o["sh_i"]),
                                P(o["mean"]), P(o["invstd"]), P(part), B, H, W, Cop, Cip, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out, part


def check_dgrad(L, shape, dt, form, o, e, gs, what="dgrad"):
    """g = relu'(scale*zref + shift) * conv^T(dz) and the partials (sum g, sum g*xhat), dz = gs * unit gradient"""
    out, part = run_dgrad(L, shape, dt, o, e, o["dz"] * gs)
    zr = o["zref"].double()

    def ref():
        gate = (zr * o["sc_i"].double() + o["sh_i"].double()) > 0
        wt = dgrad_w(o["wd"])
        return conv_ref(o["dz"].double(), wt) * gate, conv_ref(o["dz"].double().abs(), wt.abs()) * gate
    gr, S = (t * gs for t in cached(o, ("dgrad",), ref))       # gs is a power of two: exact
    assert_gate(dt, form, f"{what} g", out, gr, S)
    xh = (zr - o["mean"].double()) * o["invstd"].double()
    s, c, px = part.double().sum(0), C_GATE[dt], (0, 1, 2)
    assert_sum(f"{what} sum g", s[0], gr.sum(px), c * S.sum(px) + SUM_ULPS * gr.abs().sum(px))
    assert_sum(f"{what} sum g*xhat", s[1], (gr * xh).sum(px), c * (xh.abs() * S).sum(px) + SUM_ULPS * (gr * xh).abs().sum(px))


WG_COMBOS = [(DZ_GIVEN, 1, 0), (DZ_GIVEN, 1, 1), (DZ_BN, 1, 0), (DZ_BN, 1, 1), (DZ_POOL, 1, 1), (DZ_POOL, 2, 0), (DZ_POOL, 2, 1)]


def check_wgrad(L, shape, dt, form, o, e, gs, combos=WG_COMBOS, what="wgrad"):
    """dwpack / torch-layout dw of sed_conv3x3_wgrad_u (dz given) and sed_conv3x3_wgrad_fused_u (dz produced, written to dz_out)"""
    B, H, W, Ci, Co = shape
    Cip, Cop = o["Cip"], o["Cop"]
    lib, P = L.lib(), L.ptr
    st = torch.cuda.current_stream().cuda_stream
    nws = lib.sed_conv_wgrad_ws_floats(B, H, W, Cip, Cop)
    for dzmode, pool, pro in combos:
        if pool == 2 and H < 2:
            continue                                     # (a 2x2 pool needs two rows)
        tag = f"{what} dz={('given', 'pool', 'bn')[dzmode]} p{pool} pro={pro}"
        gsrc, dzr, dzs = dz_unit(o, H, dzmode, pool)
        ws = torch.full((nws + 256,), float("nan"), device="cuda")
        ws[:nws] = -5.0
        dzo = torch.full((B, H, W, Cop), float("nan"), device="cuda")
        dwp = torch.full((9 * Cip * Cop,), float("nan"), device="cuda")
        dw = torch.full((Co, Ci, 3, 3), float("nan"), device="cuda")
        ps, ph = (P(o["sc_i"]), P(o["sh_i"])) if pro else (None, None)
        gsrc = gsrc * gs
        if dzmode == DZ_GIVEN:
            L.check(lib.sed_conv3x3_wgrad_u(_with_exp(dt, e), pro, P(o["x"]), ps, ph, P(gsrc), P(dwp), P(ws), B, H, W, Cip, Cop,
                                            P(dw), Co, Ci, st))
        else:
            pooled = dzmode == DZ_POOL
            cb, cc = o["cb"] * gs, o["cc"] * gs
            L.check(lib.sed_conv3x3_wgrad_fused_u(_with_exp(dt, e), pro, P(o["x"]), ps, ph, dzmode, P(gsrc), P(o["z"]),
                                                  P(o["sc_o"]) if pooled else None, P(o["sh_o"]) if pooled else None,
                                                  P(o["ca"]), P(cb), P(cc), pool, P(dzo), P(dwp), P(ws), B, H, W, Cip, Cop,
                                                  P(dw), Co, Ci, st))
        torch.cuda.synchronize()
        assert bool(torch.isnan(ws[nws:]).all()), f"{tag}: workspace written past sed_conv_wgrad_ws_floats"
        if dzmode != DZ_GIVEN:
            d = (dzo.double() - dzr * gs).abs()
            bad = int((~(d <= DZ_ULPS * gs * dzs)).sum())
            assert bad == 0, f"{tag}: {bad} dz_out elements off the float64 dz by more than 2^-21 of |ca*g| + |cb*z| + |cc|"
        dwr, S = (t * gs for t in cached(o, ("wgrad", dzmode, pool, pro),
                                         lambda: (wgrad_ref(prologue(o, pro), dzr), wgrad_ref(prologue(o, pro).abs(), dzr.abs()))))
        assert_gate(dt, form, f"{tag} dwpack", dwp.view(9, Cip, Cop), to_pack_layout(dwr, Cip, Cop), to_pack_layout(S, Cip, Cop))
        unpacked = dwp.view(3, 3, Cip, Cop)[:, :, :Ci, :Co].permute(3, 2, 0, 1)
        assert torch.equal(dw, unpacked), f"{tag}: torch-layout dw differs from the unpacked dwpack"


# ---- tests -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(LONG))
def test_long_strip_tile_counts(L, shape):
    """each long-strip shape holds the tiles per strip it is listed for (3 and 5: several tiles, odd counts for the tile pairs)"""
    B, H, W = shape[:3]
    tps, nparts = x3_tiles_per_strip(B, H, W)
    assert nparts == L.lib().sed_conv_nparts(B, H, W)
    assert tps == LONG[shape]


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_conv_vs_float64(L, engine, monkeypatch, case):
    """forward (every prologue x epilogue pair, statistics), data gradient (ReLU-backward / BN1 partials), weight gradient (dz given,
    BN-produced, pool-produced with pool 1 / 2; with and without the prologue) of one shape, dtype and kernel form.  Outputs are
    pre-filled with NaN: every element, padded channels included (those exactly 0), must be written."""
    shape, kind, dt, form = case
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    L.lib().sed_config_reload()
    B, H, W = shape[:3]
    o = operands(shape)
    e = _grad_exp(engine, B, H, W)
    gs = 2.0 ** (2 - e)                  # the gradient scale the engine's exponent is chosen for (2^e * gs = 4)
    if kind == "fwd":
        check_fwd(L, shape, dt, form, o)
    elif kind == "dgrad":
        check_dgrad(L, shape, dt, form, o, e, gs)
    else:
        check_wgrad(L, shape, dt, form, o, e, gs)


@pytest.mark.parametrize("shape", [(2, 41, 32, 64, 64), (2, 13, 16, 256, 256)])
def test_bf16_fails_the_fp32_gate(L, shape):
    """sensitivity: the bf16 kernel on the same operands (rounded to bf16 on the way in) misses the fp32 gate by far"""
    B, H, W, Ci, Co = shape
    o = operands(shape)
    lib, P = L.lib(), L.ptr
    nparts = lib.sed_conv_nparts(B, H, W)
    wp = pack(L, BF16, o["w"], o["Cip"], o["Cop"], 0)
    xb = o["x"].to(torch.bfloat16)
    z = torch.full((B, H, W, o["Cop"]), float("nan"), device="cuda", dtype=torch.bfloat16)
    part = torch.full((nparts, 2, o["Cop"]), float("nan"), device="cuda")
    L.check(lib.sed_conv3x3_fwd(BF16, 0, 1, P(xb), None, None, P(wp), P(z), None, None, None, None, None, P(part), B, H, W,
                                o["Cip"], o["Cop"], torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    a = o["x"].double()
    zr, S = conv_ref(a, o["wd"]), conv_ref(a.abs(), o["wd"].abs())
    err, r = record(BF16, "", "fwd (sensitivity)", z, zr, S)
    nbad = int((err > C_GATE[F32] * S).sum())
    print(f"  bf16 against the fp32 gate: max err/S {r:.3e}, {nbad} of {err.numel()} elements over c = {C_GATE[F32]:.2e}")
    assert math.isfinite(r) and nbad > err.numel() // 2, "the fp32 gate cannot tell the bf16 kernel from the fp32 one"


SWEEP_SHAPES = [(2, 41, 32, 64, 64), (3, 17, 8, 128, 128)]
SWEEP_K = (-12, -8, -4, 0, 4, 8, 12)


@pytest.mark.parametrize("shape", SWEEP_SHAPES)
def test_f16x3_gradient_exponent_window(L, engine, shape):
    """f16x3 with the pre-scale exponent e the engine picks (CnnEngine._grad_dtype) across true gradient scales 2^(-e+k),
    k in [-12, 12]: the data gradient and the weight gradient with dz given / BN-produced / pool-produced meet the f16x3 gate"""
    B, H, W = shape[:3]
    o = operands(shape)
    e = _grad_exp(engine, B, H, W)
    for k in SWEEP_K:
        gs = 2.0 ** (k - e)
        check_dgrad(L, shape, H3, "", o, e, gs, what=f"k={k:+d} dgrad")
        check_wgrad(L, shape, H3, "", o, e, gs, combos=[(DZ_GIVEN, 1, 1), (DZ_BN, 1, 0), (DZ_POOL, 2, 1)], what=f"k={k:+d} wgrad")


@pytest.mark.parametrize("shape", SWEEP_SHAPES)
def test_f16x3_gradient_outlier_stays_finite(L, engine, shape):
    """one gradient element 2^17 above the rest (past fp16's range after the pre-scale; clamped to +-60000): every output finite"""
    B, H, W, Ci, Co = shape
    o = operands(shape)
    e = _grad_exp(engine, B, H, W)
    gs = 2.0 ** -e
    lib, P = L.lib(), L.ptr
    st = torch.cuda.current_stream().cuda_stream
    dz = o["dz"] * gs
    dz[B - 1, H // 2, W // 2, 3] = 2.0 ** 17 * gs
    out, part = run_dgrad(L, shape, H3, o, e, dz)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(part).all())
    nws = lib.sed_conv_wgrad_ws_floats(B, H, W, o["Cip"], o["Cop"])
    for dzmode in (DZ_GIVEN, DZ_BN, DZ_POOL):
        g = o["g"] * gs
        g[0, H // 3, W // 4, 5] = 2.0 ** 17 * gs
        ws = torch.zeros(nws, device="cuda")
        dzo = torch.full((B, H, W, o["Cop"]), float("nan"), device="cuda")
        dwp = torch.full((9 * o["Cip"] * o["Cop"],), float("nan"), device="cuda")
        dw = torch.full((Co, Ci, 3, 3), float("nan"), device="cuda")
        if dzmode == DZ_GIVEN:
            L.check(lib.sed_conv3x3_wgrad_u(_with_exp(H3, e), 1, P(o["x"]), P(o["sc_i"]), P(o["sh_i"]), P(g), P(dwp), P(ws),
                                            B, H, W, o["Cip"], o["Cop"], P(dw), Co, Ci, st))
        else:
            pooled = dzmode == DZ_POOL
            cb, cc = o["cb"] * gs, o["cc"] * gs
            L.check(lib.sed_conv3x3_wgrad_fused_u(_with_exp(H3, e), 1, P(o["x"]), P(o["sc_i"]), P(o["sh_i"]), dzmode, P(g), P(o["z"]),
                                                  P(o["sc_o"]) if pooled else None, P(o["sh_o"]) if pooled else None, P(o["ca"]),
                                                  P(cb), P(cc), 1, P(dzo), P(dwp), P(ws), B, H, W, o["Cip"], o["Cop"], P(dw), Co, Ci, st))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dwp).all()) and bool(torch.isfinite(dw).all()), f"dzmode {dzmode}: non-finite weight gradient"
