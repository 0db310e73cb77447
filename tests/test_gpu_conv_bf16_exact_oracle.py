"""GPU: the bf16 3x3 convolution family (dtype SED_BF16: csrc/sed_conv_pc.hip, the LDS-weights and register-weights kernels of
csrc/sed_conv.hip, csrc/sed_conv_anyw.hip, csrc/sed_wgrad.hip, csrc/sed_wgrad_wide.hip, csrc/sed_conv_wgrad.hip, csrc/sed_bwd_fused.hip
and the block-0 C1-mode kernels of csrc/sed_c1.hip, csrc/sed_dgrad_c1.hip, csrc/sed_bwd_fused_c1.hip) against float64, through the C ABI.

References, operand families and gates: tests/conv_bf16_formula.py (its docstring states the derivations; tests/test_conv_bf16_formula_host.py
proves on the CPU that the gates reject a dropped product, a foreign halo row, a zeroed tap, a pixel counted twice, a truncating store
and a statistics row missing a pixel).  In short: the EXACT family (small integers) demands torch-equal fp32 outputs and bit-equal bf16
stores; the RANDOM family takes |got - ref| <= C*S (fp32 results, C = 2^-16) and half a bf16 ulp of the accumulator on top of that
for stored bf16 results, with no absolute floor and no share of elements left out.  References are float64 on the device, cached one
shape at a time.  Every output lies in a NaN-filled buffer between two canary regions: every element must have been written, the
canaries must be intact, the inputs unchanged.

Which value a statistics row sums (read in the kernels; the reference sums the same, the other choice fails on the exact family as
soon as |z| > 256 occurs):
  producer/consumer kernel (default route), STATS and RELUBWD       the STORED bf16 values (the flush reads the staged bf16 tile)
  register-weights kernel (SED_CONV_KERNEL=w), STATS                 the STORED bf16 values (same flush)
  LDS-weights kernel (SED_CONV_KERNEL=l), STATS                      the fp32 ACCUMULATORS (before staging); RELUBWD: the STORED values
  width-general kernels (sed_conv3x3_fwd_anyw), STATS and RELUBWD    the fp32 ACCUMULATORS
  sed_conv3x3_dgrad_poolstats, sed_conv3x3_bwd_fused                 the STORED bf16 dy / g
  C1 mode: sed_conv3x3_fwd_c1 as the producer/consumer kernel; the [A; sum g] rows contract the bf16-ROUNDED gated g on the matrix
  pipe (row 9 against a tile of ones).
Rows that sum stored values are also compared with the float64 sum of the tensor the kernel stored (only the fp32 summation between
them: 2^-20 of the sum of magnitudes) -- far sharper than the propagated element gate at the large shapes.

The worst error/gate of every (entry point, route, check) is collected and printed at the end of the module (run with -s); the exact
family's entries count mismatching elements (0).
"""
import importlib
import math

import pytest
import torch

import conv_bf16_formula as Fm

pytestmark = pytest.mark.gpu

BF16 = 1
STORE, STATS, RELUBWD, POOLSTATS = 0, 1, 2, 4
DZ_POOL, DZ_BN = 1, 2
BF, F64 = torch.bfloat16, torch.float64
CANARY, PAD = -12352.0, 256            # (representable in bf16)
RESULTS = {}                           # (entry, route, family, check) -> worst error/gate (random) or mismatches (exact)
FAMILIES = ("exact", "random")

ROUTES = {"": {}, "l": {"SED_CONV_KERNEL": "l"}, "w": {"SED_CONV_KERNEL": "w"}}
STAT_SOURCE = {"": "stored", "w": "stored", "l": "acc", "anyw": "acc", "col": "stored"}      # forward STATS; RELUBWD: stored except anyw
WG_FORMS = {"": {}, "narrow": {"SED_WGRAD_WIDE": "0"}, "k2": {"SED_WGRAD_WIDE": "0", "SED_WGRAD_KERNEL": "2"},
            "k3": {"SED_WGRAD_KERNEL": "3"}}


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module("soundeventdetection-pytorch_amd")._lib


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if RESULTS:
        print("\nworst error/gate by entry point, route, family and check (exact family: mismatching elements)")
        for k in sorted(RESULTS):
            print(f"  {k[0]:28s} {k[1] or 'default':8s} {k[2]:6s} {k[3]:34s} {RESULTS[k]:.3e}")
    _CACHE.clear()


class Routed:
    """set A/B knobs through monkeypatch, reload the library's cached knobs, restore on exit"""

    def __init__(self, L, monkeypatch, env):
        self.L, self.mp, self.env = L, monkeypatch, env

    def __enter__(self):
        for k, v in self.env.items():
            self.mp.setenv(k, v)
        self.L.lib().sed_config_reload()

    def __exit__(self, *exc):
        for k in self.env:
            self.mp.delenv(k, raising=False)
        self.L.lib().sed_config_reload()
        return False


# ---- buffers -------------------------------------------------------------------------------------------------------------------
class Out:
    """an output tensor pre-filled with a sentinel (NaN; integer tensors: `fill`) between two canary regions"""

    def __init__(self, shape, dtype=BF, canary=CANARY, fill=float("nan")):
        n = math.prod(shape)
        self.flat = torch.full((n + 2 * PAD,), canary, device="cuda", dtype=dtype)
        self.t = self.flat[PAD:PAD + n].view(shape)
        self.t.fill_(fill)
        self.n, self.canary = n, canary

    def verify(self, what):
        assert bool((self.flat[:PAD] == self.canary).all()) and bool((self.flat[PAD + self.n:] == self.canary).all()), f"{what}: canary overwritten"
        if self.t.is_floating_point():
            assert not bool(torch.isnan(self.t).any()), f"{what}: {int(torch.isnan(self.t).sum())} of {self.n} elements not written (or NaN)"
        return self.t


class Frozen:
    """inputs must be unchanged after the call"""

    def __init__(self, *tensors):
        self.pairs = [(t, t.clone()) for t in tensors if t is not None]

    def verify(self, what):
        for i, (t, c) in enumerate(self.pairs):
            assert torch.equal(t, c), f"{what}: input {i} modified by the call"


def st():
    return torch.cuda.current_stream().cuda_stream


def record(entry, route, family, what, value):
    k = (entry, route, family, what)
    RESULTS[k] = max(RESULTS.get(k, 0.0), value)


def expect(entry, route, family, what, ok, got=None, ref=None, bound=None):
    """ok: per-element verdicts; records mismatches (exact) or the worst error/gate (random) and asserts"""
    nbad = int((~ok).sum())
    if family == "exact" or bound is None:
        record(entry, route, family, what, float(nbad))
        worst = ""
    else:
        err = (got.to(F64) - ref).abs()
        b = bound if torch.is_tensor(bound) else torch.full_like(err, bound)
        pos = b > 0
        r = float((err[pos] / b[pos]).max()) if bool(pos.any()) else 0.0
        if bool((err[~pos] > 0).any()) or not math.isfinite(r):
            r = math.inf
        record(entry, route, family, what, r)
        worst = f", worst error/gate {r:.3e}"
    print(f"  {entry:28s} {route or 'default':8s} {family:6s} {what:34s} {RESULTS[(entry, route, family, what)]:.3e}")
    assert nbad == 0, f"{entry} [{route or 'default'}] {family} {what}: {nbad} of {ok.numel()} elements fail{worst}"


def expect_row(entry, route, family, what, got, ref, mags, elem=None):
    """a statistics row (summed over the partial rows in float64).  exact family: equal where the channel's sum of magnitudes is
    below 2^24, the fp32 summation gate elsewhere; random family: the propagated element gate + the fp32 summation"""
    got = got.to(F64)
    if family == "exact":
        small = mags < Fm.LIMIT
        ok = torch.where(small, got.float() == ref.float(), Fm.within(got, ref, Fm.SUM_ULPS * mags))
        expect(entry, route, family, what, ok)
    else:
        bound = Fm.SUM_ULPS * mags + (elem if elem is not None else 0.0)
        expect(entry, route, family, what, Fm.within(got, ref, bound), got, ref, bound)


# ---- operands and cached references -----------------------------------------------------------------------------------------
_CACHE = {}


def operands(key, draw):
    """device copy of one drawn case; the cache holds one case at a time"""
    if key not in _CACHE:
        _CACHE.clear()
        torch.cuda.empty_cache()
        o = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in draw().items()}
        o["refs"] = {}
        _CACHE[key] = o
    return _CACHE[key]


def cached(o, key, fn):
    if key not in o["refs"]:
        o["refs"][key] = fn()
    return o["refs"][key]


def pack(L, w, Cip, Cop, transposed):
    Co, Ci = w.shape[:2]
    wp = Out((9 * Cip * Cop,))
    L.check(L.lib().sed_pack_conv_weight(BF16, L.ptr(w), L.ptr(wp.t), Co, Ci, Cop, Cip, transposed, st()))
    torch.cuda.synchronize()
    return wp.verify("sed_pack_conv_weight")


def wd_of(o):
    """the weights in float64, zero padded to [Cop][Cip][3][3]"""
    def f():
        w = o["w"]
        wd = torch.zeros(o["Cop"], o["Cip"], 3, 3, dtype=F64, device="cuda")
        wd[:w.shape[0], :w.shape[1]] = w.to(F64)
        return wd
    return cached(o, "wd", f)


def activation(o, pro, key="x", sc="sc_i", sh="sh_i"):
    """(a, flip): the conv input as the loader forms it, in float64: x, or relu(scale*x + shift) rounded to bf16; flip = per element,
    how far the kernel's fp32 evaluation may move the rounded value (one bf16 ulp next to a rounding boundary, the fp32 error next
    to the ReLU's kink), None where nothing is rounded"""
    def f():
        x = o[key].to(F64)
        if not pro:
            return x, None
        un = Fm.bn_relu(x, o[sc], o[sh])
        if o["family"] == "exact":
            return un, None
        arg, M = Fm.gate_arg(x, o[sc], o[sh])
        margin = Fm.DZ_ULPS * M
        flip = torch.where(Fm.flip_mask(un, margin), Fm.ulp_bf16(un), torch.zeros_like(un)) + torch.where(arg.abs() <= margin, margin, torch.zeros_like(un))
        return Fm.rne(un), flip
    return cached(o, ("act", pro, key), f)


def nparts_of(L, B, H, W):
    return L.lib().sed_conv_nparts(B, H, W)


# ---- forward (STATS / STORE) -----------------------------------------------------------------------------------------------------
def check_forward(L, o, entry, route, fn, stat_source, pros=(0, 1), wkey="wd"):
    B, H, W, Ci, Co = o["shape"]
    Cip, Cop, fam = o["Cip"], o["Cop"], o["family"]
    P = L.ptr
    wd = wd_of(o) if wkey == "wd" else o["refs"][wkey]
    wp = cached(o, ("wpack", wkey), lambda: pack(L, wd[:Co, :Ci].float().contiguous(), Cip, Cop, 0))
    xb = cached(o, "xb", lambda: o["x"].to(BF))
    nparts = nparts_of(L, B, H, W)
    for pro in pros:
        a, flip = activation(o, pro)
        zr, S, allow = cached(o, ("fwd", pro, wkey), lambda: (Fm.conv_ref(a, wd), Fm.conv_ref(a.abs(), wd.abs()),
                                                            None if flip is None else Fm.conv_ref(flip, wd.abs())))
        if fam == "exact":
            assert Fm.exact_ok(float(S.max())), "the drawn case leaves the exact range"
        for epi in (STATS, STORE):
            z, part = Out((B, H, W, Cop)), Out((nparts, 2, Cop), torch.float32)
            frozen = Frozen(xb, wp, o["sc_i"], o["sh_i"])
            L.check(fn(BF16, pro, epi, P(xb), P(o["sc_i"]) if pro else None, P(o["sh_i"]) if pro else None, P(wp), P(z.t), None, None,
                       None, None, None, P(part.t) if epi else None, B, H, W, Cip, Cop, st()))
            torch.cuda.synchronize()
            tag = f"fwd pro={pro} epi={epi}"
            frozen.verify(tag)
            zt = z.verify(tag + " z")
            if fam == "exact":
                expect(entry, route, fam, tag + " z", Fm.eq_bf16(zt, zr))
            else:
                bound = Fm.bound_bf16(zr, S, allow)
                expect(entry, route, fam, tag + " z", Fm.within(zt, zr, bound), zt, zr, bound)
            if not epi:
                continue
            s = part.verify(tag + " partial").to(F64).sum(0)
            zs = zt.to(F64)
            if stat_source == "stored":          # against the tensor the kernel stored: only the fp32 summation in between
                expect_row(entry, route, fam, tag + " sum z (of stored)", s[0], zs.sum((0, 1, 2)), zs.abs().sum((0, 1, 2)))
                expect_row(entry, route, fam, tag + " sum z^2 (of stored)", s[1], (zs * zs).sum((0, 1, 2)), (zs * zs).sum((0, 1, 2)))
            vals = Fm.rne(zr) if (stat_source == "stored" and fam == "exact") else zr
            e = None if fam == "exact" else (Fm.bound_bf16(zr, S, allow) if stat_source == "stored" else Fm.bound_f32(S, allow))
            expect_row(entry, route, fam, tag + " sum z", s[0], vals.sum((0, 1, 2)), vals.abs().sum((0, 1, 2)),
                       None if e is None else e.sum((0, 1, 2)))
            expect_row(entry, route, fam, tag + " sum z^2", s[1], (vals * vals).sum((0, 1, 2)), (vals * vals).sum((0, 1, 2)),
                       None if e is None else Fm.square_bound(zr, e).sum((0, 1, 2)))


# ---- data gradient with the ReLU / BN-backward epilogue -----------------------------------------------------------------------
def check_relubwd(L, o, entry, route, fn, stat_source):
    """g = [es*zref + et > 0] * conv^T(dz), rows sum g and sum g*xhat (accumulated as sum g*(zref - mean), times invstd at the end)"""
    B, H, W, Ci, Co = o["shape"]
    Cip, Cop, fam = o["Cip"], o["Cop"], o["family"]
    P = L.ptr
    wd = wd_of(o)
    wpt = cached(o, "wpack_t", lambda: pack(L, o["w"], Cip, Cop, 1))
    dzb, zrefb = cached(o, "dzb", lambda: o["dz"].to(BF)), cached(o, "zrefb", lambda: o["zref"].to(BF))
    nparts = nparts_of(L, B, H, W)

    def ref():
        wt = Fm.dgrad_w(wd)
        full, S = Fm.conv_ref(o["dz"].to(F64), wt), Fm.conv_ref(o["dz"].to(F64).abs(), wt.abs())
        arg, _ = Fm.gate_arg(o["zref"], o["sc_i"], o["sh_i"])
        either = Fm.relu_either(o["zref"], o["sc_i"], o["sh_i"]) if fam == "random" else torch.zeros_like(arg, dtype=torch.bool)
        return full, S, arg > 0, either
    full, S, on, either = cached(o, "relubwd", ref)
    if fam == "exact":
        assert Fm.exact_ok(float(S.max()))
    else:
        share = float(either[..., :Ci].double().mean())
        assert share <= Fm.EITHER_SHARE, f"either-branch share {share:.2e}"
    out, part = Out((B, H, W, Cip)), Out((nparts, 2, Cip), torch.float32)
    frozen = Frozen(dzb, zrefb, wpt, o["sc_i"], o["sh_i"], o["mean_i"], o["invstd_i"])
    L.check(fn(BF16, 0, RELUBWD, P(dzb), None, None, P(wpt), P(out.t), P(zrefb), P(o["sc_i"]), P(o["sh_i"]), P(o["mean_i"]),
               P(o["invstd_i"]), P(part.t), B, H, W, Cop, Cip, st()))
    torch.cuda.synchronize()
    frozen.verify("dgrad")
    g = out.verify("dgrad g")
    gr = full * on
    if fam == "exact":
        expect(entry, route, fam, "dgrad g", Fm.eq_bf16(g, gr))
    else:
        bound = Fm.bound_bf16(gr, S * on)
        ok = torch.where(either, Fm.within(g, full, Fm.bound_bf16(full, S)) | (g == 0), Fm.within(g, gr, bound))
        expect(entry, route, fam, "dgrad g", ok, torch.where(either, gr, g.to(F64)), gr, bound)
    s = part.verify("dgrad partial").to(F64).sum(0)
    zc = o["zref"].to(F64) - o["mean_i"].to(F64)
    inv = o["invstd_i"].to(F64)
    gs = g.to(F64)
    px = (0, 1, 2)
    if stat_source == "stored":
        expect_row(entry, route, fam, "dgrad sum g (of stored)", s[0], gs.sum(px), gs.abs().sum(px))
        expect_row(entry, route, fam, "dgrad sum g*xhat (of stored)", s[1], (gs * zc).sum(px) * inv, (gs * zc).abs().sum(px) * inv * 2.0)
    vals = Fm.rne(gr) if (stat_source == "stored" and fam == "exact") else gr
    if fam == "exact":
        e0 = e1 = None
    else:
        e = Fm.bound_bf16(gr, S * on) if stat_source == "stored" else Fm.bound_f32(S * on)
        e = e + torch.where(either, full.abs() + Fm.bound_bf16(full, S), torch.zeros_like(e))
        e0, e1 = e.sum(px), (e * zc.abs()).sum(px) * inv
    expect_row(entry, route, fam, "dgrad sum g", s[0], vals.sum(px), vals.abs().sum(px), e0)
    # (zref - mean is rounded once in fp32 before the multiply: twice the summation allowance covers it)
    expect_row(entry, route, fam, "dgrad sum g*xhat", s[1], (vals * zc).sum(px) * inv, (vals * zc).abs().sum(px) * inv * 2.0, e1)


# ---- weight gradient --------------------------------------------------------------------------------------------------------
WG_MODES = [("given", 0, 1), ("given", 1, 1), ("bn", 0, 1), ("pool", 1, 1), ("pool", 1, 2)]      # dz mode, prologue, pool


def dz_of(o, mode, pool, gkey="g", g2key="g2", zkey="z", sc="sc_o", sh="sh_o"):
    """(gsrc tensor name, float64 dz, M, either-branch elements with the size of the branch's step)"""
    def f():
        if mode == "given":
            return gkey, o[gkey].to(F64), None, None
        src = g2key if (mode == "pool" and pool == 2) else gkey
        if mode == "bn":
            dz, M = Fm.dz_ref(o[src], o[zkey], o["ca"], o["cb"], o["cc"])
            return src, dz, M, None
        dz, M = Fm.dz_ref(o[src], o[zkey], o["ca"], o["cb"], o["cc"], pool, o[sc], o[sh])
        step = None
        if o["family"] == "random":
            gup = Fm.upsample_pool(o[src], pool, o[zkey].shape[1], o[zkey].shape[2])
            step = torch.where(Fm.relu_either(o[zkey], o[sc], o[sh]), (o["ca"].to(F64) * gup).abs(), torch.zeros_like(dz))
        return src, dz, M, step
    return cached(o, ("dz", mode, pool, gkey), f)


def check_dz_out(entry, route, fam, tag, dzo, dz, M, step):
    if fam == "exact":
        expect(entry, route, fam, tag + " dz_out", Fm.eq_bf16(dzo, dz))
        return
    bound = Fm.bound_dz(dz, M)
    if step is not None:                        # the other ReLU branch on the either-branch elements: dz -+ ca*g
        assert float((step > 0).double().mean()) <= Fm.EITHER_SHARE
        d = (dzo.to(F64) - dz).abs()
        ok = (d <= bound) | ((step > 0) & ((d - step).abs() <= bound + Fm.half_ulp(step)))
    else:
        ok = Fm.within(dzo, dz, bound)
    shown = dzo.to(F64) if step is None else torch.where(step > 0, dz, dzo.to(F64))      # (the table's ratio: the settled elements)
    expect(entry, route, fam, tag + " dz_out", ok, shown, dz, bound)


def check_dw(L, entry, route, fam, tag, dwp, dwr, S, allow, Ci, Co, Cip, Cop, dw_u=None):
    """dwpack [9][Cinp][Coutp] (padded entries exactly 0) and the torch-layout dW of sed_unpack_conv_wgrad"""
    ref_p, S_p = Fm.to_pack_layout(dwr[:Co, :Ci], Cip, Cop), Fm.to_pack_layout(S[:Co, :Ci], Cip, Cop)
    got = dwp.view(9, Cip, Cop)
    if fam == "exact":
        assert Fm.exact_ok(float(S.max()))
        expect(entry, route, fam, tag + " dwpack", Fm.eq_f32(got, ref_p))
    else:
        bound = Fm.bound_f32(S_p, None if allow is None else Fm.to_pack_layout(allow[:Co, :Ci], Cip, Cop))
        expect(entry, route, fam, tag + " dwpack", Fm.within(got, ref_p, bound), got, ref_p, bound)
    un = Out((Co, Ci, 3, 3), torch.float32)
    L.check(L.lib().sed_unpack_conv_wgrad(L.ptr(dwp), L.ptr(un.t), Co, Ci, Cop, Cip, st()))
    torch.cuda.synchronize()
    unpacked = got.view(3, 3, Cip, Cop)[:, :, :Ci, :Co].permute(3, 2, 0, 1)
    assert torch.equal(un.verify(tag + " dW"), unpacked), f"{tag}: sed_unpack_conv_wgrad differs from the packed gradient"
    if dw_u is not None:
        assert torch.equal(dw_u, unpacked), f"{tag}: the fused launch's torch-layout dW differs from the packed gradient"
    if fam == "exact":
        expect(entry, route, fam, tag + " dW (unpacked)", Fm.eq_f32(un.t, dwr[:Co, :Ci]))


def check_wgrad(L, o, entry, route, anyw=False):
    B, H, W, Ci, Co = o["shape"]
    Cip, Cop, fam = o["Cip"], o["Cop"], o["family"]
    lib, P = L.lib(), L.ptr
    xb = cached(o, "xb", lambda: o["x"].to(BF))
    zb = cached(o, "zb", lambda: o["z"].to(BF))
    nws = lib.sed_conv_wgrad_ws_floats(B, H, W, Cip, Cop)
    for mode, pro, pool in (WG_MODES[:2] if anyw else WG_MODES):
        tag = f"wgrad dz={mode} p{pool} pro={pro}"
        a, flip = activation(o, pro)
        src, dz, M, step = dz_of(o, mode, pool)
        gb = cached(o, ("bf", src), lambda: o[src].to(BF))
        gp = P(gb) if gb.numel() else P(zb)              # (H = 1 under pool 2: the pooled tensor is empty, every row is the pooling floor's dropped row)
        ws = Out((nws,), torch.float32)
        ws.t.fill_(-5.0)
        dwp = Out((9 * Cip * Cop,), torch.float32)
        dzo = Out((B, H, W, Cop))
        ps, ph = (P(o["sc_i"]), P(o["sh_i"])) if pro else (None, None)
        frozen = Frozen(xb, gb, zb, o["sc_i"], o["sh_i"], o["sc_o"], o["sh_o"], o["ca"], o["cb"], o["cc"])
        if mode == "given":
            fn = lib.sed_conv3x3_wgrad_anyw if anyw else lib.sed_conv3x3_wgrad
            L.check(fn(BF16, pro, P(xb), ps, ph, P(gb), P(dwp.t), P(ws.t), B, H, W, Cip, Cop, st()))
        else:
            pooled = mode == "pool"
            L.check(lib.sed_conv3x3_wgrad_fused(BF16, pro, P(xb), ps, ph, DZ_POOL if pooled else DZ_BN, gp, P(zb),
                                                P(o["sc_o"]) if pooled else None, P(o["sh_o"]) if pooled else None, P(o["ca"]), P(o["cb"]),
                                                P(o["cc"]), pool, P(dzo.t), P(dwp.t), P(ws.t), B, H, W, Cip, Cop, st()))
        torch.cuda.synchronize()
        frozen.verify(tag)
        assert bool((ws.flat[:PAD] == CANARY).all()) and bool((ws.flat[PAD + nws:] == CANARY).all()), f"{tag}: workspace written past sed_conv_wgrad_ws_floats"
        dwt = dwp.verify(tag + " dwpack")
        if mode == "given":
            dzk = dz
        else:
            dzt = dzo.verify(tag + " dz_out")
            check_dz_out(entry, route, fam, tag, dzt, dz, M, step)
            dzk = dzt.to(F64)                            # the reference contracts the dz the kernel stored: its rounding does not enter
        key = ("dw", mode, pool, pro)
        if key in o["refs"] and not torch.equal(o["refs"][key][0], dzk):
            del o["refs"][key]                           # (another kernel form stored another dz: allowed on either-branch elements only, checked above)
        _, dwr, S, allow = cached(o, key, lambda: (dzk, Fm.wgrad_ref(a, dzk), Fm.wgrad_ref(a.abs(), dzk.abs()),
                                                   None if flip is None else Fm.wgrad_ref(flip, dzk.abs())))
        check_dw(L, entry, route, fam, tag, dwt, dwr, S, allow, Ci, Co, Cip, Cop)


# ---- cases ------------------------------------------------------------------------------------------------------------------
def _conv_cases():
    out = []
    for s in Fm.WGRAD_SHAPES:                  # shape-major: the cache holds one (shape, family) at a time
        for fam in FAMILIES:
            if s in Fm.CONV_SHAPES:
                Cip, Cop = Fm.pad32(s[3]), Fm.pad32(s[4])
                out += [(s, fam, "fwd", r) for r in ("", "l")] + ([(s, fam, "fwd", "w")] if Cop % 128 == 0 and Cip >= 64 else [])
                out += [(s, fam, "dgrad", r) for r in ("", "l")]
            out += [(s, fam, "wgrad", f) for f in WG_FORMS]
    return out


CONV_CASES = _conv_cases()


def _id(c):
    (B, H, W, Ci, Co), fam, kind, route = c
    return f"{B}x{H}x{W}_{Ci}-{Co}-{fam}-{kind}" + (f"-{route}" if route else "")


@pytest.mark.parametrize("case", CONV_CASES, ids=[_id(c) for c in CONV_CASES])
def test_conv_bf16_vs_float64(L, monkeypatch, case):
    """sed_conv3x3_fwd (prologue none / BN+ReLU x epilogue STATS / STORE / RELUBWD; the producer/consumer, LDS-weights and
    register-weights routes), sed_conv3x3_wgrad and sed_conv3x3_wgrad_fused (DZ_BN, DZ_POOL at pool 1 / 2, with dz_out; the default
    form -- the wide kernel where it covers the layer --, SED_WGRAD_WIDE=0, SED_WGRAD_KERNEL=2 / 3) on both operand families"""
    shape, fam, kind, route = case
    o = operands((shape, fam), lambda: Fm.draw_conv(shape, fam))
    lib = L.lib()
    with Routed(L, monkeypatch, WG_FORMS[route] if kind == "wgrad" else ROUTES[route]):
        if kind == "fwd":
            check_forward(L, o, "sed_conv3x3_fwd", route, lib.sed_conv3x3_fwd, STAT_SOURCE[route])
        elif kind == "dgrad":
            check_relubwd(L, o, "sed_conv3x3_fwd RELUBWD", route, lib.sed_conv3x3_fwd, "stored")
        else:
            check_wgrad(L, o, "sed_conv3x3_wgrad(_fused)", route)


@pytest.mark.parametrize("route", ["", "l", "w"])
def test_statistics_source_is_pinned(L, monkeypatch, route):
    """on an exact-family layer with |z| > 256 the sums of the accumulators and of the stored bf16 values differ, so the equality
    asserted by check_forward holds for one source only: the one the module's docstring states for the route"""
    shape = (2, 19, 8, 256, 128)
    o = operands((shape, "exact"), lambda: Fm.draw_conv(shape, "exact"))
    zr = Fm.conv_ref(activation(o, 0)[0], wd_of(o))
    assert float(zr.abs().max()) > 256 and not torch.equal(Fm.rne(zr).sum((0, 1, 2)), zr.sum((0, 1, 2)))
    with Routed(L, monkeypatch, ROUTES[route]):
        check_forward(L, o, "sed_conv3x3_fwd", route, L.lib().sed_conv3x3_fwd, STAT_SOURCE[route], pros=(0,))


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("shape", Fm.ANYW_SHAPES, ids=[f"W{s[2]}" for s in Fm.ANYW_SHAPES])
def test_any_width_entries_vs_float64(L, shape, fam):
    """sed_conv3x3_fwd_anyw (every prologue x epilogue pair) and sed_conv3x3_wgrad_anyw in bf16; W = 255 / 256: one row per
    weight-gradient tile"""
    assert shape[2] in Fm.ANYW_WIDTHS
    o = operands((shape, fam), lambda: Fm.draw_conv(shape, fam))
    lib = L.lib()
    check_forward(L, o, "sed_conv3x3_fwd_anyw", "", lib.sed_conv3x3_fwd_anyw, STAT_SOURCE["anyw"])
    check_relubwd(L, o, "sed_conv3x3_fwd_anyw RELUBWD", "", lib.sed_conv3x3_fwd_anyw, "acc")
    check_wgrad(L, o, "sed_conv3x3_wgrad_anyw", "", anyw=True)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("shape", Fm.COL_SHAPES, ids=[f"{s[0]}x{s[1]}_{s[3]}-{s[4]}" for s in Fm.COL_SHAPES])
def test_column_taps_entry_vs_float64(L, shape, fam):
    """sed_conv3x3_fwd_col (taps 1, 4, 7 only, W = 8) on weights whose side columns are zero: the float64 reference is the full 3x3
    convolution of those weights.  (Only the centre column is dense here: that is the entry point's contract.)"""
    o = operands((shape, fam, "col"), lambda: Fm.draw_conv(shape, fam))

    def wcol():
        wd = wd_of(o).clone()
        wd[:, :, :, 0] = 0
        wd[:, :, :, 2] = 0
        return wd
    cached(o, "wcol", wcol)
    check_forward(L, o, "sed_conv3x3_fwd_col", "", L.lib().sed_conv3x3_fwd_col, STAT_SOURCE["col"], wkey="wcol")


# ---- sed_conv3x3_dgrad_poolstats ---------------------------------------------------------------------------------------------
def pool_stats_rows(dy, y, cnt, scale, shift, mean, invstd):
    """the two rows from the STORED dy, the pooled activation y and the active-pixel counts: sum g = sum dy*cnt / 4;
    sum g*xhat = (sum dy*y - beta/4 * sum dy*cnt) / gamma, gamma = scale/invstd, beta = shift + mean*scale.  Returns
    (row 0, its magnitudes, row 1, its magnitudes)"""
    px = (0, 1, 2)
    d, yy, c = dy.to(F64), y.to(F64), cnt.to(F64)
    sc, is_ = scale.to(F64), invstd.to(F64)
    beta = shift.to(F64) + mean.to(F64) * sc
    s0, m0 = 0.25 * (d * c).sum(px), 0.25 * (d * c).abs().sum(px)
    k = (is_ / sc).abs()
    s1 = ((d * yy).sum(px) - 0.25 * beta * (d * c).sum(px)) * (is_ / sc)
    m1 = ((d * yy).abs().sum(px) + 0.25 * beta.abs() * (d * c).abs().sum(px)) * k * 4.0      # (beta, is/sc: a few fp32 roundings more)
    return s0, m0, s1, m1


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("B,H,W,Cd,Cc", Fm.POOLSTATS_SHAPES)
def test_dgrad_poolstats_vs_float64(L, B, H, W, Cd, Cc, fam):
    """dy = conv^T(dz) (stored bf16), the pooled activation and counts of sed_bn_relu_pool_cnt_fwd on a (2H+1) x 2W tensor (the odd
    row is dropped by the pooling floor), and the two statistics rows, which the kernel forms from the STORED dy"""
    lib, P = L.lib(), L.ptr
    shape = (B, H, W, Cc, Cd)                        # as a forward layer Cc -> Cd; the data gradient maps the Cd channels back to Cc
    o = operands((shape, fam, "ps"), lambda: Fm.draw_conv(shape, fam))
    Hz, Wz = 2 * H + 1, 2 * W
    zf = cached(o, "zfull", lambda: Fm.draw_pool_z(shape, fam).cuda())
    scale, shift, mean, invstd = o["sc_i"], o["sh_i"], o["mean_i"], o["invstd_i"]
    if fam == "random":
        scale = cached(o, "scale_neg", lambda: torch.cat([scale[:1], -scale[1:2], scale[2:]]))      # one negative gamma
    zfb = zf.to(BF)
    y, cnt = Out((B, H, W, Cc)), Out((B, H, W, Cc), torch.uint8, canary=77, fill=255)
    L.check(lib.sed_bn_relu_pool_cnt_fwd(BF16, P(zfb), P(scale), P(shift), P(y.t), P(cnt.t), B, Hz, Wz, Cc, st()))
    torch.cuda.synchronize()
    assert bool((cnt.verify("counts") <= 4).all()), "counts not written"
    yt = y.verify("pooled activation")
    act = Fm.bn_relu(zf, scale, shift)
    yr = Fm.avgpool_fwd(act)
    on = Fm.avgpool_fwd((Fm.gate_arg(zf, scale, shift)[0] > 0).to(F64)) * 4.0
    entry = "sed_conv3x3_dgrad_poolstats"
    if fam == "exact":
        expect(entry, "", fam, "pooled activation", Fm.eq_bf16(yt, yr))
        expect(entry, "", fam, "active-pixel counts", cnt.t.to(F64) == on)
    else:
        _, M = Fm.gate_arg(zf, scale, shift)
        bound = Fm.half_ulp(yr + Fm.DZ_ULPS * Fm.avgpool_fwd(M)) + Fm.DZ_ULPS * Fm.avgpool_fwd(M)      # four fp32 fma + their mean
        expect(entry, "", fam, "pooled activation", Fm.within(yt, yr, bound), yt, yr, bound)
        amb = Fm.avgpool_fwd(Fm.relu_either(zf, scale, shift).to(F64)) * 4.0
        assert float((amb > 0).double().mean()) <= Fm.EITHER_SHARE
        expect(entry, "", fam, "active-pixel counts", (cnt.t.to(F64) - on).abs() <= amb)
    wd = wd_of(o)                                    # [Cd][Cc][3][3]
    wpt = pack(L, o["w"], Cc, Cd, 1)
    dzb = o["dz"].to(BF)                             # [B][H][W][Cd]
    nparts = nparts_of(L, B, H, W)
    dy, part = Out((B, H, W, Cc)), Out((nparts, 2, Cc), torch.float32)
    flag = torch.zeros(1, device="cuda", dtype=torch.int32)
    frozen = Frozen(dzb, wpt, yt, cnt.t, scale, shift, mean, invstd)
    L.check(lib.sed_conv3x3_dgrad_poolstats(BF16, P(dzb), P(wpt), P(dy.t), P(yt), P(cnt.t), P(scale), P(shift), P(mean), P(invstd),
                                            P(part.t), nparts, P(flag), B, H, W, Cd, Cc, st()))
    torch.cuda.synchronize()
    frozen.verify(entry)
    assert int(flag.item()) == 0, "no channel here has |beta| > 8 |gamma|"
    wt = Fm.dgrad_w(wd)
    dyr, S = Fm.conv_ref(o["dz"].to(F64), wt), Fm.conv_ref(o["dz"].to(F64).abs(), wt.abs())
    dyt = dy.verify("dy")
    if fam == "exact":
        assert Fm.exact_ok(float(S.max()))
        expect(entry, "", fam, "dy", Fm.eq_bf16(dyt, dyr))
    else:
        bound = Fm.bound_bf16(dyr, S)
        expect(entry, "", fam, "dy", Fm.within(dyt, dyr, bound), dyt, dyr, bound)
    s = part.verify("partial").to(F64).sum(0)
    s0, m0, s1, m1 = pool_stats_rows(dyt, yt, cnt.t, scale, shift, mean, invstd)
    expect_row(entry, "", fam, "sum g (of stored dy)", s[0], s0, m0)
    expect_row(entry, "", fam, "sum g*xhat (of stored dy)", s[1], s1, m1)


# ---- sed_conv3x3_bwd_fused (dz exists only in LDS) ------------------------------------------------------------------------------
def ws_guard(L, B, H, W, Cip, Cop):
    n = L.lib().sed_conv_wgrad_ws_floats(B, H, W, Cip, Cop)
    ws = Out((n,), torch.float32)
    ws.t.fill_(-5.0)
    return ws, (lambda: bool((ws.flat[:PAD] == CANARY).all()) and bool((ws.flat[PAD + n:] == CANARY).all()))


def dz_flip(o, dz, M, step):
    """how far the kernel's bf16 dz may differ from rne(float64 dz): one ulp next to a rounding boundary, the ReLU branch's step on
    the either-branch elements (+ the rounding of the other branch)"""
    if o["family"] == "exact":
        return None
    f = torch.where(Fm.flip_mask(dz, Fm.DZ_ULPS * M), Fm.ulp_bf16(dz), torch.zeros_like(dz))
    if step is not None:
        f = f + torch.where(step > 0, step + Fm.ulp_bf16(step + dz.abs()), torch.zeros_like(dz))
    return f


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("W,Ci,Co", Fm.GEOM_C1)
@pytest.mark.parametrize("B,H,nwg", Fm.FUSED_CASES)
def test_bwd_fused_conv1_vs_float64(L, monkeypatch, B, H, nwg, W, Ci, Co, fam):
    """conv1 of a block: dz1 = ca*g + cb*z1 + cc (bf16, LDS only), dW1 = x (x) dz1, dx = conv1^T(dz1) stored in bf16, with
    SED_EPI_POOLSTATS (rows from the STORED dx, the pooled activation x and the counts) and SED_EPI_STORE"""
    lib, P = L.lib(), L.ptr
    shape = (B, H, W, Ci, Co)
    entry = "sed_conv3x3_bwd_fused conv1"
    o = operands((shape, fam, "bf1"), lambda: Fm.draw_conv(shape, fam))
    with Routed(L, monkeypatch, {} if nwg is None else {"SED_BWD_FUSED_BLOCKS": str(nwg)}):
        assert lib.sed_conv3x3_bwd_fused_supported(BF16, W, Ci, Co, DZ_BN, 0, POOLSTATS)
        x = cached(o, "xpos", lambda: o["x"].abs())                  # the pooled activation of the block before (>= 0)
        xb, zb, gb = x.to(BF), o["z"].to(BF), o["g"].to(BF)
        cnt = cached(o, "cnt", lambda: torch.randint(0, 5, (B, H, W, Ci), generator=torch.Generator().manual_seed(B * 57 + H)).to(torch.uint8).cuda())
        wd = wd_of(o)
        wpt = cached(o, "wpack_t", lambda: pack(L, o["w"], Ci, Co, 1))
        scale, shift, mean, invstd = o["sc_i"], o["sh_i"], o["mean_i"], o["invstd_i"]
        _, dz, M, _ = dz_of(o, "bn", 1)
        dzr = Fm.rne(dz)
        f = dz_flip(o, dz, M, None)
        a = x.to(F64)
        wt = Fm.dgrad_w(wd)
        dwr, S = Fm.wgrad_ref(a, dzr), Fm.wgrad_ref(a.abs(), dzr.abs())
        dxr, Sx = Fm.conv_ref(dzr, wt), Fm.conv_ref(dzr.abs(), wt.abs())
        allow_w = None if f is None else Fm.wgrad_ref(a.abs(), f)
        allow_x = None if f is None else Fm.conv_ref(f, wt.abs())
        nparts = nparts_of(L, B, H, W)
        for epi in (POOLSTATS, STORE):
            tag = f"epi={epi}"
            ws, ws_ok = ws_guard(L, B, H, W, Ci, Co)
            dwp, dw = Out((9 * Ci * Co,), torch.float32), Out((Co, Ci, 3, 3), torch.float32)
            dx, part = Out((B, H, W, Ci)), Out((nparts, 2, Ci), torch.float32)
            flag = torch.zeros(1, device="cuda", dtype=torch.int32)
            frozen = Frozen(xb, zb, gb, cnt, wpt, o["ca"], o["cb"], o["cc"], scale, shift, mean, invstd)
            e = bool(epi)
            L.check(lib.sed_conv3x3_bwd_fused(BF16, 0, P(xb), None, None, DZ_BN, P(gb), P(zb), None, None, P(o["ca"]), P(o["cb"]), P(o["cc"]), 1,
                                              P(wpt), P(dx.t), epi, P(xb) if e else None, P(cnt) if e else None, P(scale) if e else None,
                                              P(shift) if e else None, P(mean) if e else None, P(invstd) if e else None,
                                              P(part.t) if e else None, nparts, P(flag) if e else None, P(dwp.t), P(ws.t), B, H, W, Ci, Co,
                                              P(dw.t), Co, Ci, st()))
            torch.cuda.synchronize()
            frozen.verify(tag)
            assert ws_ok(), "slab written beyond sed_conv_wgrad_ws_floats()"
            check_dw(L, entry, "", fam, tag, dwp.verify(tag + " dwpack"), dwr, S, allow_w, Ci, Co, Ci, Co, dw.verify(tag + " dW"))
            dxt = dx.verify(tag + " dx")
            if fam == "exact":
                assert Fm.exact_ok(float(Sx.max()))
                expect(entry, "", fam, tag + " dx", Fm.eq_bf16(dxt, dxr))
            else:
                bound = Fm.bound_bf16(dxr, Sx, allow_x)
                expect(entry, "", fam, tag + " dx", Fm.within(dxt, dxr, bound), dxt, dxr, bound)
            if e:
                assert int(flag.item()) == 0
                s = part.verify(tag + " partial").to(F64).sum(0)
                s0, m0, s1, m1 = pool_stats_rows(dxt, xb, cnt, scale, shift, mean, invstd)
                expect_row(entry, "", fam, "sum g (of stored dx)", s[0], s0, m0)
                expect_row(entry, "", fam, "sum g*xhat (of stored dx)", s[1], s1, m1)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("agate", ["1", "0"])
@pytest.mark.parametrize("W,Cc,Cq,pool", Fm.GEOM_C2)
@pytest.mark.parametrize("B,H,nwg", Fm.FUSED_CASES)
def test_bwd_fused_conv2_vs_float64(L, monkeypatch, B, H, nwg, W, Cc, Cq, pool, agate, fam):
    """conv2 of a block: a1 = relu(bn1(z1)) rebuilt on load, dz2 = BN2 / ReLU / avg-pool backward of (dy, z2) (bf16, LDS only),
    dW2 = a1 (x) dz2, g1 = relu'(bn1(z1)) * conv2^T(dz2) stored in bf16, rows sum g1 and sum g1*xhat1 from the STORED g1.
    H = 1: the pooled tensor is empty, every dz row is the pooling floor's dropped row."""
    lib, P = L.lib(), L.ptr
    shape = (B, H, W, Cc, Cc)
    entry = "sed_conv3x3_bwd_fused conv2"
    route = "" if agate == "1" else "agate0"
    o = operands((shape, fam, "bf2"), lambda: Fm.draw_conv(shape, fam))
    env = {"SED_BF_AGATE": agate}
    if nwg is not None:
        env["SED_BWD_FUSED_BLOCKS"] = str(nwg)
    with Routed(L, monkeypatch, env):
        assert lib.sed_conv3x3_bwd_fused_supported_pool(BF16, W, Cc, Cc, DZ_POOL, 1, RELUBWD, pool)
        z1b, z2b = cached(o, "xb", lambda: o["x"].to(BF)), cached(o, "zb", lambda: o["z"].to(BF))
        dyb = cached(o, ("bf", "g2"), lambda: o["g2"].to(BF))
        sc1, sh1, mean1, invstd1 = o["sc_i"], o["sh_i"], o["mean_i"], o["invstd_i"]
        wd = wd_of(o)
        wpt = cached(o, "wpack_t", lambda: pack(L, o["w"], Cc, Cc, 1))
        a1, flip_a = activation(o, 1)
        _, dz, M, step = dz_of(o, "pool", pool)
        dzr = Fm.rne(dz)
        f = dz_flip(o, dz, M, step)
        wt = Fm.dgrad_w(wd)
        arg1, _ = Fm.gate_arg(o["x"], sc1, sh1)
        on = arg1 > 0
        either = Fm.relu_either(o["x"], sc1, sh1) if fam == "random" else torch.zeros_like(on)
        dwr, S = Fm.wgrad_ref(a1, dzr), Fm.wgrad_ref(a1.abs(), dzr.abs())
        full, Sg = Fm.conv_ref(dzr, wt), Fm.conv_ref(dzr.abs(), wt.abs())
        allow_w = allow_g = None
        if fam == "random":
            allow_w = Fm.wgrad_ref(a1.abs(), f) + Fm.wgrad_ref(flip_a, dzr.abs() + f)
            allow_g = Fm.conv_ref(f, wt.abs())
            assert float(either.double().mean()) <= Fm.EITHER_SHARE and float((step > 0).double().mean()) <= Fm.EITHER_SHARE
        nparts = nparts_of(L, B, H, W)
        ws, ws_ok = ws_guard(L, B, H, W, Cc, Cc)
        dwp, dw = Out((9 * Cc * Cc,), torch.float32), Out((Cc, Cc, 3, 3), torch.float32)
        g1, part = Out((B, H, W, Cc)), Out((nparts, 2, Cc), torch.float32)
        frozen = Frozen(z1b, z2b, dyb, wpt, sc1, sh1, mean1, invstd1, o["sc_o"], o["sh_o"], o["ca"], o["cb"], o["cc"])
        dyp = P(dyb) if dyb.numel() else P(z2b)
        L.check(lib.sed_conv3x3_bwd_fused(BF16, 1, P(z1b), P(sc1), P(sh1), DZ_POOL, dyp, P(z2b), P(o["sc_o"]), P(o["sh_o"]), P(o["ca"]), P(o["cb"]),
                                          P(o["cc"]), pool, P(wpt), P(g1.t), RELUBWD, P(z1b), None, P(sc1), P(sh1), P(mean1), P(invstd1),
                                          P(part.t), nparts, None, P(dwp.t), P(ws.t), B, H, W, Cc, Cc, P(dw.t), Cc, Cc, st()))
        torch.cuda.synchronize()
        frozen.verify(entry)
        assert ws_ok(), "slab written beyond sed_conv_wgrad_ws_floats()"
        check_dw(L, entry, route, fam, "conv2", dwp.verify("dwpack"), dwr, S, allow_w, Cc, Cc, Cc, Cc, dw.verify("dW"))
        gt = g1.verify("g1")
        gr = full * on
        if fam == "exact":
            assert Fm.exact_ok(float(Sg.max()))
            expect(entry, route, fam, "g1", Fm.eq_bf16(gt, gr))
        else:
            bound = Fm.bound_bf16(gr, Sg * on, allow_g * on)
            ok = torch.where(either, Fm.within(gt, full, Fm.bound_bf16(full, Sg, allow_g)) | (gt == 0), Fm.within(gt, gr, bound))
            expect(entry, route, fam, "g1", ok, torch.where(either, gr, gt.to(F64)), gr, bound)
        s = part.verify("partial").to(F64).sum(0)
        gs, px = gt.to(F64), (0, 1, 2)
        zc, inv = o["x"].to(F64) - mean1.to(F64), invstd1.to(F64)
        expect_row(entry, route, fam, "sum g1 (of stored)", s[0], gs.sum(px), gs.abs().sum(px))
        # sum g*z1 in fp32, the mean taken off once per workgroup: magnitudes of both terms
        mags = ((gs * o["x"].to(F64)).abs().sum(px) + mean1.to(F64).abs() * gs.abs().sum(px)) * inv * 2.0
        expect_row(entry, route, fam, "sum g1*xhat (of stored)", s[1], (gs * zc).sum(px) * inv, mags)


# ---- block 0, C1 mode -----------------------------------------------------------------------------------------------------------
def c1_refs(o):
    def f():
        a1, pre, S, xz = Fm.c1_activation(o["x1"], o["fmean"], o["fstd"], o["w1"], o["sc1"], o["sh1"])
        if o["family"] == "exact":
            return a1, pre, xz, None, torch.zeros_like(pre, dtype=torch.bool)
        margin = Fm.C * S                                # the accumulator's own gate: one fp32 MFMA chain of 9 products + the shift
        un = torch.relu(pre)
        flip = torch.where(Fm.flip_mask(un, margin), Fm.ulp_bf16(un), torch.zeros_like(un)) + torch.where(pre.abs() <= margin, margin, torch.zeros_like(un))
        return a1, pre, xz, flip, pre.abs() <= margin
    return cached(o, "c1", f)


def mask_words(on):
    """[B][H][W][32] bool -> the relu_mask words [B][H][W][2] int16: channel c <-> half (c >> 2) & 1, bit (c & 3) + 4*(c >> 3)"""
    c = torch.arange(32, device=on.device)
    half, bit = (c >> 2) & 1, (c & 3) + 4 * (c >> 3)
    v = on.to(torch.int32) << bit
    w = torch.stack([(v * (half == h)).sum(-1) for h in (0, 1)], -1)
    return torch.where(w >= 32768, w - 65536, w).to(torch.int16)


def mask_bits(mask):
    mk = mask.to(torch.int32) & 0xFFFF
    c = torch.arange(32, device=mask.device)
    half, bit = (c >> 2) & 1, (c & 3) + 4 * (c >> 3)
    return ((mk[..., half] >> bit) & 1).bool()


def c1_args(L, o):
    P = L.ptr
    return P(o["x1"]), P(o["fmean"]), P(o["fstd"]), P(o["w1"]), P(o["sc1"]), P(o["sh1"])


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("B,H", Fm.BLOCK0)
def test_block0_forward_c1_vs_float64(L, B, H, fam):
    """sed_conv3x3_fwd_c1: conv2 of block 0 on the activation rebuilt from x1 (STATS and STORE), the ReLU-decision mask, the rows
    from the STORED z2"""
    lib, P = L.lib(), L.ptr
    W, Cc = 64, 32
    entry = "sed_conv3x3_fwd_c1"
    assert lib.sed_c1_mode_supported(BF16, W, Cc, Cc)
    o = operands((B, H, fam, "c1"), lambda: Fm.draw_c1(B, H, fam))
    a1, pre, xz, flip, either = c1_refs(o)
    w2 = o["w2"].to(F64)
    wp = cached(o, "wpack", lambda: pack(L, o["w2"], Cc, Cc, 0))
    zr, S = Fm.conv_ref(a1, w2), Fm.conv_ref(a1.abs(), w2.abs())
    allow = None if flip is None else Fm.conv_ref(flip, w2.abs())
    nparts = nparts_of(L, B, H, W)
    for epi in (STATS, STORE):
        tag = f"epi={epi}"
        z, part = Out((B, H, W, Cc)), Out((nparts, 2, Cc), torch.float32)
        mask = Out((B, H, W, 2), torch.int16, canary=-7, fill=0)
        frozen = Frozen(o["x1"], o["fmean"], o["fstd"], o["w1"], o["sc1"], o["sh1"], wp)
        L.check(lib.sed_conv3x3_fwd_c1(BF16, epi, *c1_args(L, o), P(wp), P(z.t), P(part.t) if epi else None, P(mask.t) if epi else None,
                                       B, H, W, Cc, st()))
        torch.cuda.synchronize()
        frozen.verify(tag)
        zt = z.verify(tag + " z2")
        if fam == "exact":
            assert Fm.exact_ok(float(S.max()), *Fm.exact_bounds_c1(B, H).values())
            expect(entry, "", fam, tag + " z2", Fm.eq_bf16(zt, zr))
        else:
            assert float(either.double().mean()) <= Fm.EITHER_SHARE
            bound = Fm.bound_bf16(zr, S, allow)
            expect(entry, "", fam, tag + " z2", Fm.within(zt, zr, bound), zt, zr, bound)
        if not epi:
            continue
        expect(entry, "", fam, "relu mask", (mask_bits(mask.verify("relu mask")) == (pre > 0)) | either)
        s = part.verify("partial").to(F64).sum(0)
        zs, px = zt.to(F64), (0, 1, 2)
        expect_row(entry, "", fam, "sum z2 (of stored)", s[0], zs.sum(px), zs.abs().sum(px))
        expect_row(entry, "", fam, "sum z2^2 (of stored)", s[1], (zs * zs).sum(px), (zs * zs).sum(px))
        vals = Fm.rne(zr) if fam == "exact" else zr
        e = None if fam == "exact" else Fm.bound_bf16(zr, S, allow)
        expect_row(entry, "", fam, "sum z2", s[0], vals.sum(px), vals.abs().sum(px), None if e is None else e.sum(px))
        expect_row(entry, "", fam, "sum z2^2", s[1], (vals * vals).sum(px), (vals * vals).sum(px),
                   None if e is None else Fm.square_bound(zr, e).sum(px))


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("B,H", Fm.BLOCK0)
def test_block0_weight_gradient_c1_vs_float64(L, B, H, fam):
    """sed_conv3x3_wgrad_fused_c1: dz2 = BN2 / ReLU / avg-pool backward of (dy, z2) written to dz_out, dW2 = a1 (x) dz2 with a1 rebuilt
    from x1; the reference contracts the dz_out the kernel stored"""
    lib, P = L.lib(), L.ptr
    W, Cc = 64, 32
    entry = "sed_conv3x3_wgrad_fused_c1"
    o = operands((B, H, fam, "c1"), lambda: Fm.draw_c1(B, H, fam))
    a1, pre, xz, flip, either = c1_refs(o)
    _, dz, M, step = dz_of(o, "pool", 2, gkey="dy", g2key="dy", zkey="z2", sc="sc2", sh="sh2")
    z2b, dyb = cached(o, "z2b", lambda: o["z2"].to(BF)), cached(o, "dyb", lambda: o["dy"].to(BF))
    ws, ws_ok = ws_guard(L, B, H, W, Cc, Cc)
    dwp, dzo = Out((9 * Cc * Cc,), torch.float32), Out((B, H, W, Cc))
    frozen = Frozen(o["x1"], o["fmean"], o["fstd"], o["w1"], o["sc1"], o["sh1"], z2b, dyb, o["sc2"], o["sh2"], o["ca"], o["cb"], o["cc"])
    L.check(lib.sed_conv3x3_wgrad_fused_c1(BF16, *c1_args(L, o), P(dyb) if dyb.numel() else P(z2b), P(z2b), P(o["sc2"]), P(o["sh2"]), P(o["ca"]), P(o["cb"]), P(o["cc"]), 2,
                                           P(dzo.t), P(dwp.t), P(ws.t), B, H, W, Cc, st()))
    torch.cuda.synchronize()
    frozen.verify(entry)
    assert ws_ok(), "workspace written past sed_conv_wgrad_ws_floats"
    dzt = dzo.verify("dz_out")
    check_dz_out(entry, "", fam, "c1", dzt, dz, M, step)
    dzk = dzt.to(F64)
    dwr, S = Fm.wgrad_ref(a1, dzk), Fm.wgrad_ref(a1.abs(), dzk.abs())
    allow = None if flip is None else Fm.wgrad_ref(flip, dzk.abs())
    check_dw(L, entry, "", fam, "c1", dwp.verify("dwpack"), dwr, S, allow, Cc, Cc, Cc, Cc)


def a_rows_check(entry, route, fam, what, part, g_used, xz, elem=None):
    """[A; sum g] summed over the partial rows against the rows of the bf16 g the matrix pipe contracts"""
    got = part.to(F64).sum(0)
    ref = Fm.c1_a_rows(g_used, xz)
    mags = Fm.c1_a_rows(g_used.abs(), xz.abs())
    mags[9] = g_used.abs().sum((0, 1, 2))
    if fam == "exact":
        assert Fm.exact_ok(float(mags.max()))
        expect(entry, route, fam, what, Fm.eq_f32(got, ref))
    else:
        bound = Fm.C * mags + (elem if elem is not None else 0.0)
        expect(entry, route, fam, what, Fm.within(got, ref, bound), got, ref, bound)


@pytest.mark.parametrize("th", ["8", "4"])
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("B,H", Fm.BLOCK0)
def test_block0_data_gradient_c1_vs_float64(L, monkeypatch, B, H, fam, th):
    """sed_conv3x3_dgrad_c1 (g stored, row sum g), sed_conv3x3_dgrad_c1_stats and its test hook _stats_g ([A; sum g] rows, g stored):
    g = conv2^T(dz) gated by conv1's ReLU decisions -- here the float64 decisions of the rebuilt activation, handed over as the
    relu_mask.  The [A; sum g] rows contract the bf16-ROUNDED g: their reference is formed from the g the hook stored, which is
    itself checked per element."""
    lib, P = L.lib(), L.ptr
    W, Cc = 64, 32
    o = operands((B, H, fam, "c1"), lambda: Fm.draw_c1(B, H, fam))
    a1, pre, xz, flip, either = c1_refs(o)
    on = pre > 0
    mask = cached(o, "mask", lambda: mask_words(on))
    assert torch.equal(mask_bits(mask), on)
    w2 = o["w2"].to(F64)
    wt = Fm.dgrad_w(w2)
    wpt = cached(o, "wpack_t", lambda: pack(L, o["w2"], Cc, Cc, 1))
    dzb = cached(o, "dzb", lambda: o["dz"].to(BF))
    full, S = Fm.conv_ref(o["dz"].to(F64), wt), Fm.conv_ref(o["dz"].to(F64).abs(), wt.abs())
    gr, Sg = full * on, S * on
    if fam == "exact":
        assert Fm.exact_ok(float(S.max()))
    route = "" if th == "8" else "th4"
    with Routed(L, monkeypatch, {"SED_DGRAD_TH": th}):
        frozen = Frozen(dzb, wpt, mask, o["x1"], o["fmean"], o["fstd"])
        # the unfused kernel
        np2 = nparts_of(L, B, H, W)
        g0, part0 = Out((B, H, W, Cc)), Out((np2, 2, Cc), torch.float32)
        part0.t.zero_()                                  # (row 1 is not this kernel's to write)
        L.check(lib.sed_conv3x3_dgrad_c1(BF16, P(dzb), P(wpt), P(g0.t), P(mask), P(part0.t), B, H, W, Cc, st()))
        # the fused kernel and its hook
        npc = lib.sed_conv_dgrad_c1_nparts()
        part, part_g, g1 = Out((npc, 10, Cc), torch.float32), Out((npc, 10, Cc), torch.float32), Out((B, H, W, Cc))
        L.check(lib.sed_conv3x3_dgrad_c1_stats(BF16, P(dzb), P(wpt), P(o["x1"]), P(o["fmean"]), P(o["fstd"]), P(mask), P(part.t), B, H, W, st()))
        L.check(lib.sed_conv3x3_dgrad_c1_stats_g(BF16, P(dzb), P(wpt), P(o["x1"]), P(o["fmean"]), P(o["fstd"]), P(mask), P(part_g.t), P(g1.t),
                                                 B, H, W, st()))
        torch.cuda.synchronize()
        frozen.verify("dgrad_c1")
    for entry, gt in (("sed_conv3x3_dgrad_c1", g0.verify("g")), ("sed_conv3x3_dgrad_c1_stats_g", g1.verify("g_out"))):
        if fam == "exact":
            expect(entry, route, fam, "g", Fm.eq_bf16(gt, gr))
        else:
            bound = Fm.bound_bf16(gr, Sg)
            expect(entry, route, fam, "g", Fm.within(gt, gr, bound), gt, gr, bound)
    gs = g0.t.to(F64)
    s0 = part0.verify("partial")[:, 0].to(F64).sum(0)
    expect_row("sed_conv3x3_dgrad_c1", route, fam, "sum g (of stored)", s0, gs.sum((0, 1, 2)), gs.abs().sum((0, 1, 2)))
    pt, pg = part.verify("a_partial"), part_g.verify("a_partial (hook)")
    assert torch.equal(pt, pg), "the hook's statistics differ from the plain launch's"
    a_rows_check("sed_conv3x3_dgrad_c1_stats", route, fam, "[A; sum g] (of the hook's g)", pt, g1.t.to(F64), xz)
    a_rows_check("sed_conv3x3_dgrad_c1_stats_g", route, fam, "[A; sum g] (of its g)", pg, g1.t.to(F64), xz)
    if fam == "exact":                                   # and against the float64 g itself, rounded as the matrix pipe's operand
        a_rows_check("sed_conv3x3_dgrad_c1_stats", route, fam, "[A; sum g]", pt, Fm.rne(gr), xz)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("B,H", Fm.BLOCK0)
def test_block0_bwd_fused_c1_vs_float64(L, B, H, fam):
    """sed_conv3x3_bwd_fused_c1 (relu_mask NULL: gated with the activation tile it rebuilds): dW2 = a1 (x) dz2 and the [A; sum g] rows of
    g = [a1 > 0] * conv2^T(dz2), dz2 (bf16) and g (bf16, the matrix pipe's operand) existing only inside the kernel.  Random family:
    dz2 next to a rounding boundary or a BN2-ReLU either-branch element, g next to a rounding boundary and conv1's either-branch
    decisions enter the rows' gate as per-element allowances (tests/conv_bf16_formula.py)."""
    lib, P = L.lib(), L.ptr
    W, Cc = 64, 32
    entry = "sed_conv3x3_bwd_fused_c1"
    assert lib.sed_conv3x3_bwd_fused_c1_supported(BF16, W, Cc, 2)
    o = operands((B, H, fam, "c1"), lambda: Fm.draw_c1(B, H, fam))
    a1, pre, xz, flip_a, either1 = c1_refs(o)
    on = pre > 0
    _, dz, M, step = dz_of(o, "pool", 2, gkey="dy", g2key="dy", zkey="z2", sc="sc2", sh="sh2")
    dzr = Fm.rne(dz)
    f = dz_flip(o, dz, M, step)
    w2 = o["w2"].to(F64)
    wt = Fm.dgrad_w(w2)
    wpt = cached(o, "wpack_t", lambda: pack(L, o["w2"], Cc, Cc, 1))
    z2b, dyb = cached(o, "z2b", lambda: o["z2"].to(BF)), cached(o, "dyb", lambda: o["dy"].to(BF))
    dwr, S = Fm.wgrad_ref(a1, dzr), Fm.wgrad_ref(a1.abs(), dzr.abs())
    full, Sg = Fm.conv_ref(dzr, wt), Fm.conv_ref(dzr.abs(), wt.abs())
    gr = Fm.rne(full * on)
    allow_w = elem = None
    if fam == "random":
        allow_w = Fm.wgrad_ref(a1.abs(), f) + Fm.wgrad_ref(flip_a, dzr.abs() + f)
        acc = Fm.C * Sg + Fm.conv_ref(f, wt.abs())                      # how far the kernel's fp32 g may lie from the float64 one
        eg = acc + torch.where(Fm.flip_mask(full, acc), Fm.ulp_bf16(full), torch.zeros_like(full))
        eg = torch.where(either1, full.abs() + eg + Fm.ulp_bf16(full), eg * on)
        elem = Fm.c1_a_rows(eg, xz.abs())
        elem[9] = eg.sum((0, 1, 2))
    npc = lib.sed_conv_dgrad_c1_nparts()
    part = Out((npc, 10, Cc), torch.float32)
    ws, ws_ok = ws_guard(L, B, H, W, Cc, Cc)
    dwp, dw = Out((9 * Cc * Cc,), torch.float32), Out((Cc, Cc, 3, 3), torch.float32)
    frozen = Frozen(o["x1"], o["fmean"], o["fstd"], o["w1"], o["sc1"], o["sh1"], z2b, dyb, wpt, o["sc2"], o["sh2"], o["ca"], o["cb"], o["cc"])
    dyp = P(dyb) if dyb.numel() else P(z2b)
    L.check(lib.sed_conv3x3_bwd_fused_c1(BF16, *c1_args(L, o), dyp, P(z2b), P(o["sc2"]), P(o["sh2"]), P(o["ca"]), P(o["cb"]), P(o["cc"]), 2, P(wpt),
                                         None, P(part.t), P(dwp.t), P(ws.t), B, H, W, Cc, P(dw.t), Cc, Cc, st()))
    torch.cuda.synchronize()
    frozen.verify(entry)
    assert ws_ok(), "slab written beyond sed_conv_wgrad_ws_floats()"
    check_dw(L, entry, "", fam, "dW2", dwp.verify("dwpack"), dwr, S, allow_w, Cc, Cc, Cc, Cc, dw.verify("dW"))
    a_rows_check(entry, "", fam, "[A; sum g]", part.verify("a_partial"), gr, xz, elem)
