"""GPU: the launches of csrc/sed_convmod.hip through the C ABI, per element against the float64 definition in
tests/convmod_formula.py, within the gates derived in that file's docstring.

Shapes: k in {3, 7, 31} x C in {4, 32, 96, 160} (one test each), and inside a test every t in {1, 2, p, k - 1, k, TILE - 1, TILE, TILE + 1,
2 TILE + 3} with B alternating between 2 and 3, so that clip boundaries fall inside and at the edges of a tile; TILE is asked of the
library.  Two operand families: exact integers (z, dv and the filter gradients equal float64 bit for bit) and Gaussian operands within
the gates.  Every input lies between NaN regions (a read of a neighbouring buffer poisons an output), every output in a NaN-filled
buffer between canary regions.  Run with -s for the worst error / gate of every check."""
import importlib

import numpy as np
import pytest
import torch

import convmod_formula as V

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
GUARD = 1024
CANARY = -1024.0
KS = [3, 7, 31]
CS = [4, 32, 96, 160]
BN_EPS, BN_MOM = 1e-5, 0.1
RED_ROWS = 128      # rows a workgroup of sed_bn_silu_bwd_reduce owns (include/sed_hip.h), checked against the part count below


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


def npy(t):
    return t.detach().cpu().numpy()


def ok(got, ref, gate, tag):
    good, worst = V.check(got, ref, gate, tag)
    assert good, (tag, worst)


def shapes(L, k):
    """(B, t) for every frame count of the list, B alternating between 2 and 3"""
    tile, p = L.lib().sed_dwconv_tile(), (k - 1) // 2
    ts = sorted({1, 2, p, k - 1, k, tile - 1, tile, tile + 1, 2 * tile + 3})
    return tile, [(2 + i % 2, t) for i, t in enumerate(ts)]


def run_fwd(L, g, w, bias, B, t, C, k, tag):
    """training form, eval form, training form again -> (z, v, partial [nparts][2][C]) as numpy after the canary / repeat checks"""
    lib, P = L.lib(), L.ptr
    R = B * t
    nparts = lib.sed_dwconv_nparts(B, t)
    assert nparts == B * -(-t // lib.sed_dwconv_tile()) and lib.sed_dwconv_glu_fwd_ws_floats(B, t, C) == nparts * 2 * C
    b = Bufs()
    host = (g, w, bias)
    dev = [b.inp(a) for a in host]
    z, v, part = b.out(R, C), b.out(R, C), b.out(nparts, 2, C)
    z2, z3, v3, part3 = b.out(R, C), b.out(R, C), b.out(R, C), b.out(nparts, 2, C)
    for zz, vv, pp in ((z, v, part), (z2, None, None), (z3, v3, part3)):
        L.check(lib.sed_dwconv_glu_fwd(*(P(a) for a in dev), P(zz), P(vv) if vv is not None else None, P(pp) if pp is not None else None,
                                       B, t, C, k, stream()), "dwconv_glu_fwd")
    b.intact()
    for d, hv in zip(dev, host):
        assert np.array_equal(npy(d), hv), "an input was modified"
    assert np.array_equal(bits(z), bits(z2)), (tag, "the eval form (NULL v, NULL partials) changed z")
    assert np.array_equal(bits(z), bits(z3)) and np.array_equal(bits(v), bits(v3)) and np.array_equal(bits(part), bits(part3)), (tag, "two runs differ")
    assert not np.isnan(npy(part)).any(), (tag, "a partial row was left unwritten")
    return npy(z), npy(v), npy(part)


def run_bwd(L, gz, z, ca, cb, cc, v, g, w, B, t, C, k, tag):
    """twice -> (dg, dw, dbias) as numpy"""
    lib, P = L.lib(), L.ptr
    R = B * t
    b = Bufs()
    host = (gz, z, ca, cb, cc, v, g, w)
    dev = [b.inp(a) for a in host]
    nws = lib.sed_dwconv_glu_bwd_ws_floats(B, t, C, k)
    assert nws == lib.sed_dwconv_nparts(B, t) * (k + 1) * C
    outs = []
    for _ in range(2):
        dg, dw, db, ws = b.out(R, 2 * C), b.out(C, k), b.out(C), b.out(nws)
        L.check(lib.sed_dwconv_glu_bwd(*(P(a) for a in dev), P(dg), P(dw), P(db), P(ws), B, t, C, k, stream()), "dwconv_glu_bwd")
        outs.append((dg, dw, db))
    b.intact()
    for d, hv in zip(dev, host):
        assert np.array_equal(npy(d), hv), "an input was modified"
    for a, c in zip(*outs):
        assert np.array_equal(bits(a), bits(c)), (tag, "two runs differ")
    return tuple(npy(a) for a in outs[0])


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("k", KS)
def test_exact_integer_family(L, k, C):
    tile, cases = shapes(L, k)
    for B, t in cases:
        case = V.exact_case(np.random.default_rng(1000 * k + 10 * C + t), B, t, C, k)
        tag = (k, C, B, t)
        z, v, part = run_fwd(L, case["g"], case["w"], case["bias"], B, t, C, k, tag)
        rv = V.glu(case["g"])
        rz = V.dwconv(rv, case["w"], case["bias"], B, t)
        assert np.array_equal(v.astype(np.float64), rv), (tag, "v is not exact")
        assert np.array_equal(z.astype(np.float64), rz), (tag, "z is not exact: a halo, tap-order or bias error")
        assert np.array_equal(part.astype(np.float64).sum(axis=0), np.stack([rz.sum(axis=0), (rz * rz).sum(axis=0)])), (tag, "statistics")
        dz = case["ca"].astype(np.float64) * case["gz"] + case["cb"].astype(np.float64) * case["z"] + case["cc"]
        rdv, rdw, rdb = V.dwconv_bwd(dz, case["v"], case["w"], B, t)
        dg, dw, db = run_bwd(L, case["gz"], case["z"], case["ca"], case["cb"], case["cc"], case["v"], case["g"], case["w"], B, t, C, k, tag)
        assert np.array_equal(dg[:, :C].astype(np.float64), rdv), (tag, "dv is not exact: the transposed convolution")
        assert not dg[:, C:].any(), (tag, "the gate half's gradient is not exactly zero at sigma = 1")
        assert np.array_equal(dw.astype(np.float64), rdw), (tag, "the filter gradient is not exact")
        assert np.array_equal(db.astype(np.float64), rdb), (tag, "the bias gradient is not exact")


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("k", KS)
def test_gaussian_family(L, k, C):
    lib, P = L.lib(), L.ptr
    tile, cases = shapes(L, k)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    for B, t in cases:
        R = B * t
        case = V.gaussian_case(np.random.default_rng(2000 * k + 10 * C + t), B, t, C, k)
        g, w, bias = case["g"], case["w"], case["bias"]
        tag = (k, C, B, t)
        # ---- sed_dwconv_glu_fwd, and the existing finalisation on the kernel's own partial rows
        z, v, part = run_fwd(L, g, w, bias, B, t, C, k, tag)
        rv = V.glu(g)
        rz = V.dwconv(rv, w, bias, B, t)
        fg = V.fwd_gates(g, w, bias, B, t, tile)
        ok(v, rv, fg["v"], tag + ("v",))
        ok(z, rz, fg["z"], tag + ("z",))
        sums = part.astype(np.float64).sum(axis=0)
        ok(sums[0], rz.sum(axis=0), fg["sum"], tag + ("sum z",))
        ok(sums[1], (rz * rz).sum(axis=0), fg["sumsq"], tag + ("sum z^2",))
        b = Bufs()
        dpart, gam, bet = b.inp(part), b.inp(case["gamma"]), b.inp(case["beta"])
        rm, rvv = b.out(C), b.out(C)
        rm.copy_(torch.from_numpy(case["rmean"]))
        rvv.copy_(torch.from_numpy(case["rvar"]))
        scale, shift, mean, invstd = b.out(C), b.out(C), b.out(C), b.out(C)
        L.check(lib.sed_bn_train_finalize(P(dpart), part.shape[0], float(R), P(gam), P(bet), P(rm), P(rvv), BN_MOM, BN_EPS, P(scale), P(shift),
                                          P(mean), P(invstd), C, C, stream()), "bn_train_finalize")
        b.intact()
        bn = V.bn_coeffs(rz, case["gamma"], case["beta"], case["rmean"], case["rvar"], True)
        fin = V.finalize_gates(rz, fg["z"], case["gamma"], case["beta"], case["rmean"], case["rvar"], tile)
        for name, got in (("scale", scale), ("shift", shift), ("mean", mean), ("invstd", invstd), ("running_mean", rm), ("running_var", rvv)):
            if R > 1 or not name.startswith("running"):
                ok(npy(got), bn[name], fin[name], tag + (name,))
        # ---- sed_bn_silu_fwd on the reference's z and coefficients rounded to fp32
        z32, sc, sh, mu, inv = f32(rz), f32(bn["scale"]), f32(bn["shift"]), f32(bn["mean"]), f32(bn["invstd"])
        dz32, dsc, dsh, dmu, dinv, dds = (b.inp(a) for a in (z32, sc, sh, mu, inv, case["ds"]))
        s, s2 = b.out(R, C), b.out(R, C)
        for ss in (s, s2):
            L.check(lib.sed_bn_silu_fwd(P(dz32), P(dsc), P(dsh), P(ss), R, C, stream()), "bn_silu_fwd")
        b.intact()
        assert np.array_equal(bits(s), bits(s2)), (tag, "bn_silu_fwd: two runs differ")
        ok(npy(s), V.bn_silu(z32, sc, sh)[1], V.bn_silu_gates(z32, sc, sh)["s"], tag + ("s",))
        # ---- sed_bn_silu_bwd_reduce, plain, again, and with gz over ds
        nbp = lib.sed_bn_silu_bwd_nparts(R)
        assert nbp == -(-R // RED_ROWS)
        gz, bp, gz2, bp2, gz3, bp3 = b.out(R, C), b.out(nbp, 2, C), b.out(R, C), b.out(nbp, 2, C), b.out(R, C), b.out(nbp, 2, C)
        gz3.copy_(torch.from_numpy(case["ds"]))
        for src, gg, pp in ((dds, gz, bp), (dds, gz2, bp2), (gz3, gz3, bp3)):
            L.check(lib.sed_bn_silu_bwd_reduce(P(src), P(dz32), P(dsc), P(dsh), P(dmu), P(dinv), P(gg), P(pp), R, C, stream()), "bn_silu_bwd_reduce")
        b.intact()
        for a, c in ((gz2, bp2), (gz3, bp3)):
            assert np.array_equal(bits(gz), bits(a)) and np.array_equal(bits(bp), bits(c)), (tag, "bn_silu_bwd_reduce: runs differ")
        rgz, rsum, rsumx = V.bn_silu_bwd(case["ds"], z32, sc, sh, mu, inv)
        bg = V.bn_silu_bwd_gates(case["ds"], z32, sc, sh, mu, inv, RED_ROWS)
        ok(npy(gz), rgz, bg["gz"], tag + ("gz",))
        bsum = npy(bp).astype(np.float64).sum(axis=0)
        ok(bsum[0], rsum, bg["sum"], tag + ("sum gz",))
        ok(bsum[1], rsumx, bg["sumx"], tag + ("sum gz xhat",))
        # ---- sed_dwconv_glu_bwd on the reference's gz, v and coefficients rounded to fp32
        ca, cb, cc = (f32(a) for a in V.bn_bwd_coeffs(rsum, rsumx, R, case["gamma"], mu, inv, True))
        gz32, v32 = f32(rgz), f32(rv)
        dz = ca.astype(np.float64) * gz32 + cb.astype(np.float64) * z32 + cc.astype(np.float64)
        rdv, rdw, rdb = V.dwconv_bwd(dz, v32, w, B, t)
        wg = V.bwd_gates(gz32, z32, ca, cb, cc, v32, g, w, B, t, tile)
        dg, dw, db = run_bwd(L, gz32, z32, ca, cb, cc, v32, g, w, B, t, C, k, tag)
        ok(dg, V.glu_bwd(rdv, g), wg["dg"], tag + ("dg",))
        ok(dw, rdw, wg["dw"], tag + ("dw",))
        ok(db, rdb, wg["dbias"], tag + ("dbias",))


def test_refusals_launch_nothing(L):
    lib, P = L.lib(), L.ptr
    b = Bufs()
    B, t, C, k = 2, 5, 8, 3
    R = B * t
    g, w, bias, zi = b.inp(np.zeros((R + 1, 2 * C))), b.inp(np.zeros((C, 31))), b.inp(np.zeros(C)), b.inp(np.zeros((R + 1, C)))
    vec = b.inp(np.ones(C))
    z, v, part = b.out(R + 1, C), b.out(R + 1, C), b.out(4 * lib.sed_dwconv_nparts(B, t), 2, C)
    st = stream()

    def fwd(g=P(g), w=P(w), bias=P(bias), z=P(z), v=P(v), part=P(part), B=B, t=t, C=C, k=k):
        return lib.sed_dwconv_glu_fwd(g, w, bias, z, v, part, B, t, C, k, st)

    bad = [fwd(B=0), fwd(t=0), fwd(C=0), fwd(B=-1), fwd(C=6), fwd(C=2), fwd(k=4), fwd(k=1), fwd(k=33), fwd(k=0), fwd(k=-3), fwd(k=30),
           fwd(g=None), fwd(w=None), fwd(bias=None), fwd(z=None), fwd(g=g.data_ptr() + 4), fwd(z=z.data_ptr() + 4), fwd(v=v.data_ptr() + 4),
           fwd(t=2 ** 31 // (2 * C * 4)), fwd(B=65536)]
    s = b.out(R + 1, C)

    def silu(z=P(zi), scale=P(vec), shift=P(vec), s=P(s), R=R, C=C):
        return lib.sed_bn_silu_fwd(z, scale, shift, s, R, C, st)

    bad += [silu(R=0), silu(C=0), silu(C=6), silu(z=None), silu(scale=None), silu(shift=None), silu(s=None), silu(z=zi.data_ptr() + 4),
            silu(s=s.data_ptr() + 4)]
    gz, bpart = b.out(R + 1, C), b.out(lib.sed_bn_silu_bwd_nparts(R) + 1, 2, C)

    def red(ds=P(zi), z=P(zi), scale=P(vec), shift=P(vec), mean=P(vec), invstd=P(vec), gz=P(gz), part=P(bpart), R=R, C=C):
        return lib.sed_bn_silu_bwd_reduce(ds, z, scale, shift, mean, invstd, gz, part, R, C, st)

    bad += [red(R=0), red(C=0), red(C=6), red(ds=None), red(z=None), red(scale=None), red(shift=None), red(mean=None), red(invstd=None),
            red(gz=None), red(part=None), red(ds=zi.data_ptr() + 4), red(z=zi.data_ptr() + 4), red(gz=gz.data_ptr() + 4)]
    dg, dw, db, ws = b.out(R + 1, 2 * C), b.out(C, 31), b.out(C), b.out(4 * lib.sed_dwconv_glu_bwd_ws_floats(B, t, C, 31))

    def bwd(gz=P(zi), z=P(zi), ca=P(vec), cb=P(vec), cc=P(vec), v=P(zi), g=P(g), w=P(w), dg=P(dg), dw=P(dw), db=P(db), ws=P(ws), B=B, t=t, C=C, k=k):
        return lib.sed_dwconv_glu_bwd(gz, z, ca, cb, cc, v, g, w, dg, dw, db, ws, B, t, C, k, st)

    bad += [bwd(B=0), bwd(t=0), bwd(C=0), bwd(C=6), bwd(k=4), bwd(k=1), bwd(k=33), bwd(gz=None), bwd(z=None), bwd(ca=None), bwd(cb=None),
            bwd(cc=None), bwd(v=None), bwd(g=None), bwd(w=None), bwd(dg=None), bwd(dw=None), bwd(db=None), bwd(ws=None),
            bwd(gz=zi.data_ptr() + 4), bwd(v=zi.data_ptr() + 4), bwd(g=g.data_ptr() + 4), bwd(dg=dg.data_ptr() + 4), bwd(ws=ws.data_ptr() + 4),
            bwd(t=2 ** 31 // (2 * C * 4))]
    assert all(rc != 0 for rc in bad), bad
    assert lib.sed_last_error()
    assert lib.sed_dwconv_nparts(0, 5) == 0 and lib.sed_dwconv_glu_bwd_ws_floats(B, t, C, 4) == 0 and lib.sed_bn_silu_bwd_nparts(0) == 0
    b.intact()
    for o in (z, v, part, s, gz, bpart, dg, dw, db, ws):
        assert bool(torch.isnan(o).all()), "a refused call wrote an output"
    # and the accepted neighbours of the refused calls do launch: one clip of one frame, the eval form; the largest accepted t is not
    # run (it needs a 2 GB tensor), its refusal above is the size check alone
    L.check(fwd(B=1, t=1, v=None, part=None), "dwconv_glu_fwd")
    L.check(silu(R=1), "bn_silu_fwd")
    torch.cuda.synchronize()
    b.intact()
    assert bool(torch.isfinite(z[0]).all()) and bool(torch.isnan(z[1:]).all()) and bool(torch.isnan(v).all())
    assert bool(torch.isfinite(s[0]).all()) and bool(torch.isnan(s[1:]).all())
