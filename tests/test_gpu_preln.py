"""GPU: sed_resid_layernorm_fwd / sed_resid_layernorm_bwd (csrc/sed_layernorm.hip) through the C ABI, per element against the float64
definitions of tests/preln_formula.py within the gates derived in that file's docstring.

  shapes     rows in {1, 3, 4, 5, 63, 64, 65, 257} (four rows per workgroup, 64-row partial chunks) x C in {4, 60, 64, 68, 128, 260, 512,
             516} (64-lane column stride; the 8-register mask cache ends at 512), s in {1, 1/2, -0.75} and p in {0, 0.3} rotating over
             the cases so that every value meets every rows and every C
  data       rows of scale 1, 1e-2 and 1e4, and a row of one constant value (1 or 1e4 with a = 0 there: variance 0)
  arguments  a NULL / given; dres_in NULL / given / aliased to dxsum; da NULL / given; stats NULL gives the same y bits
  bit-equal  s = 1, p = 0: y and stats are sed_add_layernorm_fwd(x, a)'s and xsum the IEEE fp32 sum; s = 1, p > 0: sed_add_layernorm_fwd_drop's;
             dres_in NULL, s = 1: dxsum, dgamma, dbeta are sed_add_layernorm_bwd's on (xsum, zeros)
             (not asserted: with da given and p = 0.3 on the forward's xsum and stats, dgamma and dbeta are sed_add_layernorm_bwd_drop(x, a)'s
             bits at every BIT_CASES shape, and so are dxsum / dres and da up to C = 512; at C = 516 they differ in the last place in
             columns 512 ... 515, the columns behind the register mask, where the two instantiations' compiled code rounds differently)
  dropout    the keep cells are the ones sed_dropout_mask reports (and dropout_formula's)
  everywhere repeats give the same bits, inputs lie between NaN regions and outputs between canaries, refusals leave the outputs untouched
Run with -s for the worst error / gate of every check."""
import importlib

import numpy as np
import pytest
import torch

import dropout_formula as DF
import preln_formula as PF

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
GUARD = 1024
CANARY = -1024.0
SEED = (0x5EDD0001, 0x00C0FFEE)
STEP = 3
ROWS = [1, 3, 4, 5, 63, 64, 65, 257]
COLS = [4, 60, 64, 68, 128, 260, 512, 516]
SCALES = [1.0, 0.5, -0.75]
PS = [0.0, 0.3]
# case (i, j): s = SCALES[(i + j) % 3], p = PS[(i + j // 3) % 2] -- every s and every p meets every rows and every C
CASES = [(r, c, SCALES[(i + j) % 3], PS[(i + j // 3) % 2]) for i, r in enumerate(ROWS) for j, c in enumerate(COLS)]
EPS = PF.EPS


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def state(step=STEP, seed=SEED):
    return np.array([seed[0], seed[1], step, 0], dtype=np.uint32)


def dev_state(st):
    return torch.from_numpy(np.asarray(st, dtype=np.uint32).view(np.int32).copy()).cuda()


class Bufs:
    def __init__(self):
        self.outs = []

    def out(self, *shape, dtype=torch.float32):
        n = int(np.prod(shape))
        fill = CANARY if dtype == torch.float32 else 0x5A
        buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        buf[GUARD:GUARD + n] = float("nan") if dtype == torch.float32 else 0x77
        self.outs.append((buf, n, fill))
        return buf[GUARD:GUARD + n].view(shape)

    def out_from(self, a):
        """an output buffer between canaries that starts as a copy of a (an in-place operand)"""
        t = self.out(*a.shape)
        t.copy_(a)
        return t

    @staticmethod
    def inp(a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        buf = torch.full((a.size + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        buf[GUARD:GUARD + a.size] = torch.from_numpy(a.reshape(-1)).cuda()
        return buf[GUARD:GUARD + a.size].view(a.shape)

    def intact(self):
        torch.cuda.synchronize()
        for buf, n, fill in self.outs:
            assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), "write outside an output buffer"


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def untouched(*tensors):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(t).all()) for t in tensors)


def ok(got, ref, gate, tag):
    good, worst = PF.check(got, ref, gate, tag)
    assert good, (tag, worst)


def data(R, C, seed=None):
    """rows of scale 1, 1e-2, 1e4 in turn; row min(3, R - 1) holds one constant value with a = 0 there"""
    rng = np.random.default_rng(1000 * R + C if seed is None else seed)
    scale = np.array([1.0, 1e-2, 1e4])[np.arange(R) % 3][:, None]
    x, a = (rng.normal(0, 1, (R, C)) * scale).astype(np.float32), (rng.normal(0, 1, (R, C)) * scale).astype(np.float32)
    rc = min(3, R - 1)
    x[rc] = 1e4 if C % 8 else 1.0
    a[rc] = 0.0
    gamma, beta = rng.normal(1, 0.2, C).astype(np.float32), rng.normal(0, 0.2, C).astype(np.float32)
    dy, dres = rng.normal(0, 0.1, (R, C)).astype(np.float32), rng.normal(0, 0.1, (R, C)).astype(np.float32)
    return x, a, gamma, beta, dy, dres


def keep_cells(L, st, sid, R, C, p):
    """the cells sed_dropout_mask reports, checked against dropout_formula's"""
    if not p:
        return None, 1.0
    keep = torch.zeros((R, C), dtype=torch.uint8, device="cuda")
    L.check(L.lib().sed_dropout_mask(L.ptr(keep), 0, R, C, 0, p, L.ptr(dev_state(st)), sid, stream()), "dropout_mask")
    keep = keep.cpu().numpy()
    assert np.array_equal(keep, DF.keep_rows(st, sid, R, C, p))
    return keep, float(DF.thr_scale(p)[1])


@pytest.mark.parametrize("R,C,s,p", CASES, ids=lambda v: str(v))
def test_pair_against_formula(L, R, C, s, p):
    lib, P = L.lib(), L.ptr
    x, a, gamma, beta, dy, dres_in = data(R, C)
    st, sid = state(), DF.stream_id(1, PF.SITE_MAC_OUT)
    keep, sd = keep_cells(L, st, sid, R, C, p)
    b = Bufs()
    r = dev_state(st) if p else None              # p = 0 takes rng = NULL
    xd, ad, gd, bd, dyd, drd = (b.inp(v) for v in (x, a, gamma, beta, dy, dres_in))
    fwd = []
    for stats_on in (True, False, True):
        xsum, y, stats = b.out(R, C), b.out(R, C), b.out(R, 2)
        L.check(lib.sed_resid_layernorm_fwd(P(xd), P(ad), s, P(gd), P(bd), P(xsum), P(y), P(stats) if stats_on else None, R, C, EPS, p, P(r), sid,
                                            stream()), "resid_ln_fwd")
        fwd.append((xsum, y, stats))
    b.intact()
    assert untouched(fwd[1][2])
    for other in fwd[1:]:
        assert np.array_equal(bits(fwd[0][0]), bits(other[0])) and np.array_equal(bits(fwd[0][1]), bits(other[1]))
    assert np.array_equal(bits(fwd[0][2]), bits(fwd[2][2]))
    xsum, y, stats = fwd[0]
    ref = PF.resid_layernorm(x, a, s, gamma, beta, keep, sd)
    g = PF.resid_layernorm_gates(x, a, s, gamma, beta, keep, sd)
    tag = f"R{R} C{C} s{s} p{p}"
    ok(xsum.cpu().numpy(), ref["xsum"], g["xsum"], tag + " xsum")
    ok(y.cpu().numpy(), ref["y"], g["y"], tag + " y")
    ok(stats.cpu().numpy()[:, 0], ref["mean"], g["mean"], tag + " mean")
    # a = NULL: y = LayerNorm(x); xsum is not written, s and p are ignored
    xs0, y0, st0 = b.out(R, C), b.out(R, C), b.out(R, 2)
    L.check(lib.sed_resid_layernorm_fwd(P(xd), None, float("nan"), P(gd), P(bd), P(xs0), P(y0), P(st0), R, C, EPS, 7.0, None, 0, stream()), "resid_ln_fwd a=NULL")
    b.intact()
    assert untouched(xs0)
    r0, g0 = PF.resid_layernorm(x, None, 1.0, gamma, beta), PF.resid_layernorm_gates(x, None, 1.0, gamma, beta)
    ok(y0.cpu().numpy(), r0["y"], g0["y"], tag + " y (a NULL)")
    # backward, fed the forward's own xsum and stats
    xs32, st32 = xsum.cpu().numpy(), stats.cpu().numpy()
    nws = lib.sed_resid_layernorm_bwd_ws_floats(R, C)
    assert nws == lib.sed_add_layernorm_bwd_ws_floats(R, C)

    def bwd(res, alias, with_da):
        dxs = b.out_from(drd) if alias else b.out(R, C)
        da, dg, db, ws = b.out(R, C), b.out(C), b.out(C), b.out(max(1, nws))
        rin = dxs if alias else (drd if res else None)
        L.check(lib.sed_resid_layernorm_bwd(P(dyd), P(rin), P(xsum), P(gd), P(stats), s, P(dxs), P(da) if with_da else None, P(dg), P(db), P(ws),
                                            R, C, p, P(r), sid, stream()), "resid_ln_bwd")
        return dxs, da, dg, db

    runs = {key: bwd(*key) for key in ((True, False, True), (True, True, True), (True, False, False), (False, False, True),
                                       (False, False, False))}
    again = bwd(True, False, True)
    b.intact()
    full = runs[(True, False, True)]
    for u_, w_ in zip(full, again):
        assert np.array_equal(bits(u_), bits(w_)), "a repeat gave other bits"
    for u_, w_ in zip(full, runs[(True, True, True)]):
        assert np.array_equal(bits(u_), bits(w_)), "dxsum aliased to dres_in gave other bits"
    # da NULL: da is not written; dgamma / dbeta come from the same launches (same bits), dxsum from another instantiation of the row
    # kernel, whose contractions the compiler chooses on its own: held to the gate below like the others
    for res in (True, False):
        noda, with_da = runs[(res, False, False)], runs[(res, False, True)]
        assert untouched(noda[1]) and all(np.array_equal(bits(with_da[i]), bits(noda[i])) for i in (2, 3))
    for res in (True, False):
        rin = dres_in if res else None
        refb = PF.resid_layernorm(x, a, s, gamma, beta, keep, sd, dy, rin, xsum=xs32, stats=st32)
        gb = PF.resid_layernorm_gates(x, a, s, gamma, beta, keep, sd, dy, rin, xsum=xs32, stats=st32)
        for name, got in zip(("dxsum", "da", "dgamma", "dbeta"), runs[(res, False, True)]):
            ok(got.cpu().numpy(), refb[name], gb[name], f"{tag} {name} (dres_in {'given' if res else 'NULL'})")
        ok(runs[(res, False, False)][0].cpu().numpy(), refb["dxsum"], gb["dxsum"], f"{tag} dxsum (da NULL, dres_in {'given' if res else 'NULL'})")


BIT_CASES = [(r, c) for r in (1, 5, 65, 257) for c in (4, 68, 260, 512, 516)]


@pytest.mark.parametrize("R,C", BIT_CASES, ids=lambda v: str(v))
def test_s1_gives_the_post_ln_entries_bits(L, R, C):
    lib, P = L.lib(), L.ptr
    x, a, gamma, beta, dy, _ = data(R, C, seed=7 * R + C)
    b = Bufs()
    st, sid = state(), DF.stream_id(2, 4)
    r = dev_state(st)
    xd, ad, gd, bd, dyd = (b.inp(v) for v in (x, a, gamma, beta, dy))
    nws = lib.sed_add_layernorm_bwd_ws_floats(R, C)
    for p in (0.0, 0.3):
        xsum, y, stats, y1, stats1 = b.out(R, C), b.out(R, C), b.out(R, 2), b.out(R, C), b.out(R, 2)
        L.check(lib.sed_resid_layernorm_fwd(P(xd), P(ad), 1.0, P(gd), P(bd), P(xsum), P(y), P(stats), R, C, EPS, p, P(r), sid, stream()), "fwd")
        if p:
            L.check(lib.sed_add_layernorm_fwd_drop(P(xd), P(ad), P(gd), P(bd), P(y1), P(stats1), R, C, EPS, p, P(r), sid, stream()), "fwd_drop")
        else:
            L.check(lib.sed_add_layernorm_fwd(P(xd), P(ad), P(gd), P(bd), P(y1), P(stats1), R, C, EPS, stream()), "fwd plain")
        b.intact()
        assert np.array_equal(bits(y), bits(y1)) and np.array_equal(bits(stats), bits(stats1))
        if not p:
            assert np.array_equal(bits(xsum), (x + a).view(np.uint32)), "xsum is not the IEEE fp32 sum"
        # dres_in = NULL, s = 1: the post-LN backward on (xsum, zeros)
        zero = torch.zeros((R, C), device="cuda")
        dxs, dg, db, ws = b.out(R, C), b.out(C), b.out(C), b.out(max(1, nws))
        dres, dg1, db1, ws1 = b.out(R, C), b.out(C), b.out(C), b.out(max(1, nws))
        L.check(lib.sed_resid_layernorm_bwd(P(dyd), None, P(xsum), P(gd), P(stats), 1.0, P(dxs), None, P(dg), P(db), P(ws), R, C, 0.0, None, 0,
                                            stream()), "bwd")
        L.check(lib.sed_add_layernorm_bwd(P(dyd), P(xsum), P(zero), P(gd), P(stats), P(dres), P(dg1), P(db1), P(ws1), R, C, stream()), "bwd plain")
        b.intact()
        assert np.array_equal(bits(dxs), bits(dres)) and np.array_equal(bits(dg), bits(dg1)) and np.array_equal(bits(db), bits(db1))


def test_refusals_leave_the_outputs_untouched(L):
    lib, P = L.lib(), L.ptr
    R, C = 5, 68
    x, a, gamma, beta, dy, dres_in = data(R, C)
    b = Bufs()
    r = dev_state(state())
    xd, ad, gd, bd, dyd, drd = (b.inp(v) for v in (x, a, gamma, beta, dy, dres_in))
    xsum, y, stats = b.out(R, C), b.out(R, C), b.out(R, 2)
    s = stream()
    fwd = lambda **kw: lib.sed_resid_layernorm_fwd(*[kw.get(k, v) for k, v in (("x", P(xd)), ("a", P(ad)), ("s", 0.5), ("gamma", P(gd)), ("beta", P(bd)),
                                                                                ("xsum", P(xsum)), ("y", P(y)), ("stats", P(stats)), ("rows", R), ("C", C),
                                                                                ("eps", EPS), ("p", 0.1), ("rng", P(r)), ("sid", 1), ("stream", s))])
    for kw in (dict(rows=0), dict(C=0), dict(C=-4), dict(x=None), dict(gamma=None), dict(beta=None), dict(y=None), dict(xsum=None),
               dict(s=float("nan")), dict(s=float("inf")), dict(p=-0.1), dict(p=1.0), dict(p=float("nan")), dict(rng=None)):
        assert fwd(**kw) != 0, kw
    assert untouched(xsum, y, stats)
    assert fwd() == 0 and fwd(p=0.0, rng=None) == 0                 # (p = 0 needs no state)
    torch.cuda.synchronize()
    xs_ok, st_ok = xsum.clone(), stats.clone()
    dxs, da, dg, db = b.out(R, C), b.out(R, C), b.out(C), b.out(C)
    ws = b.out(max(1, lib.sed_resid_layernorm_bwd_ws_floats(R, C)))
    bwd = lambda **kw: lib.sed_resid_layernorm_bwd(*[kw.get(k, v) for k, v in (("dy", P(dyd)), ("dres_in", P(drd)), ("xsum", P(xs_ok)), ("gamma", P(gd)),
                                                                                ("stats", P(st_ok)), ("s", 0.5), ("dxsum", P(dxs)), ("da", P(da)),
                                                                                ("dgamma", P(dg)), ("dbeta", P(db)), ("ws", P(ws)), ("rows", R), ("C", C),
                                                                                ("p", 0.1), ("rng", P(r)), ("sid", 1), ("stream", s))])
    for kw in (dict(rows=0), dict(C=0), dict(dy=None), dict(xsum=None), dict(gamma=None), dict(stats=None), dict(dxsum=None), dict(dgamma=None),
               dict(dbeta=None), dict(ws=None), dict(rows=65535 * 64 + 1), dict(s=float("nan")), dict(s=float("-inf")), dict(p=-0.1), dict(p=1.0),
               dict(p=float("nan")), dict(rng=None)):
        assert bwd(**kw) != 0, kw
    assert untouched(dxs, da, dg, db, ws)
    assert lib.sed_resid_layernorm_bwd_ws_floats(0, C) == 0 and lib.sed_resid_layernorm_bwd_ws_floats(R, 0) == 0
    assert bwd() == 0 and bwd(p=0.0, rng=None) == 0 and bwd(da=None, s=float("nan"), p=3.0, rng=None) == 0      # (da NULL: s, p ignored)
    b.intact()
    assert L.lib().sed_last_error()
