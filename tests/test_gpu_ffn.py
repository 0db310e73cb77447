"""GPU: the fused feed-forward sub-layer and the activation backward of csrc/sed_ffn.hip through the C ABI, per element against the
float64 definition in tests/ffn_formula.py, within the gates derived in that file's docstring (SED_F32 and SED_BF16, ReLU and GELU).

Shapes (R, C, D): rows under, on and over the 32-row tile and over several workgroups; C with one to four output tiles per wave and
tile counts that are no multiple of the four waves (C = 160: five); D under, on and over the 128-wide step, with a ragged last step
(96, 160, 416) and many steps (2048).  Every input lies between NaN regions (a read past the R rows poisons an output), every output
in a NaN-filled buffer between canary regions.  Run with -s for the worst error / gate of every check."""
import importlib

import numpy as np
import pytest
import torch

import ffn_formula as F

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
GUARD = 1024
CANARY = -1024.0
F32, BF16 = 0, 1
SHAPES = [(1, 32, 32), (31, 32, 96), (33, 64, 160), (65, 160, 416), (130, 128, 512), (40, 512, 2048)]
ACTS = ["relu", "gelu"]


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


def run_fwd(L, dt, act, x, w1, b1, w2, b2, tag):
    """with u, without u, with u again; -> (y, u) as numpy after the poisoning / canary / repeat checks"""
    lib, P = L.lib(), L.ptr
    R, C = x.shape
    D = w1.shape[0]
    b = Bufs()
    host = (x, w1, b1, w2, b2)
    dev = [b.inp(v) for v in host]
    y, u, y2, y3, u3 = b.out(R, C), b.out(R, D), b.out(R, C), b.out(R, C), b.out(R, D)
    code = F.ACT_CODE[act]
    for yy, uu in ((y, u), (y2, None), (y3, u3)):
        L.check(lib.sed_ffn_fwd(dt, code, *(P(v) for v in dev), P(yy), P(uu) if uu is not None else None, R, C, D, stream()), "ffn_fwd")
    b.intact()
    for d, hv in zip(dev, host):
        assert np.array_equal(d.cpu().numpy(), hv), "an input was modified"
    assert np.array_equal(bits(y), bits(y2)), (tag, "u = NULL changed y")
    assert np.array_equal(bits(y), bits(y3)) and np.array_equal(bits(u), bits(u3)), (tag, "two runs differ")
    return y.cpu().numpy(), u.cpu().numpy()


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] <= 64], ids=str)
def test_exact_integer_family(L, shape, dt):
    R, C, D = shape
    x, w1, b1, w2, b2 = F.exact_case(np.random.default_rng(R + C + D), R, C, D)
    ref = F.ffn(x, w1, b1, w2, b2, "relu")
    assert np.abs(ref["u"]).max() <= 256 and np.array_equal(ref["u"], np.round(ref["u"]))
    y, u = run_fwd(L, dt, "relu", x, w1, b1, w2, b2, (shape, dt))
    assert np.array_equal(u.astype(np.float64), ref["u"]), "u is not exact: a fragment-order or bias error"
    assert np.array_equal(y.astype(np.float64), ref["y"]), "y is not exact: a fragment-order or column-split error"


def gaussian_case(shape, dt, seed=0):
    R, C, D = shape
    rng = np.random.default_rng(R * 7 + C * 3 + D + seed)
    x = rng.normal(0.0, 1.0, (R, C)).astype(np.float32)
    w1 = rng.normal(0.0, 1.0 / np.sqrt(C), (D, C)).astype(np.float32)
    b1 = rng.normal(0.0, 0.5, D).astype(np.float32)
    w2 = rng.normal(0.0, 1.0 / np.sqrt(D), (C, D)).astype(np.float32)
    b2 = rng.normal(0.0, 0.5, C).astype(np.float32)
    return x, w1, b1, w2, b2


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gaussian_family(L, shape, dt, act):
    case = gaussian_case(shape, dt)
    ref = F.ffn(*case, act)
    gates = F.ffn_gates(*case, act, mode="bf16" if dt == BF16 else "f32")
    y, u = run_fwd(L, dt, act, *case, (shape, dt, act))
    ok(u, ref["u"], gates["u"], (shape, dt, act, "u"))
    ok(y, ref["y"], gates["y"], (shape, dt, act, "y"))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("n", [1, 3, 4, 255, 1024, 1027, 40 * 2048 + 2])
def test_act_bwd_plain_and_aliased(L, n, act):
    lib, P = L.lib(), L.ptr
    rng = np.random.default_rng(n)
    u = rng.normal(0.0, 2.5, n).astype(np.float32)
    u[:: 7] = 0.0                                  # ReLU's convention at 0
    u[n // 2] = -9.5
    da = rng.normal(0.0, 1.0, n).astype(np.float32)
    ref_a, ref_du = F.act_fwd(u, act), da.astype(np.float64) * F.act_grad(u, act)
    gates = F.act_bwd_gates(u, da, act)
    code = F.ACT_CODE[act]
    b = Bufs()

    def verify(a, du, tag):
        b.intact()
        ok(a.cpu().numpy(), ref_a, gates["a"], (n, act, tag, "a"))
        ok(du.cpu().numpy(), ref_du, gates["du"], (n, act, tag, "du"))
        return bits(a), bits(du)

    du_, dda, a, du = b.inp(u), b.inp(da), b.out(n), b.out(n)
    L.check(lib.sed_ffn_act_bwd(code, P(du_), P(dda), P(a), P(du), n, stream()), "ffn_act_bwd")
    plain = verify(a, du, "plain")
    assert np.array_equal(du_.cpu().numpy(), u) and np.array_equal(dda.cpu().numpy(), da), "an input was modified"
    # both aliased forms at once: a over u, du over da (outputs between canaries, holding the inputs)
    ua, dua = b.out(n), b.out(n)
    ua.copy_(torch.from_numpy(u))
    dua.copy_(torch.from_numpy(da))
    L.check(lib.sed_ffn_act_bwd(code, P(ua), P(dua), P(ua), P(dua), n, stream()), "ffn_act_bwd")
    alias = verify(ua, dua, "aliased")
    assert np.array_equal(plain[0], alias[0]) and np.array_equal(plain[1], alias[1]), "the aliased form gives other bits"
    # one aliased pair each
    ua2, du2 = b.out(n), b.out(n)
    ua2.copy_(torch.from_numpy(u))
    L.check(lib.sed_ffn_act_bwd(code, P(ua2), P(dda), P(ua2), P(du2), n, stream()), "ffn_act_bwd")
    assert np.array_equal(verify(ua2, du2, "a over u")[1], plain[1])
    if n > 1:                                      # the scalar route (a pointer off the 16-byte grid) gives the same values
        uo, dao, ao, duo = b.inp(u), b.inp(da), b.out(n + 1), b.out(n + 1)
        L.check(lib.sed_ffn_act_bwd(code, P(uo), P(dao), ao.data_ptr() + 4, duo.data_ptr() + 4, n - 1, stream()), "ffn_act_bwd")
        b.intact()
        assert np.array_equal(bits(ao[1:n]), plain[0][:n - 1]) and np.array_equal(bits(duo[1:n]), plain[1][:n - 1])
        assert bool(torch.isnan(ao[0])) and bool(torch.isnan(ao[n])) and bool(torch.isnan(duo[n]))


def test_refusals_launch_nothing(L):
    lib, P = L.lib(), L.ptr
    b = Bufs()
    R, C, D = 5, 32, 64
    x, w1, b1, w2, b2 = (b.inp(np.zeros(s)) for s in ((R + 1, C), (D, C), (D,), (C, D), (C,)))
    y, u = b.out(R + 1, C), b.out(R + 1, D)
    st = stream()

    def fwd(dt=F32, act=0, x=P(x), w1=P(w1), b1=P(b1), w2=P(w2), b2=P(b2), y=P(y), u=P(u), R=R, C=C, D=D):
        return lib.sed_ffn_fwd(dt, act, x, w1, b1, w2, b2, y, u, R, C, D, st)

    bad = [fwd(R=0), fwd(C=48), fwd(C=0), fwd(C=544), fwd(D=48), fwd(D=0), fwd(D=4128), fwd(dt=2), fwd(dt=-1), fwd(act=2), fwd(act=-1),
           fwd(x=None), fwd(w1=None), fwd(b1=None), fwd(w2=None), fwd(b2=None), fwd(y=None),
           fwd(x=x.data_ptr() + 4), fwd(w1=w1.data_ptr() + 4), fwd(w2=w2.data_ptr() + 4), fwd(y=y.data_ptr() + 4), fwd(u=u.data_ptr() + 4)]
    n = R * D
    a, du = b.out(2 * n), b.out(2 * n)

    def bwd(act=0, u=P(u), da=P(x), a=P(a), du=P(du), n=n):
        return lib.sed_ffn_act_bwd(act, u, da, a, du, n, st)

    bad += [bwd(n=0), bwd(act=2), bwd(u=None), bwd(da=None), bwd(a=None), bwd(du=None),
            bwd(u=P(a), a=a.data_ptr() + 16), bwd(u=a.data_ptr() + 16, a=P(a)),          # a partly over u
            bwd(da=P(du), du=du.data_ptr() + 4 * (n - 1)),                              # du partly over da
            bwd(da=P(a)), bwd(u=P(du)), bwd(a=P(a), du=a.data_ptr() + 4 * (n - 1))]      # an output over the other pair's buffer
    assert all(rc != 0 for rc in bad), bad
    assert lib.sed_last_error()
    b.intact()
    for o in (y, u, a, du):
        assert bool(torch.isnan(o).all()), "a refused call wrote an output"
    # and the accepted neighbours of the refused calls do launch: R = 1 row, u = NULL
    L.check(fwd(R=1, u=None), "ffn_fwd")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y[0]).all()) and bool(torch.isnan(y[1:]).all())
