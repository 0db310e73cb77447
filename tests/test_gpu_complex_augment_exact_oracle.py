"""GPU: the Complex-mode batch kernel (csrc/sed_frontend.hip: sed_complex_augment_logmel -- crop gather from the STFT bank, mean of up to
four crops, real Gaussian noise from a caller's array or the in-kernel splitmix64 / Box-Muller generator, complex z-score, |.|^2, mel
bands, 10 log10 with the floor) per element against float64, through the C ABI.  Reference, gate, their derivation and the case list:
tests/frontend_formula.py (mix_logmel_reference, mix_ratio, MIX_CASES), checked without a GPU in tests/test_frontend_formula_host.py: a
plain fp32 emulation passes the gate at every case, every mutated reference fails it.

Constants (derived there, fixed before the first GPU run): the per-bin bound E_k counts nmix - 1 adds, the rounded 1 / nmix and its
product (nmix 3 only), the fma with the noise, the subtraction of the mean, the rounded 1 / std and its product; generator noise adds
nstd * C_GEN u, C_GEN = sqrt(48 ln 2) (4 pi + 8 + 4 + 1) = 147.5; the power gate adds sed_complex_to_logmel's C_ABS2 = 5 plus a quarter
of the band length + 2 plus the dB terms.

Every input sits between NaN words (the integer tables between words that are no legal index), the bank between NaN rows, so the row
after the last legal crop is NaN; `out` sits between marked words.  Every element of every case is checked.

Measured on the MI355X, max err / bound per group (run with -s for the table; records, not thresholds):
  group                max err/bound   margin   where the maximum sits
  plain                0.400           2.5x     bands of 1 .. 5 bins (bank "lengths"): the bound counts a handful of roundings in the worst case
  mixed                0.568           1.8x     n_mels 65, nmix 4 3 2 1, a clip at 30 beside one at 1e-3
  explicit noise       0.576           1.7x     n_mels 130, nstd 0.7 .. 0.004, the same amplitudes
  generator            0.509           2.0x     n_mels 65, nstd 0.3 and 0.004
  z-score              0.554           1.8x     n_mels 130, bank "lengths"
  wide bins            0.275           3.6x     bins 16385, bank "lengths"; bins 32769: 0.196
  generator read-out   0.175           5.7x     every draw of 2 x 3 x 257 within 2.0e-5 of the float64 Box-Muller value
  device_batch         0.304           3.3x     tests/test_gpu_dataset_eval.py: 64 augmented clips of 30 frames, 513 bins
  identity, bits       bit-equal
No group exceeds the gate, n_mels > 64 and bins 32769 included: the file found nothing to fix in the kernel.  The margins of 1.7 .. 2.5 are
those of sed_complex_to_logmel's own gate (0.60 in tests/test_gpu_frontend_exact_oracle.py) on the same short bands; the plain fp32
emulation of the host file reaches 0.28 .. 0.33 on the same cases.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import frontend_formula as FF
from oracle import dataset_oracle as DO

pytestmark = pytest.mark.gpu

GUARD = 64
NAN_BITS = 0x7FC00000                    # a quiet NaN as a float, 2143289344 as an index
RATIOS = {}                              # group -> max err / bound measured
_RUNS = {}                               # case id -> (inputs, the kernel's output): one launch per case for all the tests that read it


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module("soundeventdetection-pytorch_amd")._lib


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if RATIOS:
        print("\nmax err / bound by group (1 = the gate)")
        for k in sorted(RATIOS):
            print(f"  {k:18s} {RATIOS[k]:.3f}   " + (f"(margin {1.0 / RATIOS[k]:.1f}x)" if RATIOS[k] > 0 else "(exact)"))


def _note(group, r):
    r = float(r)
    RATIOS[group] = max(RATIOS.get(group, 0.0), r)
    return r


class Fenced:
    """a host array on the device between `guard` words of NaN_BITS on either side (None stays NULL)"""

    def __init__(self, a, guard=GUARD):
        a = np.ascontiguousarray(a)
        assert a.dtype.itemsize % 4 == 0 and guard % 2 == 0
        h = np.full(a.size * a.dtype.itemsize // 4 + 2 * guard, NAN_BITS, np.uint32)
        h[guard:len(h) - guard] = a.reshape(-1).view(np.uint32)
        self.buf = torch.from_numpy(h.view(np.int32)).cuda()
        self.ptr = self.buf.data_ptr() + 4 * guard


def _fence(a, guard=GUARD):
    return None if a is None else Fenced(a, guard)


def _p(f):
    return None if f is None else f.ptr


class Guarded:
    """a float32 device buffer of n words, NaN-filled, with GUARD marked words in front and behind"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), 12345.0, dtype=torch.float32, device="cuda")
        self.buf[GUARD:GUARD + n] = float("nan")
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def numpy(self):
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == 12345.0).all() and (h[GUARD + self.n:] == 12345.0).all(), "write outside the output"
        return h[GUARD:GUARD + self.n]


class Launch:
    """one case's arrays on the device; run(**overrides) -> (return code, Guarded out)"""

    def __init__(self, L, d):
        self.L, self.d = L, d
        self.starts_h = np.ascontiguousarray(d["starts"], np.int32)
        self.nmix_h = np.ascontiguousarray(d["nmix"], np.int32)
        assert self.starts_h.shape == (d["B"], 4)
        self.dev = dict(bank=Fenced(d["bank"], 2 * d["bins"]), starts=Fenced(self.starts_h), nmix=Fenced(self.nmix_h), nstd=_fence(d["nstd"]),
                        z=_fence(d["z"]), cmean=_fence(d["cmean"]), cstd=_fence(d["cstd"]), W=Fenced(d["W"]), lo=Fenced(d["lo"]),
                        hi=Fenced(d["hi"]))

    def run(self, **kw):
        d, v = self.d, self.dev
        a = dict(bank=v["bank"].ptr, frames=d["frames"], starts_h=self.starts_h.ctypes.data, nmix_h=self.nmix_h.ctypes.data,
                 starts=v["starts"].ptr, nmix=v["nmix"].ptr, nstd=_p(v["nstd"]), z=_p(v["z"]), seed=d["seed"], cmean=_p(v["cmean"]),
                 cstd=_p(v["cstd"]), W=v["W"].ptr, lo=v["lo"].ptr, hi=v["hi"].ptr, B=d["B"], crop=d["crop"], bins=d["bins"],
                 n_mels=d["n_mels"], out_words=d["B"] * d["crop"] * d["n_mels"])
        a.update(kw)
        out = Guarded(a["out_words"])
        rc = self.L.lib().sed_complex_augment_logmel(
            a["bank"], a["frames"], a["starts_h"], a["nmix_h"], a["starts"], a["nmix"], a["nstd"], a["z"], ctypes.c_ulonglong(a["seed"]),
            a["cmean"], a["cstd"], a["W"], a["lo"], a["hi"], out.ptr, a["B"], a["crop"], a["bins"], a["n_mels"],
            torch.cuda.current_stream().cuda_stream)
        return rc, out

    def output(self, **kw):
        rc, out = self.run(**kw)
        self.L.check(rc, "complex_augment_logmel")
        return out.numpy().reshape(self.d["B"], self.d["crop"], self.d["n_mels"]).copy()


def _case(L, c):
    key = FF.mix_id(c)
    if key not in _RUNS:
        d = FF.make_mix_inputs(c)
        k = np.arange(c["bins"])[None, :]
        assert (d["W"][(k < d["lo"][:, None]) | (k >= d["hi"][:, None])] == 0).all()
        _RUNS[key] = (d, Launch(L, d).output())
    return _RUNS[key]


# ---- cases: every element within its bound ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FF.MIX_CASES, ids=FF.mix_id)
def test_every_element_meets_its_bound(L, c):
    d, got = _case(L, c)
    ref = FF.mix_reference_of(d)
    r = FF.mix_ratio(got, ref)
    print(f"\n{FF.mix_id(c)} [{FF.mix_group(c)}]: max err/bound {_note(FF.mix_group(c), r.max()):.3f}", end="")
    i = np.unravel_index(r.argmax(), r.shape)
    assert r.max() <= 1.0, f"element {i}: err/bound {r[i]}, got {got[i]!r}, reference {ref.v[i]!r} (mel power {ref.p[i]!r})"
    if c["kind"] == "zero" and not c["zscore"]:
        assert (got == -100.0).all()                        # silence
    assert (got[..., d["hi"] == d["lo"]] == -100.0).all()   # empty bands


# ---- sensitivity: the gate rejects every mutated reference on the kernel's own output --------------------------------------------------
@pytest.mark.parametrize("c", [c for c in FF.MIX_CASES if FF.mix_mutations_for(c)], ids=FF.mix_id)
def test_mutated_references_fail_the_gate(L, c):
    d, got = _case(L, c)
    assert FF.mix_ratio(got, FF.mix_reference_of(d)).max() <= 1.0
    for mut in FF.mix_mutations_for(c):
        r = FF.mix_ratio(got, FF.mix_reference_of(d, mut)).max()
        print(f"\n{FF.mix_id(c)} {mut}: max err/bound {r:.3g}", end="")
        assert r > 1.0, mut


# ---- the generator, read out draw by draw ----------------------------------------------------------------------------------------------
def test_generator_read_out(L):
    """bank == (8, 0), nmix 1, nstd 1, no z-score, one unit filter per bin: out = 10 log10((8 + z)^2), and 8 + z > 0 since |z| < 5.8.
    Bound on the recovered z: C_GEN u (the device's Box-Muller against float64) + u |z| (the oracle's draw is rounded to fp32) + half
    the relative error of the power times 8 + z: the fma 8 + z (u, twice in the power), sqrt(x^2)^2 (C_ABS2 u), the logarithm and the
    product by 10 (C_LOG u |v| dB); the single-term band sum and its two adds of zero are exact."""
    bins, B, crop = 257, 2, 3
    d = dict(bins=bins, n_mels=bins, crop=crop, frames=crop, B=B, bank=np.full((crop, bins), 8.0, np.complex64),
             starts=np.array([[0, -1, FF.INT_MAX, -1]] * B, np.int32), nmix=np.ones(B, np.int32), nstd=np.ones(B, np.float32), z=None,
             seed=0xC0FFEE123456789, cmean=None, cstd=None, W=np.eye(bins, dtype=np.float32), lo=np.arange(bins, dtype=np.int32),
             hi=np.arange(1, bins + 1, dtype=np.int32))
    run = Launch(L, d)
    ctr = (np.arange(B * crop, dtype=np.uint64)[:, None] * np.uint64(bins) + np.arange(bins, dtype=np.uint64)[None, :]).reshape(B, crop, bins)

    def read(seed):
        out = run.output(seed=seed).astype(np.float64)
        z_ref = DO.counter_normal(seed, ctr).astype(np.float64)
        x = 8.0 + z_ref
        c_r = 2.0 + FF.C_ABS2 + FF.LN10_10 * FF.C_LOG * np.abs(20.0 * np.log10(x))
        bound = FF.U * (FF.C_GEN + np.abs(z_ref) + 0.5 * c_r * x)
        return 10.0 ** (out / 20.0) - 8.0, z_ref, bound

    z, z_ref, bound = read(d["seed"])
    r = np.abs(z - z_ref) / bound
    print(f"\ngenerator read-out: max err/bound {_note('generator read-out', r.max()):.3f}, largest bound {bound.max():.3g}", end="")
    assert r.max() <= 1.0, (np.unravel_index(r.argmax(), r.shape), r.max())
    assert np.abs(z_ref).max() > 3.5 and bound.max() < 1e-4
    # the counter is (b * crop + t) * bins + k and nothing else
    for name, other in (("no frame term", np.broadcast_to(ctr[0, 0], ctr.shape)), ("the frame within the clip alone", np.broadcast_to(ctr[0], ctr.shape)),
                        ("one element on", ctr + np.uint64(1))):
        off = np.abs(z - DO.counter_normal(d["seed"], other).astype(np.float64)) > bound
        assert off[other != ctr].mean() > 0.99 and (other != ctr).sum() >= 2 * bins, name
    # two frames and two clips draw differently; so do two seeds
    assert (np.abs(z[:, 0] - z[:, 1]) > 2 * bound[:, 0]).mean() > 0.99 and (np.abs(z[0] - z[1]) > 2 * bound[0]).mean() > 0.99
    z2, z2_ref, bound2 = read(d["seed"] ^ (1 << 63))                               # (the top bit of the seed reaches the kernel)
    assert (np.abs(z2 - z2_ref) <= bound2).all() and (np.abs(z2 - z) > 2 * bound).mean() > 0.99


# ---- identity: without mixing, noise and z-score the kernel IS sed_complex_to_logmel on the gathered rows ------------------------------
@pytest.mark.parametrize("c", [FF._mc(513, 65, 9, "lengths", [1, 1, 1]), FF._mc(16385, 17, 1, "lengths", [1, 1], frames=6)], ids=FF.mix_id)
def test_plain_crops_equal_complex_to_logmel_bit_for_bit(L, c):
    d = FF.make_mix_inputs(c)
    run = Launch(L, d)
    got = run.output()
    rows = np.concatenate([d["bank"][s:s + c["crop"]] for s in d["starts"][:, 0]])
    spec = Fenced(rows)
    out = Guarded(rows.shape[0] * c["n_mels"])
    L.check(L.lib().sed_complex_to_logmel(spec.ptr, run.dev["W"].ptr, run.dev["lo"].ptr, run.dev["hi"].ptr, None, None, out.ptr, rows.shape[0],
                                          c["bins"], c["n_mels"], torch.cuda.current_stream().cuda_stream), "complex_to_logmel")
    want = out.numpy().reshape(got.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a zero nstd gives the bits of noise_std == NULL, with and without a noise array behind it
    zeros = Fenced(np.zeros(d["B"], np.float32))
    noise = Fenced(np.full((d["B"], c["crop"], c["bins"]), 3.0, np.float32))
    assert np.array_equal(run.output(nstd=zeros.ptr).view(np.uint32), got.view(np.uint32))
    assert np.array_equal(run.output(nstd=zeros.ptr, z=noise.ptr).view(np.uint32), got.view(np.uint32))


# ---- bits: a repeated launch, and the same rows through another (B, crop) --------------------------------------------------------------
def test_bits_do_not_depend_on_the_launch_or_the_batch_shape(L):
    c = FF._mc(257, 65, 6, "lengths", [3], "explicit", (0.05,), zscore=True)
    base = FF.make_mix_inputs(c)
    s0 = np.array([3, 20, 11], np.int32)
    outs = {}
    for B, crop in ((1, 6), (2, 3), (6, 1)):
        starts = np.full((B, 4), -1, np.int32)
        starts[:, :3] = s0[None, :] + crop * np.arange(B, dtype=np.int32)[:, None]
        d = dict(base, B=B, crop=crop, starts=starts, nmix=np.full(B, 3, np.int32), nstd=np.full(B, 0.05, np.float32),
                 z=base["z"].reshape(B, crop, c["bins"]))
        run = Launch(L, d)
        outs[B] = run.output().reshape(6, c["n_mels"])
        assert np.array_equal(run.output().reshape(6, -1).view(np.uint32), outs[B].view(np.uint32)), "a repeated launch"
        r = FF.mix_ratio(outs[B].reshape(B, crop, -1), FF.mix_reference_of(d))
        assert _note("explicit noise", r.max()) <= 1.0
        if B == 2:                                                             # generator noise: the same launch gives the same bits
            g = run.output(z=None, seed=99)
            assert np.array_equal(run.output(z=None, seed=99).view(np.uint32), g.view(np.uint32))
            assert not np.array_equal(run.output(z=None, seed=100).view(np.uint32), g.view(np.uint32))
    assert np.array_equal(outs[1].view(np.uint32), outs[2].view(np.uint32)) and np.array_equal(outs[1].view(np.uint32), outs[6].view(np.uint32))


# ---- refusals: the error code, and nothing is launched ----------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(L):
    c = FF._mc(33, 17, 3, "lengths", [2, 1], "explicit", (0.004, 0.0), zscore=True, frames=10)
    d = FF.make_mix_inputs(c)
    run = Launch(L, d)
    rc, out = run.run()
    assert rc == 0 and np.isfinite(out.numpy()).all()

    def host(field, b, j, value):
        a = (run.starts_h if field == "starts_h" else run.nmix_h).copy()
        a[(b, j) if field == "starts_h" else b] = value
        return a

    last = c["frames"] - c["crop"]
    small = dict(out_words=64)
    bad = {
        "nmix 0": dict(nmix_h=host("nmix_h", 1, 0, 0)), "nmix 5": dict(nmix_h=host("nmix_h", 0, 0, 5)),
        "start -1": dict(starts_h=host("starts_h", 0, 1, -1)), "start + crop == frames + 1": dict(starts_h=host("starts_h", 1, 0, last + 1)),
        "mean without std": dict(cstd=None), "std without mean": dict(cmean=None),
        "bins 0": dict(bins=0), "bins 32770": dict(bins=32770), "n_mels 0": dict(n_mels=0), "B 0": dict(B=0), "crop 0": dict(crop=0),
        "B * crop >= 2^31": dict(B=46341, crop=46341, **small),
        "host starts NULL": dict(starts_h=None), "host nmix NULL": dict(nmix_h=None), "device starts NULL": dict(starts=None),
        "device nmix NULL": dict(nmix=None),
    }
    for name, kw in bad.items():
        rc, out = run.run(**{k: (v.ctypes.data if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
        assert rc != 0, name
        assert L.lib().sed_last_error(), name
        assert np.isnan(out.numpy()).all(), name
    rc, out = run.run()                                                        # and the launch still works afterwards
    assert rc == 0 and np.isfinite(out.numpy()).all()
