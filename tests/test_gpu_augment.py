"""GPU: sed_logmel_augment (csrc/sed_augment.hip) through the C ABI, and the layers on top of it (LogMelAugment,
SpectogramDataset(spec_augment=...), train(batch_augment=...)).

Reference: tests/augment_formula.py (checked on the host in tests/test_augment_host.py).  No kernel of this library serves as a
reference; the one comparison with sed_logmel_crops is an identity check (everything off = the plain crop launch, bit for bit).

Exactness rules (augment_formula.augment_vectorised returns the stage values):
  * a masked cell holds mask_value, np.array_equal; masked and unmasked cells are compared separately;
  * an unmasked cell of a sample without mixup equals u32 bit for bit: the shifted source value, or float32(z) + float32(g), ONE
    IEEE add.  With mean / std, z is the fp32 expression (x - mean) / std -- one IEEE subtraction and one IEEE division -- and sits
    within rtol = atol = 1e-6 of float64, the tolerance of the dataset's end-to-end test;
  * an unmasked cell of a mixed sample: |out - ref64| <= 3 * 2^-24 * (|lam * u_b| + |(1 - lam) * u_p|) with ref64 = lam * u_b +
    (1 - lam) * u_p in float64 over the fp32 u: one rounding per product and one for the sum (fewer with an FMA; 1 - lam is exact
    for lam in [0.5, 1] and costs at most the second product's slack below that).  Derived, not measured;
  * labels: max rule np.array_equal, convex rule within 4 * 2^-53 relative (two products, one sum, in double).
Every output lies in a sentinel-filled buffer between two canary regions; every input must be unmodified afterwards.  The banks are
continuous random values, distinct around every crop, so a shift that leaks into a neighbouring frame cannot go unnoticed."""
import importlib
import os
import pickle

import numpy as np
import pytest
import torch

from augment_formula import augment_vectorised, make_row, table_lam

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
GUARD = 1024
FILL = {torch.float32: (float("nan"), -1024.0), torch.float64: (float("nan"), -4096.0)}


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)._lib


@pytest.fixture(scope="module")
def aug():
    return importlib.import_module(PKG + ".dataset.spectogram.augment")


class Guards:
    """output buffers: a sentinel inside, a canary region on both sides (offset: extra elements in front, to move the alignment)"""

    def __init__(self):
        self.bufs = []

    def new(self, dtype, *shape, offset=0):
        n = int(np.prod(shape))
        inside, canary = FILL[dtype]
        lo = GUARD + offset
        buf = torch.full((n + lo + GUARD,), canary, dtype=dtype, device="cuda")
        buf[lo:lo + n] = inside
        self.bufs.append((buf, lo, n, canary))
        return buf[lo:lo + n].view(shape)

    def intact(self):
        torch.cuda.synchronize()
        for buf, lo, n, canary in self.bufs:
            assert bool((buf[:lo] == canary).all()) and bool((buf[lo + n:] == canary).all()), "write outside an output buffer"


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, offset=0):
    """numpy -> device copy whose first element sits `offset` elements past an aligned allocation"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device="cuda")
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def run_augment(L, bank, tab, T, F, nt, nf, mean=None, std=None, gain=None, mask_value=0.0, events=None, label_mix=0, offset=0):
    """through the C ABI into guarded buffers -> (out (B, T, F) float32, ev (B, T, K) float64 or None) as numpy"""
    tab = np.ascontiguousarray(tab, dtype=np.int32)
    B = tab.shape[0]
    assert tab.shape[1] == L.lib().sed_logmel_augment_row_ints(nt, nf)
    g = Guards()
    ins = {"bank": (bank, dev(bank, offset)), "tab": (tab, dev(tab))}
    for name, a in (("mean", mean), ("std", std), ("gain", gain), ("events", events)):
        if a is not None:
            ins[name] = (a, dev(a))
    d = {k: v[1] for k, v in ins.items()}
    K = 0 if events is None else events.shape[1]
    out = g.new(torch.float32, B, T, F, offset=offset)
    ev = None if events is None else g.new(torch.float64, B, T, K)
    if offset:
        assert d["bank"].data_ptr() % 16 != 0 and out.data_ptr() % 16 != 0
    else:
        assert d["bank"].data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    L.check(L.lib().sed_logmel_augment(L.ptr(d["bank"]), bank.shape[0], L.ptr(d.get("events")), K, L.ptr(d.get("mean")),
                                       L.ptr(d.get("std")), tab.ctypes.data, L.ptr(d["tab"]), L.ptr(d.get("gain")),
                                       float(mask_value), label_mix, L.ptr(out), L.ptr(ev), B, T, F, nt, nf, stream()),
            "logmel_augment")
    g.intact()
    for name, (host, device) in ins.items():
        assert np.array_equal(device.cpu().numpy(), host, equal_nan=True), f"the input {name} was modified"
    return out.cpu().numpy(), (None if ev is None else ev.cpu().numpy())


def check(got, got_ev, v, mask_value, label_mix, gain_given, tag=""):
    """the module docstring's rules against the stage values of augment_vectorised"""
    assert not np.isnan(got).any(), ("an output cell was not written", tag)
    mv = np.float32(mask_value)
    assert np.array_equal(got[v.masked], np.full(int(v.masked.sum()), mv, dtype=np.float32)), ("masked cells", tag)
    free = ~v.masked
    plain = free & ~v.mixed[:, None, None]
    assert np.array_equal(got[plain], v.u32[plain]), ("cells without mixup", tag)
    np.testing.assert_allclose(v.z32, v.z64, rtol=1e-6, atol=1e-6)
    if not gain_given:
        np.testing.assert_allclose(got[plain], v.out[plain], rtol=1e-6, atol=1e-6, err_msg=str(tag))
    mixed = free & v.mixed[:, None, None]
    err = np.abs(got[mixed].astype(np.float64) - v.mix64[mixed])
    assert (err <= v.bound[mixed]).all(), ("mixup cells", tag, float((err / np.maximum(v.bound[mixed], 1e-300)).max()))
    if v.ev is not None:
        assert not np.isnan(got_ev).any(), ("a label cell was not written", tag)
        assert np.array_equal(got_ev[~v.mixed], v.ev[~v.mixed]), ("labels without mixup", tag)
        if label_mix == 0:
            assert np.array_equal(got_ev[v.mixed], v.ev[v.mixed]), ("max labels", tag)
        else:
            assert (np.abs(got_ev[v.mixed] - v.ev[v.mixed]) <= 4 * 2.0 ** -53 * np.abs(v.ev[v.mixed])).all(), ("soft labels", tag)


# ---- inputs and tables -----------------------------------------------------------------------------------------------------------
def make_bank(rng, frames, F, K=None, soft=False):
    bank = (10 * rng.standard_normal((frames, F)) - 30).astype(np.float32)
    mean = (rng.standard_normal(F) - 30).astype(np.float32)
    std = (5 + 5 * rng.random(F)).astype(np.float32)
    events = None
    if K:
        events = rng.random((frames, K)) if soft else (rng.random((frames, K)) < 0.4).astype(np.float64)
    return bank, mean, std, events


def intervals(rng, axis, n, b, whole=False):
    """n intervals of row b.  The fixed patterns: [0, w), [axis - w, axis), width 0 (also at t0 = axis), two overlapping ones; every
    third row carries width-0 intervals only, so that unmasked cells remain at every size; whole: the first one covers the axis."""
    w = max(1, axis // 4)
    a = axis // 3
    second = min(a + max(1, w // 2), axis - 1)
    pats = [(0, w), (axis - w, w), (axis // 2, 0), (a, min(w, axis - a)), (second, min(w, axis - second)), (axis, 0)]
    while len(pats) < 8:
        t0 = int(rng.integers(0, axis))
        pats.append((t0, int(rng.integers(0, min(max(1, axis // 8), axis - t0) + 1))))
    if b % 3 == 2:
        out = [(int(rng.integers(0, axis + 1)), 0) for _ in range(n)]
    else:
        out = [pats[(b + j) % len(pats)] for j in range(n)]
    if whole and n:
        out[0] = (0, axis)
    return out


def make_table(rng, B, T, F, nt, nf, frames, mix, whole_t=None, whole_f=None):
    """starts at 0 and at frames - T; shifts 0, 1, T - 1; partners: self at B = 1, a 3-cycle at B = 3, at larger B sample 0 is the
    partner of two others and every fourth sample stays alone; lam in [0.5, 1], one 0.3, and at B > 3 one 0.0 and one 1.0"""
    rows = []
    for b in range(B):
        start = 0 if (b == 0 and B > 1) else frames - T if b == B - 1 else int(rng.integers(0, frames - T + 1))
        shift = [0, 1 % T, T - 1][b % 3]
        partner, lam = b, 1.0
        if mix and B == 3:
            partner, lam = (b + 1) % 3, [float(rng.uniform(0.5, 1.0)), 0.3, 0.5][b]
        elif mix and B > 3:
            partner = 0 if b in (1, 2) else b if (b % 4 == 3 or b == 0) else (b * 7 + 3) % B
            lam = 1.0 if partner == b else 0.3 if b == 1 else 0.0 if b == 4 else 1.0 if b == 5 else float(rng.uniform(0.5, 1.0))
        rows.append(make_row(start, shift, partner, lam, intervals(rng, T, nt, b, whole_t == b),
                             intervals(rng, F, nf, b + 1, whole_f == b)))
    return np.array(rows, dtype=np.int32)


TS = [1, 2, 30, 257]
FS = [1, 3, 40, 64, 256]


# ---- everything off ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("F", FS)
def test_everything_off_is_the_crop(L, T, F):
    rng = np.random.default_rng(100 * T + F)
    frames, B = 3 * T + 5, 3
    bank, mean, std, events = make_bank(rng, frames, F, K=1)
    tab = make_table(rng, B, T, F, 0, 0, frames, mix=False)
    tab[:, 1] = 0
    raw = np.stack([bank[s:s + T] for s in tab[:, 0]])
    got, ev = run_augment(L, bank, tab, T, F, 0, 0, events=events)
    assert np.array_equal(got, raw)
    assert np.array_equal(ev, np.stack([events[s:s + T] for s in tab[:, 0]]))
    # with mean / std: the z-score at the end-to-end test's tolerance against float64 ...
    got, _ = run_augment(L, bank, tab, T, F, 0, 0, mean=mean, std=std)
    v = augment_vectorised(bank, tab, T, F, 0, 0, mean, std)
    check(got, None, v, 0.0, 0, False, (T, F))
    # ... and the bits of the plain crop launch for the same starts (an identity check, not a correctness reference)
    starts = np.ascontiguousarray(tab[:, 0])
    d_bank, d_starts, d_mean, d_std = dev(bank), dev(starts), dev(mean), dev(std)
    plain = torch.empty((B, T, F), dtype=torch.float32, device="cuda")
    L.check(L.lib().sed_logmel_crops(L.ptr(d_bank), frames, starts.ctypes.data, L.ptr(d_starts), L.ptr(d_mean), L.ptr(d_std),
                                     L.ptr(plain), B, T, F, stream()), "logmel_crops")
    torch.cuda.synchronize()
    assert np.array_equal(got.view(np.int32), plain.cpu().numpy().view(np.int32))


# ---- shift, gain, masks; no mixup: every cell exact ---------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("F", FS)
def test_shift_gain_masks_exact(L, T, F):
    rng = np.random.default_rng(200 * T + F)
    frames, B = 3 * T + 5, 3
    bank, mean, std, events = make_bank(rng, frames, F, K=3)
    gain = rng.uniform(-1.5, 1.5, (B, F)).astype(np.float32)
    for nt, nf, zscore, with_gain, mv in ((2, 2, True, True, -1.5), (5, 5, False, True, 0.0), (2, 0, True, False, 0.0),
                                          (0, 2, False, False, -1.5)):
        tab = make_table(rng, B, T, F, nt, nf, frames, mix=False)
        m, s = (mean, std) if zscore else (None, None)
        g = gain if with_gain else None
        got, ev = run_augment(L, bank, tab, T, F, nt, nf, m, s, g, mv, events, 0)
        v = augment_vectorised(bank, tab, T, F, nt, nf, m, s, g, mv, events, 0)
        check(got, ev, v, mv, 0, with_gain, (T, F, nt, nf))
        assert set(tab[:, 1]) == {0, 1 % T, T - 1} and tab[0, 0] == 0 and tab[-1, 0] == frames - T


# ---- mixup ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("F", FS)
def test_mixup_three_cycle(L, T, F):
    rng = np.random.default_rng(300 * T + F)
    frames, B = 3 * T + 5, 3
    gain = rng.uniform(-1.5, 1.5, (B, F)).astype(np.float32)
    for K, label_mix, zscore, with_gain, nt, nf in ((1, 0, False, False, 0, 0), (3, 1, True, True, 2, 2), (3, 0, False, True, 1, 1)):
        bank, mean, std, events = make_bank(rng, frames, F, K=K, soft=label_mix == 1)
        tab = make_table(rng, B, T, F, nt, nf, frames, mix=True)
        assert np.array_equal(tab[:, 2], [1, 2, 0])
        m, s = (mean, std) if zscore else (None, None)
        g = gain if with_gain else None
        got, ev = run_augment(L, bank, tab, T, F, nt, nf, m, s, g, -1.5, events, label_mix)
        v = augment_vectorised(bank, tab, T, F, nt, nf, m, s, g, -1.5, events, label_mix)
        check(got, ev, v, -1.5, label_mix, with_gain, (T, F, K, label_mix))


@pytest.mark.parametrize("B", [1, 32])
@pytest.mark.parametrize("T,F", [(30, 64), (257, 40), (2, 3)])
def test_batch_sizes_and_shared_partner(L, B, T, F):
    rng = np.random.default_rng(400 * T + F + B)
    frames = 5 * T + 9
    bank, mean, std, events = make_bank(rng, frames, F, K=3, soft=True)
    gain = rng.uniform(-1.5, 1.5, (B, F)).astype(np.float32)
    tab = make_table(rng, B, T, F, 2, 2, frames, mix=True)
    if B == 1:
        assert tab[0, 2] == 0 and tab[0, 0] == frames - T
    else:
        assert tab[1, 2] == 0 and tab[2, 2] == 0 and (tab[:, 2] == np.arange(B)).sum() >= 8
        lam = table_lam(tab)
        assert lam[1] == np.float32(0.3) and lam[4] == 0.0 and lam[5] == 1.0 and tab[4, 2] != 4 and tab[5, 2] != 5
    for label_mix in (0, 1):
        got, ev = run_augment(L, bank, tab, T, F, 2, 2, mean, std, gain, 0.0, events, label_mix)
        v = augment_vectorised(bank, tab, T, F, 2, 2, mean, std, gain, 0.0, events, label_mix)
        check(got, ev, v, 0.0, label_mix, True, (B, T, F, label_mix))


# ---- mask edge cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,F", [(30, 64), (257, 3), (2, 40), (1, 256), (30, 1)])
def test_eight_masks_whole_axis_and_no_labels(L, T, F):
    rng = np.random.default_rng(500 * T + F)
    frames, B = 3 * T + 5, 3
    bank, mean, std, _ = make_bank(rng, frames, F)
    gain = rng.uniform(-1.5, 1.5, (B, F)).astype(np.float32)
    for whole_t, whole_f in ((None, None), (0, None), (None, 1)):
        tab = make_table(rng, B, T, F, 8, 8, frames, mix=True, whole_t=whole_t, whole_f=whole_f)
        got, ev = run_augment(L, bank, tab, T, F, 8, 8, mean, std, gain, -1.5)            # events = NULL
        v = augment_vectorised(bank, tab, T, F, 8, 8, mean, std, gain, -1.5)
        assert ev is None
        check(got, None, v, -1.5, 0, True, (T, F, whole_t, whole_f))
        if whole_t is not None:
            assert v.masked[whole_t].all() and np.array_equal(got[whole_t], np.full((T, F), -1.5, dtype=np.float32))
        if whole_f is not None:
            assert v.masked[whole_f].all()
    # hand-written intervals on one sample: [0, w), [T - w, T), width 0, two overlapping ones
    if T >= 30:
        tm = [(0, 4), (T - 4, 4), (10, 0), (12, 5), (14, 6), (T, 0), (0, 0), (20, 1)]
        fm = [(0, 1), (F - 1, 1), (0, 0), (F, 0)] + [(F // 2, min(3, F - F // 2)), (min(F - 1, F // 2 + 1), min(3, F - min(F - 1, F // 2 + 1)))] * 2
        tab = np.array([make_row(0, 1, 0, 1.0, tm, fm)], dtype=np.int32)
        got, _ = run_augment(L, bank, tab, T, F, 8, 8, None, None, None, -1.5)
        trow = np.zeros(T, dtype=bool)
        for t0, w in tm:
            trow[t0:t0 + w] = True
        assert trow.sum() == 4 + 4 + 8 + 1
        frow = np.zeros(F, dtype=bool)
        for f0, w in fm:
            frow[f0:f0 + w] = True
        want = np.roll(bank[:T], 1, axis=0).copy()
        want[trow, :] = np.float32(-1.5)
        want[:, frow] = np.float32(-1.5)
        assert np.array_equal(got[0], want)


def test_gain_null_equals_a_zero_table(L):
    rng = np.random.default_rng(6)
    for T, F in ((30, 64), (7, 3)):
        frames, B = 3 * T + 5, 3
        bank, mean, std, events = make_bank(rng, frames, F, K=1)
        tab = make_table(rng, B, T, F, 2, 2, frames, mix=True)
        a, ea = run_augment(L, bank, tab, T, F, 2, 2, mean, std, None, 0.0, events, 0)
        b, eb = run_augment(L, bank, tab, T, F, 2, 2, mean, std, np.zeros((B, F), dtype=np.float32), 0.0, events, 0)
        assert np.array_equal(a, b) and np.array_equal(ea, eb)


# ---- float4-eligible widths on buffers one float off the alignment: the element-wise path, the same results --------------------------
@pytest.mark.parametrize("F", [40, 64, 256])
def test_unaligned_buffers_take_the_scalar_path(L, F):
    rng = np.random.default_rng(700 + F)
    T, B = 30, 3
    frames = 3 * T + 5
    bank, mean, std, events = make_bank(rng, frames, F, K=1, soft=True)
    gain = rng.uniform(-1.5, 1.5, (B, F)).astype(np.float32)
    for mix in (True, False):
        tab = make_table(rng, B, T, F, 2, 2, frames, mix=mix)
        v = augment_vectorised(bank, tab, T, F, 2, 2, mean, std, gain, -1.5, events, 1)
        got1, ev1 = run_augment(L, bank, tab, T, F, 2, 2, mean, std, gain, -1.5, events, 1, offset=1)
        check(got1, ev1, v, -1.5, 1, True, ("offset", F, mix))
        got0, ev0 = run_augment(L, bank, tab, T, F, 2, 2, mean, std, gain, -1.5, events, 1, offset=0)
        check(got0, ev0, v, -1.5, 1, True, ("aligned", F, mix))
        if not mix:
            assert np.array_equal(got0, got1) and np.array_equal(ev0, ev1)


# ---- at size ----------------------------------------------------------------------------------------------------------------------
def test_at_size_everything_on(L):
    rng = np.random.default_rng(8)
    B, T, F, K, frames = 32, 6001, 64, 1, 40000
    bank, mean, std, events = make_bank(rng, frames, F, K=K, soft=True)
    gain = rng.uniform(-1.5, 1.5, (B, F)).astype(np.float32)
    tab = make_table(rng, B, T, F, 2, 2, frames, mix=True)
    perm = np.roll(np.arange(B), 5)
    tab[:, 2] = perm                                                   # mixup on every sample
    tab[:, 3] = rng.uniform(0.5, 1.0, B).astype(np.float32).view(np.int32)
    tab[:, 1] = rng.integers(0, T, B)
    tab[0, 1], tab[1, 1] = 0, T - 1
    got, ev = run_augment(L, bank, tab, T, F, 2, 2, mean, std, gain, 0.0, events, 1)
    v = augment_vectorised(bank, tab, T, F, 2, 2, mean, std, gain, 0.0, events, 1)
    assert v.mixed.all() and 0.01 < v.masked.mean() < 0.9
    check(got, ev, v, 0.0, 1, True, "at size")


# ---- upper layers -------------------------------------------------------------------------------------------------------------------
def full_config(aug, **kw):
    base = dict(time_masks=2, time_mask_frames=6, freq_masks=2, freq_mask_bins=10, time_shift=True, mixup_prob=0.7,
                mixup_alpha=0.4, label_mix="soft", filter_prob=0.7, mask_value=-1.5)
    base.update(kw)
    return aug.SpecAugmentConfig(**base)


def check_layer(x_out, y_out, bank, events, tab, gain, cfg, T, F, mean=None, std=None, tag=""):
    v = augment_vectorised(bank, tab, T, F, cfg.time_masks, cfg.freq_masks, mean, std, gain, cfg.mask_value, events,
                           cfg.label_mix_code)
    check(x_out.cpu().numpy()[:, 0], y_out.double().cpu().numpy(), v, cfg.mask_value, cfg.label_mix_code, gain is not None, tag)
    return v


def test_logmel_augment_callable(aug):
    cfg = full_config(aug)
    fn = aug.LogMelAugment(cfg)
    rng = np.random.default_rng(9)
    B, T, F, K = 4, 30, 64, 2
    x_h = (10 * rng.standard_normal((B, 1, T, F)) - 30).astype(np.float32)
    y_h = rng.random((B, T, K))
    x, y = torch.from_numpy(x_h).cuda(), torch.from_numpy(y_h).cuda()
    np.random.seed(21)
    x2, y2 = fn(x, y)
    assert x2.shape == x.shape and x2.dtype == torch.float32 and y2.shape == y.shape and y2.dtype == torch.float64
    assert x2.data_ptr() != x.data_ptr() and y2.data_ptr() != y.data_ptr()
    assert np.array_equal(x.cpu().numpy(), x_h) and np.array_equal(y.cpu().numpy(), y_h), "the inputs were modified"
    tab, gain = fn.last_tab, fn.last_gain
    assert np.array_equal(tab[:, 0], np.arange(B) * T) and gain is not None and gain.shape == (B, F)
    v = check_layer(x2, y2, x_h.reshape(B * T, F), y_h.reshape(B * T, K), tab, gain, cfg, T, F, tag="callable")
    assert v.mixed.any() and v.masked.any() and (tab[:, 1] > 0).any()
    # the same seed draws the same tables and gives the same bits
    np.random.seed(21)
    x3, y3 = fn(x, y)
    assert torch.equal(x2, x3) and torch.equal(y2, y3)
    # float32 labels come back as float32: the double result, rounded once
    np.random.seed(21)
    x4, y4 = fn(x, y.float())
    assert y4.dtype == torch.float32 and torch.equal(x4, x2)
    ref = augment_vectorised(x_h.reshape(B * T, F), tab, T, F, 2, 2, None, None, gain, -1.5,
                             y_h.astype(np.float32).astype(np.float64).reshape(B * T, K), 1).ev
    assert (np.abs(y4.double().cpu().numpy() - ref) <= (2.0 ** -24 + 4 * 2.0 ** -53) * np.abs(ref)).all()
    # the all-zero config is the identity
    x5, y5 = aug.LogMelAugment(aug.SpecAugmentConfig())(x, y)
    assert torch.equal(x5, x) and torch.equal(y5, y) and x5.data_ptr() != x.data_ptr()


def _complex_bank(rng, frames, bins):
    return (rng.standard_normal((frames, bins)) + 1j * rng.standard_normal((frames, bins))).astype(np.complex64)


def _write_dataset(root, mode, cfg, rng, n=4, frames=(70, 64, 90, 75)):
    d = os.path.join(root, f"{mode}-features_and_labels")
    os.makedirs(d, exist_ok=True)
    allf = []
    for i in range(n):
        T = frames[i]
        if mode == "logMel":
            f = (10 * rng.standard_normal((1, T, cfg.mel_bins)) - 30).astype(np.float32)
        else:
            f = _complex_bank(rng, T, cfg.bins)[None] * np.float32(5.0)
        allf.append(f)
        with open(os.path.join(d, f"rec{i}_{mode}_features_and_labels.pkl"), "wb") as fh:
            pickle.dump({"features": f, "start_times": [3.0 + i, 15.0], "end_times": [4.0 + i, 16.5]}, fh)
    cat = np.concatenate(allf, axis=1)
    ms = os.path.join(root, f"{mode}-features_mean_std.pkl")
    with open(ms, "wb") as fh:
        pickle.dump({"mean": np.mean(cat, axis=(0, 1)), "std": np.std(cat, axis=(0, 1))}, fh)
    return d, ms


@pytest.mark.parametrize("mode", ["logMel", "Complex"])
def test_spectogram_dataset_with_spec_augment(L, aug, tmp_path, mode):
    sc = importlib.import_module(PKG + ".dataset.spectogram.spectogram_configs")
    dsm = importlib.import_module(PKG + ".dataset.spectogram.spectograms_dataset")
    tr = importlib.import_module(PKG + ".train")
    sed = importlib.import_module(PKG)
    cfg = sc.SpectogramConfig(3000, 1000, 1000, 1024)          # fps 3 -> crop 30 frames, 513 bins, 64 mel bins
    d, ms = _write_dataset(str(tmp_path), mode, cfg, np.random.default_rng(2))
    acfg = full_config(aug)
    mix = mode == "Complex"                                     # the reference's own mix + noise run in front of the second launch

    def build(spec_augment):
        np.random.seed(0)
        return dsm.SpectogramDataset(d, ms, val_descriptor="rec3", augment_data=mix, preprocessed_mode=mode, cfg=cfg,
                                     spec_augment=spec_augment)

    plain, augd, ident = build(None), build(acfg), build(aug.SpecAugmentConfig())
    assert np.array_equal(plain.train_start_indices, augd.train_start_indices)
    idx = list(range(3, 11))
    B, T, F = len(idx), 30, 64
    np.random.seed(33)
    x0, y0 = plain.device_batch(idx)
    np.random.seed(33)
    x1, y1 = augd.device_batch(idx)
    np.random.seed(33)
    x2, y2 = ident.device_batch(idx)
    assert x1.shape == (B, 1, T, F) and x1.dtype == torch.float32 and y1.shape == (B, T, 1) and y1.dtype == torch.float64
    assert torch.equal(x2, x0) and torch.equal(y2, y0), "the all-zero config is the identity"
    tab, gain = augd.last_tab, augd.last_gain
    if mode == "logMel":
        files = sorted(p for p in os.listdir(d) if "rec3" not in p)
        feats = np.concatenate([pickle.load(open(os.path.join(d, p), "rb"))["features"] for p in files], axis=1)[0]
        msd = pickle.load(open(ms, "rb"))
        mean = np.broadcast_to(msd["mean"], (F,)).astype(np.float32)
        std = np.broadcast_to(msd["std"], (F,)).astype(np.float32)
        assert np.array_equal(tab[:, 0], plain.train_start_indices[idx])
        v = check_layer(x1, y1, feats, plain.train_event_matrix, tab, gain, acfg, T, F, mean, std, tag=mode)
        # spec_augment=None launches the parent's sed_logmel_crops: its bits for the same starts
        starts = np.ascontiguousarray(tab[:, 0])
        want = torch.empty((B, T, F), dtype=torch.float32, device="cuda")
        L.check(L.lib().sed_logmel_crops(L.ptr(plain.bank), plain.bank_frames, starts.ctypes.data, L.ptr(dev(starts)),
                                         L.ptr(plain.d_mean), L.ptr(plain.d_std), L.ptr(want), B, T, F, stream()), "logmel_crops")
        assert torch.equal(x0[:, 0], want)
        assert np.array_equal(y0.cpu().numpy(), np.stack([plain.train_event_matrix[s:s + T] for s in starts]))
        # the band gain is drawn in dB and divided by the z-score's std
        assert np.abs(gain.astype(np.float64) * std[None, :]).max() <= 6 + 1e-4
    else:
        assert np.array_equal(tab[:, 0], np.arange(B) * T)
        v = check_layer(x1, y1, x0.cpu().numpy().reshape(B * T, F), y0.cpu().numpy().reshape(B * T, 1), tab, gain, acfg, T, F,
                        tag=mode)
    assert v.mixed.any() and v.masked.any()
    # validation never augments
    for (fa, ea, na), (fb, eb, nb) in zip(plain.get_validation_sampler(3), augd.get_validation_sampler(3)):
        assert torch.equal(fa, fb) and torch.equal(ea, eb) and na == nb and fa.shape == (1, 1, 75, 64)
    # train() on the augmented loader: six steps, a finite loss, its checkpoint
    loader = dsm.DeviceBatchLoader(augd, 32)
    model = sed.Cnn_AvgPooling(1, [(8, 2), (16, 2), (16, 2), (16, 1)])
    tr.train(model, loader, sed.WeightedBCE(5, True), num_steps=6, lr=1e-3, log_freq=3, outputs_dir=str(tmp_path / "out"),
             device="cuda")
    assert os.path.exists(tmp_path / "out" / "checkpoints" / "iteration_6.pth")
    rec = [__import__("json").loads(ln) for ln in open(tmp_path / "out" / "progress.jsonl")]
    assert len(rec) == 2 and all(np.isfinite(r["train_loss"]) for r in rec)


def test_train_batch_augment_on_the_synthetic_dataset(aug, tmp_path):
    from torch.utils.data import DataLoader
    sed = importlib.import_module(PKG)
    tr = importlib.import_module(PKG + ".train")
    syn = importlib.import_module(PKG + ".dataset.synthetic")
    ds = syn.SyntheticSedDataset(n_train_crops=16, crop=32, n_val=1, val_frames=64)
    fn = aug.LogMelAugment(full_config(aug))
    calls = []

    def counted(x, y):
        calls.append((tuple(x.shape), x.is_cuda))
        return fn(x, y)

    model = sed.Cnn_AvgPooling(1, [(8, 2), (16, 2), (16, 2), (16, 1)])
    np.random.seed(4)
    tr.train(model, DataLoader(ds, batch_size=4, num_workers=0), sed.WeightedBCE(5, True), num_steps=3, lr=1e-3, log_freq=3,
             outputs_dir=str(tmp_path / "out"), device="cuda", batch_augment=counted)
    assert calls == [((4, 1, 32, 64), True)] * 3 and fn.last_tab.shape == (4, 12)
    rec = [__import__("json").loads(ln) for ln in open(tmp_path / "out" / "progress.jsonl")]
    assert len(rec) == 1 and np.isfinite(rec[0]["train_loss"])
    assert os.path.exists(tmp_path / "out" / "checkpoints" / "iteration_3.pth")
