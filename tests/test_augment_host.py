"""Host side of the log-mel batch augmentation (no GPU): the tests' formula (tests/augment_formula.py) in its two forms, the host
draws of dataset/spectogram/augment.py, the CLI flags, and every argument refusal of sed_logmel_augment through the built library.
The refusal cases pass a real host table and NULL for `out` and the device table, so a validation bug would end in the null-pointer
refusal and never in a launch."""
import ctypes as C
import importlib
import inspect
import os
from types import SimpleNamespace

import numpy as np
import pytest

from augment_formula import augment_formula, augment_vectorised, make_row, table_lam
from conftest import ROOT

PKG = "soundeventdetection-pytorch_amd"
LIB = os.path.join(ROOT, PKG, "libsed_hip.so")


@pytest.fixture(scope="module")
def sed():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def aug():
    return importlib.import_module(PKG + ".dataset.spectogram.augment")


# ---- the formula in its two forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zscore,with_gain,label_mix", [(False, False, 0), (True, True, 1), (True, False, 0), (False, True, 1)])
def test_formula_loops_equal_vectorised(zscore, with_gain, label_mix):
    rng = np.random.default_rng(7)
    B, T, F, K, frames = 4, 7, 5, 2, 40
    bank = (10 * rng.standard_normal((frames, F)) - 30).astype(np.float32)
    events = rng.random((frames, K))
    mean = rng.standard_normal(F).astype(np.float32) - 30 if zscore else None
    std = (5 + rng.random(F)).astype(np.float32) if zscore else None
    gain = rng.uniform(-1, 1, (B, F)).astype(np.float32) if with_gain else None
    tab = np.array([make_row(0, 0, 1, 0.75, [(0, 2), (6, 1)], [(1, 2)]),
                    make_row(frames - T, 1, 2, 0.5, [(3, 0), (2, 3)], [(0, 0)]),
                    make_row(11, T - 1, 0, 1.0, [(3, 2), (4, 2)], [(4, 1)]),
                    make_row(20, 3, 3, 1.0, [(0, 0), (0, 0)], [(0, 5)])], dtype=np.int32)
    out, ev = augment_formula(bank, tab, T, F, 2, 1, mean, std, gain, -1.5, events, label_mix)
    v = augment_vectorised(bank, tab, T, F, 2, 1, mean, std, gain, -1.5, events, label_mix)
    assert np.array_equal(out, v.out) and np.array_equal(ev, v.ev)
    assert np.array_equal(v.mixed, [True, True, True, False]) and v.masked[3].all() and not v.masked[1, :, 0].all()
    assert np.array_equal(v.masked[0, :, 0], [True, True, False, False, False, False, True])
    # the fp32 stages sit at fp32 rounding distance of the float64 formula, the bound dominates the fp32 / float64 gap of the mix
    np.testing.assert_allclose(v.z32, v.z64, rtol=1e-6, atol=1e-6)
    free = ~v.masked & ~v.mixed[:, None, None]
    np.testing.assert_allclose(v.u32[free], v.out[free], rtol=1e-6, atol=1e-6)
    assert v.u32.dtype == np.float32 and (v.bound >= 0).all()
    # hand-checked cells: sample 2 shifts by T - 1 = -1 frame and mixes with sample 0 under lam = 1 (identity weights)
    z = (lambda r, f: (float(bank[r, f]) - float(mean[f])) / float(std[f])) if zscore else (lambda r, f: float(bank[r, f]))
    g = (lambda b, f: float(gain[b, f])) if with_gain else (lambda b, f: 0.0)
    assert out[2, 0, 0] == 1.0 * (z(11 + 1, 0) + g(2, 0)) + 0.0 * (z(0, 0) + g(0, 0))
    assert out[1, 0, 2] == 0.5 * (z(frames - T + T - 1, 2) + g(1, 2)) + 0.5 * (z(11 + 1, 2) + g(2, 2))
    assert out[0, 0, 0] == -1.5 and out[0, 3, 1] == -1.5 and out[0, 3, 3] != -1.5
    e10 = (events[frames - 1, 1], events[12, 1])
    assert ev[1, 0, 1] == (max(e10) if label_mix == 0 else 0.5 * e10[0] + 0.5 * e10[1])
    assert ev[0, 0, 0] == (max(events[0, 0], events[frames - 1, 0]) if label_mix == 0 else
                           0.75 * events[0, 0] + 0.25 * events[frames - 1, 0])         # masks do not touch labels


def test_formula_without_labels_and_table_helpers():
    bank = np.arange(12, dtype=np.float32).reshape(6, 2)
    tab = np.array([make_row(1, 2, 0, 1.0)], dtype=np.int32)
    out, ev = augment_formula(bank, tab, 3, 2, 0, 0)
    assert ev is None and np.array_equal(out[0, :, 0], [4.0, 6.0, 2.0])          # u[t] = z[(t - 2) mod 3]
    assert augment_vectorised(bank, tab, 3, 2, 0, 0).ev is None
    assert table_lam(np.array([make_row(0, lam=0.625)], dtype=np.int32))[0] == np.float32(0.625)


# ---- the host draws --------------------------------------------------------------------------------------------------------------
def full_config(aug, **kw):
    base = dict(time_masks=3, time_mask_frames=9, freq_masks=2, freq_mask_bins=70, time_shift=True, mixup_prob=0.6,
                mixup_alpha=0.4, label_mix="soft", filter_prob=0.7)
    base.update(kw)
    return aug.SpecAugmentConfig(**base)


def test_draw_is_reproducible_and_inside_the_axes(aug):
    cfg = full_config(aug)
    B, T, F = 32, 30, 64
    starts = np.arange(B) * 17
    std_mel = np.linspace(2.0, 9.0, F)
    np.random.seed(123)
    tab, gain = aug.draw(cfg, starts, T, F, std_mel=std_mel)
    np.random.seed(123)
    tab2, gain2 = aug.draw(cfg, starts, T, F, std_mel=std_mel)
    tab3, _ = aug.draw(cfg, starts, T, F, std_mel=std_mel)
    assert np.array_equal(tab, tab2) and np.array_equal(gain, gain2) and not np.array_equal(tab, tab3)
    assert tab.dtype == np.int32 and tab.shape == (B, aug.row_ints(cfg)) == (B, 4 + 2 * 5)
    assert gain.dtype == np.float32 and gain.shape == (B, F)
    assert np.array_equal(tab[:, 0], starts)
    assert ((tab[:, 1] >= 0) & (tab[:, 1] < T)).all() and len(set(tab[:, 1])) > 4
    t0, tw = tab[:, 4:10:2], tab[:, 5:10:2]
    f0, fw = tab[:, 10:14:2], tab[:, 11:14:2]
    assert (t0 >= 0).all() and (tw >= 0).all() and (tw <= 9).all() and (t0 + tw <= T).all()
    assert (f0 >= 0).all() and (fw >= 0).all() and (fw <= F).all() and (f0 + fw <= F).all()       # 70 bins are clipped to the axis
    lam = table_lam(tab)
    mixed = tab[:, 2] != np.arange(B)
    assert ((tab[:, 2] >= 0) & (tab[:, 2] < B)).all() and 4 < mixed.sum() < B
    assert (lam[~mixed] == 1.0).all() and (lam >= 0.5).all() and (lam <= 1.0).all() and (lam[mixed] < 1.0).any()
    # band gains: inside filter_db / std, zero rows where the coin said no, piecewise linear in dB
    db = gain.astype(np.float64) * std_mel[None, :]
    assert (db >= -6 - 1e-5).all() and (db <= 6 + 1e-5).all()
    rows_on = np.abs(db).max(axis=1) > 0
    assert 8 < rows_on.sum() < B
    kinks = np.abs(np.diff(db[rows_on], n=2, axis=1)) > 1e-4
    assert (kinks.sum(axis=1) <= 5).all()                   # at most hi - 1 = 5 interior knots


def test_draw_with_mixup_off_and_identity_config(aug):
    np.random.seed(5)
    tab, gain = aug.draw(full_config(aug, mixup_prob=0.0, filter_prob=0.0), np.arange(6), 30, 64)
    assert gain is None and np.array_equal(tab[:, 2], np.arange(6)) and (table_lam(tab) == 1.0).all()
    # the all-zero config: the identity table, no gain, and not one call to the RNG
    cfg = aug.SpecAugmentConfig()
    np.random.seed(9)
    state = np.random.get_state()[1].copy()
    tab, gain = aug.draw(cfg, [4, 0, 9], 30, 64)
    assert gain is None and aug.row_ints(cfg) == 4
    assert np.array_equal(tab, [make_row(4, 0, 0, 1.0), make_row(0, 0, 1, 1.0), make_row(9, 0, 2, 1.0)])
    assert np.array_equal(np.random.get_state()[1], state)
    # tiny axes
    np.random.seed(2)
    tab, gain = aug.draw(full_config(aug, filter_prob=1.0), [0], 1, 1)
    assert tab[0, 1] == 0 and gain.shape == (1, 1) and (tab[0, 5::2] <= 1).all()
    tab, gain = aug.draw(full_config(aug, filter_prob=1.0), [0, 1], 2, 2)
    assert gain.shape == (2, 2) and np.isfinite(gain).all()


def test_config_refuses_bad_values(aug):
    for bad in (dict(time_masks=-1), dict(time_masks=9), dict(freq_masks=9), dict(freq_mask_bins=-2), dict(mixup_prob=1.5),
                dict(mixup_prob=-0.1), dict(filter_prob=2.0), dict(mixup_alpha=0.0), dict(label_mix="mean"),
                dict(filter_bands=(0, 3)), dict(filter_bands=(4, 3)), dict(filter_db=(3.0, -3.0)), dict(mask_value=float("nan")),
                dict(time_mask_frames=1.5)):
        with pytest.raises(ValueError):
            aug.SpecAugmentConfig(**bad)
    assert aug.SpecAugmentConfig(time_masks=8, freq_masks=8).label_mix_code == 0
    assert aug.SpecAugmentConfig(label_mix="soft").label_mix_code == 1


def test_logmel_augment_refuses_cpu_tensors(aug):
    import torch
    with pytest.raises(RuntimeError, match="no CPU path"):
        aug.LogMelAugment(aug.SpecAugmentConfig())(torch.zeros(2, 1, 30, 64), torch.zeros(2, 30, 1))


# ---- CLI -------------------------------------------------------------------------------------------------------------------------
def test_cli_flags_defaults_and_refusals(aug):
    main = importlib.import_module(PKG + ".main")
    train = importlib.import_module(PKG + ".train")
    a = main.build_full_parser().parse_args([])
    assert a.spec_augment is False and main.spec_augment_config(a) is None and main.synthetic_batch_augment(a) is None
    assert (a.time_masks, a.time_mask_frames, a.freq_masks, a.freq_mask_bins) == (2, 4, 2, 8)
    assert (a.time_shift, a.mixup_prob, a.mixup_alpha, a.soft_labels, a.filter_augment) == (False, 0.0, 0.2, False, 0.0)
    assert vars(a).items() >= vars(main.build_parser().parse_args([])).items()          # every training flag, same defaults
    assert not hasattr(main.build_parser().parse_args([]), "spec_augment")
    main.validate_args(a)
    # a Namespace built by hand, without any of the new names
    bare = main.build_parser().parse_args([])
    main.validate_args(bare)
    assert main.spec_augment_config(bare) is None
    assert main.spec_augment_config(SimpleNamespace(spec_augment=True)) == aug.SpecAugmentConfig(
        time_masks=2, time_mask_frames=4, freq_masks=2, freq_mask_bins=8)
    a = main.build_full_parser().parse_args(["--train_features", "Spectogram", "--dataset_name", "synthetic", "--spec_augment",
                                             "--time_masks", "3", "--time_mask_frames", "20", "--freq_masks", "1",
                                             "--freq_mask_bins", "12", "--time_shift", "--mixup_prob", "0.5", "--mixup_alpha", "0.3",
                                             "--soft_labels", "--filter_augment", "0.25"])
    main.validate_args(a)
    assert main.spec_augment_config(a) == aug.SpecAugmentConfig(
        time_masks=3, time_mask_frames=20, freq_masks=1, freq_mask_bins=12, time_shift=True, mixup_prob=0.5, mixup_alpha=0.3,
        label_mix="soft", filter_prob=0.25)
    assert isinstance(main.synthetic_batch_augment(a), aug.LogMelAugment)
    a.dataset_name = "TAU"
    assert main.synthetic_batch_augment(a) is None               # the spectrogram datasets augment in their own launch
    for name, bad in (("time_masks", -1), ("time_mask_frames", -3), ("freq_masks", -1), ("freq_mask_bins", -1),
                      ("mixup_prob", -0.5), ("mixup_prob", 1.5), ("mixup_alpha", -1.0), ("filter_augment", -0.1),
                      ("filter_augment", 1.01), ("mixup_prob", float("nan")), ("time_masks", 9)):
        b = main.build_full_parser().parse_args(["--train_features", "Spectogram", "--spec_augment"])
        setattr(b, name, bad)
        with pytest.raises(ValueError):
            main.validate_args(b)
    with pytest.raises(ValueError, match="Spectogram"):
        main.validate_args(main.build_full_parser().parse_args(["--train_features", "Waveform", "--spec_augment"]))
    main.validate_args(main.build_full_parser().parse_args(["--train_features", "Waveform"]))
    assert inspect.signature(train.train).parameters["batch_augment"].default is None
    assert inspect.signature(train.train).parameters["batch_augment"].kind is inspect.Parameter.KEYWORD_ONLY
    ds = importlib.import_module(PKG + ".dataset.spectogram.spectograms_dataset")
    assert inspect.signature(ds.SpectogramDataset.__init__).parameters["spec_augment"].default is None


# ---- the C ABI refuses bad arguments before any launch ---------------------------------------------------------------------------
def test_argument_validation_without_gpu(sed):
    lib = sed._lib.lib()
    assert lib.sed_logmel_augment_row_ints(0, 0) == 4 and lib.sed_logmel_augment_row_ints(8, 8) == 36
    assert lib.sed_logmel_augment_row_ints(2, 3) == 14
    B, T, F, K, frames, nt, nf = 3, 6, 8, 2, 40, 2, 1
    # host memory standing in for the device buffers: never touched, every call below is refused first
    bank, gain = (C.c_float * (frames * F))(), (C.c_float * (B * F))()
    events, ev_out = (C.c_double * (frames * K))(), (C.c_double * (B * T * K))()
    mean, std = (C.c_float * F)(), (C.c_float * F)()
    good = np.array([make_row(0, 0, 1, 0.75, [(0, 2), (4, 2)], [(1, 7)]),
                     make_row(frames - T, T - 1, 2, 0.5, [(0, 0), (0, T)], [(0, F)]),
                     make_row(5, 1, 2, 1.0, [(T, 0), (2, 2)], [(F, 0)])], dtype=np.int32)
    assert good.shape == (B, lib.sed_logmel_augment_row_ints(nt, nf))

    def call(tab=good, bank_p=C.addressof(bank), bank_frames=frames, events_p=C.addressof(events), K_=K,
             mean_p=C.addressof(mean), std_p=C.addressof(std), gain_p=C.addressof(gain), label_mix=0, out_p=None,
             ev_out_p=C.addressof(ev_out), B_=B, T_=T, F_=F, nt_=nt, nf_=nf, tab_host=True):
        tab = np.ascontiguousarray(tab, dtype=np.int32)
        return lib.sed_logmel_augment(bank_p, bank_frames, events_p, K_, mean_p, std_p, tab.ctypes.data if tab_host else None,
                                      None, gain_p, 0.0, label_mix, out_p, ev_out_p, B_, T_, F_, nt_, nf_, None)

    def refused(rc, word):
        assert rc != 0 and word in lib.sed_last_error(), (rc, word, lib.sed_last_error())

    def edit(r, c, v):
        t = good.copy()
        t[r, c] = v
        return t

    nan_bits = int(np.array([np.nan], dtype=np.float32).view(np.int32)[0])
    bits = lambda x: int(np.array([x], dtype=np.float32).view(np.int32)[0])          # noqa: E731
    # a valid call with out = tab = NULL passes every check and stops at the last one
    refused(call(), b"null")
    refused(call(B_=0), b"bad sizes")
    refused(call(T_=0), b"bad sizes")
    refused(call(F_=-1), b"bad sizes")
    refused(call(bank_frames=0), b"bad sizes")
    refused(call(nt_=9), b"at most 8")
    refused(call(nf_=9), b"at most 8")
    refused(call(nt_=-1), b"at most 8")
    refused(call(edit(0, 0, frames - T + 1)), b"outside the feature bank")
    refused(call(edit(2, 0, -1)), b"outside the feature bank")
    refused(call(edit(1, 1, T)), b"shift")
    refused(call(edit(1, 1, -1)), b"shift")
    refused(call(edit(0, 2, B)), b"partner")
    refused(call(edit(0, 2, -1)), b"partner")
    refused(call(edit(0, 3, nan_bits)), b"lam")
    refused(call(edit(0, 3, bits(1.0000001))), b"lam")
    refused(call(edit(0, 3, bits(-0.25))), b"lam")
    refused(call(edit(0, 4, -1)), b"time mask")
    refused(call(edit(0, 5, -1)), b"time mask")
    refused(call(edit(1, 6, 1)), b"time mask")                     # t0 + w = 1 + T
    refused(call(edit(2, 7, T)), b"time mask")
    refused(call(edit(0, 8, -1)), b"frequency mask")
    refused(call(edit(0, 9, -2)), b"frequency mask")
    refused(call(edit(0, 9, F)), b"frequency mask")                # f0 + w = 1 + F
    refused(call(edit(0, 4, 2 ** 31 - 1)), b"time mask")           # t0 + w must not wrap
    refused(call(mean_p=None), b"mean/std")
    refused(call(std_p=None), b"mean/std")
    refused(call(ev_out_p=None), b"ev_out")
    refused(call(K_=0), b"K > 0")
    refused(call(K_=-2), b"K > 0")
    refused(call(label_mix=2), b"label_mix")
    refused(call(bank_p=None), b"null")
    refused(call(tab_host=False), b"null")
    refused(call(out_p=C.addressof(bank)), b"overlaps the feature bank")
    refused(call(out_p=C.addressof(bank) + 4 * (frames * F - 1)), b"overlaps the feature bank")
    refused(call(out_p=C.addressof(gain) + 4), b"overlaps the gain")
    refused(call(events_p=C.addressof(ev_out) + 8), b"overlaps the label bank")
    # without labels K and ev_out do not matter; without mean / std, gain: still only the null refusal
    refused(call(events_p=None, K_=0, ev_out_p=None, mean_p=None, std_p=None, gain_p=None), b"null")
    with pytest.raises(RuntimeError, match="shift"):
        sed._lib.check(call(edit(1, 1, T)), "logmel_augment")
