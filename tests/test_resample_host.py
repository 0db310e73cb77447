"""CPU-only: the host half of the audio ingest (dataset/dataset_utils.py) -- the numpy filter design against scipy.signal.firwin, the
float64 formula the GPU tests use as their reference (tests/resample_formula.py) against scipy.signal.resample_poly, the phase-major
table sed_resample_poly reads, the ratio helper, range errors on both sides of the C ABI (argument checks fire before any launch), and
read_multichannel_audio without a device against the formula it has always used."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from resample_formula import n_out_of, resample_formula

PKG = "soundeventdetection-pytorch_amd"
RATIOS = [(2, 3), (3, 2), (160, 147), (320, 441), (1, 2), (147, 320), (640, 147)]
RATES = [8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 96000]


@pytest.fixture(scope="module")
def du():
    return importlib.import_module(PKG + ".dataset.dataset_utils")


@pytest.mark.parametrize("up,down", RATIOS)
def test_filter_matches_firwin(du, up, down):
    from scipy.signal import firwin
    half = 10 * max(up, down)
    ref = firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    h = du.resample_filter(up, down)
    assert h.dtype == np.float64 and h.shape == ref.shape
    assert np.abs(h - ref).max() <= 1e-15


@pytest.mark.parametrize("up,down", RATIOS)
def test_formula_matches_resample_poly(du, up, down):
    from scipy.signal import resample_poly
    h = torch.from_numpy(du.resample_filter(up, down))
    rng = np.random.default_rng(up * 1000 + down)
    for n_in in (1, 7, 33, 1000):
        x = rng.uniform(-1.0, 1.0, n_in)
        y, S, taps = resample_formula(torch.from_numpy(x), h, up, down)
        ref = resample_poly(x, up, down)
        assert y.shape == ref.shape == (n_out_of(n_in, up, down),)
        assert np.abs(y.numpy() - ref).max() <= 1e-14, (n_in, np.abs(y.numpy() - ref).max())
        assert int(taps.min()) >= 1 and bool((S >= y.abs() - 1e-15).all())


@pytest.mark.parametrize("up,down", RATIOS + [(1, 640), (640, 1), (1, 6)])
def test_phase_table_layout(du, up, down):
    h = du.resample_filter(up, down)
    tab = du.resample_phases(up, down)
    tp = 20 * max(up, down) // up + 1
    assert tab.dtype == np.float32 and tab.shape == (up, tp | 1) and tab.flags.c_contiguous
    for p in {0, 1 % up, up // 2, up - 1}:
        row = h[p::up].astype(np.float32)
        assert np.array_equal(tab[p, :row.size], row) and not tab[p, row.size:].any()


def test_resample_ratio(du):
    from fractions import Fraction
    for s in RATES:
        for d in RATES:
            up, down = du.resample_ratio(s, d)
            assert Fraction(up, down) == Fraction(d, s) and np.gcd(up, down) == 1
            # every pair of these rates is inside the supported range but 11.025 kHz against 32 or 96 kHz (1280 / 441, 1280 / 147)
            if {s, d} in ({11025, 32000}, {11025, 96000}):
                assert max(up, down) == 1280
                with pytest.raises(ValueError, match="supported range"):
                    du.resample_filter(up, down)
            else:
                assert max(up, down) <= du.MAX_RESAMPLE_RATIO, (s, d)
                assert du.resample_filter(up, down).size == 20 * max(up, down) + 1
    assert du.resample_ratio(48000, 32000) == (2, 3) and du.resample_ratio(44100, 48000) == (160, 147)
    assert du.resample_ratio(32000, 32000) == (1, 1)
    assert du.resampled_length(20011, 2, 3) == 13341 and du.resampled_length(3, 2, 3) == 2


def test_range_errors(du):
    for bad in ((641, 1), (1, 641), (2, 4), (0, 1), (3, -2)):
        with pytest.raises(ValueError):
            du.resample_filter(*bad)
    with pytest.raises(ValueError):
        du.resample_ratio(0, 48000)
    with pytest.raises(ValueError):
        du.resample_ratio(44100.5, 48000)
    with pytest.raises(ValueError, match="supported range"):
        du.resample_filter(*du.resample_ratio(44100, 47999))
    with pytest.raises(RuntimeError, match="MI355X"):
        du.AudioIngest("cpu")
    L = importlib.import_module(PKG)._lib
    lib = L.lib()
    tp, tile = C.c_int(-1), C.c_int(-1)
    assert lib.sed_resample_plan(2, 3, C.byref(tp), C.byref(tile)) == 0 and tp.value == 31 and tile.value % 256 == 0
    assert lib.sed_resample_plan(641, 1, None, None) != 0 and b"1..640" in lib.sed_last_error()
    assert lib.sed_resample_plan(4, 6, None, None) != 0 and b"coprime" in lib.sed_last_error()
    # argument checks of the launch entry point come before anything touches the device (dummy non-null pointers, never used)
    P = 4096
    ok = dict(dt=L.PCM_I16, pcm=P, taps=P, out=P, B=1, n_in=9, n_out=6, ci=2, co=1, up=2, down=3)
    for change, text in ((dict(dt=3), b"dtype"), (dict(dt=-1), b"dtype"), (dict(pcm=None), b"null"), (dict(out=None), b"null"),
                         (dict(taps=None), b"null"), (dict(up=4, down=6), b"coprime"), (dict(up=641, down=3, n_out=1923), b"1..640"),
                         (dict(up=0), b"1..640"), (dict(down=0), b"1..640"), (dict(n_out=5), b"n_out"), (dict(n_out=7), b"n_out"),
                         (dict(n_in=0, n_out=0), b"frame"), (dict(B=0), b"B in"), (dict(ci=0), b"channels"),
                         (dict(co=65), b"channels")):
        a = dict(ok, **change)
        rc = lib.sed_resample_poly(a["dt"], a["pcm"], a["taps"], a["out"], a["B"], a["n_in"], a["n_out"], a["ci"], a["co"], a["up"],
                                   a["down"], None)
        assert rc != 0 and text in lib.sed_last_error(), (change, lib.sed_last_error())


def test_read_multichannel_audio_without_device_is_the_host_path(du, tmp_path):
    """decode / channel rule / scipy.signal.resample_poly per channel in float64, as before the device path existed"""
    import dataclasses
    from scipy.io import wavfile
    from scipy.signal import resample_poly
    rng = np.random.default_rng(5)
    pcm = rng.integers(-32768, 32768, size=(2205, 2), dtype=np.int16)
    p = str(tmp_path / "s.wav")
    wavfile.write(p, 44100, pcm)
    a = du.read_multichannel_audio(p, target_fs=48000)
    mono = (pcm.astype(np.float64) / 32768.0).mean(1)
    assert a.dtype == np.float64 and a.shape == (2400, 1)
    assert np.array_equal(a[:, 0], resample_poly(mono, 160, 147))
    assert np.array_equal(du.read_multichannel_audio(p, target_fs=None)[:, 0], mono)
    cfg4 = dataclasses.replace(du.REF_NATIVE, audio_channels=4)
    b = du.read_multichannel_audio(p, target_fs=32000, cfg=cfg4)
    assert b.shape == (1600, 4)
    for c in range(4):
        assert np.array_equal(b[:, c], resample_poly(mono, 320, 441))
    cfg2 = dataclasses.replace(du.REF_NATIVE, audio_channels=2)
    c2 = du.read_multichannel_audio(p, target_fs=44100, cfg=cfg2)
    assert np.array_equal(c2, pcm.astype(np.float64) / 32768.0)
