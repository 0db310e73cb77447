"""GPU: the audio ingest kernel of csrc/sed_resample.hip (PCM decode + channel downmix + polyphase resampler) through the C ABI,
per element against float64, and the layers on top of it (AudioIngest, read_multichannel_audio(device=...), LogMelFrontEnd(source_rate=...),
infer_file).

Reference: tests/resample_formula.py in float64 (torch on the device) -- y[m] = sum_k h[m*down + half - k*up] * x[k] with h from
scipy.signal.firwin and x the exactly decoded, downmixed samples; the formula is checked against scipy.signal.resample_poly in
tests/test_resample_host.py.  No kernel of this library serves as a reference.  Every output starts as NaN inside a buffer with a canary
region on both sides.

Gate, per element: |got - ref| <= SAFE * (taps + 3) * u * S, u = 2^-24, SAFE = 4, taps = the number of terms present for that output,
S = sum |h_k| |x_k| in float64: the dot-product bound in any summation order; + 3 = the rounding of h to fp32, the downmix rounding
and the final store.  An output whose bound is 0 must be exact.  Nothing here was set from a measurement.
  unit impulse   x = -1 (int16 -32768) or +1 (float32) at one frame: every product and every sum with zeros is exact, so besides the
                 gate the output must be the fp32 tap (float)h[m*down + half - k*up] (negated for int16) bit for bit.
  up = down = 1  integer PCM: float32(float64 host formula) bit for bit -- exact integer channel sum, scaling and division in fp64,
                 one rounding.  float32 PCM: within one fp32 ulp (numpy's float64 mean and the kernel's may add in another order).
  ratios         2/3, 3/2, 1/2, 1/6, 160/147, 320/441, 147/320, 640/147 at n_in 1, 7, T - 1 (T = taps per phase), 4097, 20011;
                 plus 1/640 and 3/250, whose input span exceeds the staging buffer (the chunked path), and 640/1 (the widest table).

Measured max err / gate on the MI355X (printed per case with -s, summarised at the end of the module; 0.25 = the operation count
without its safety factor):
  ratios         0.06 .. 0.15 over every ratio, dtype, length, batch and channel map: worst 0.146 (640/1, int32), 0.125 (640/147,
                 float32), 0.123 (2/3, int32); the chunked path 0.03 .. 0.065 (1/640, 3/250)
  unit impulse   0.002 .. 0.016 against float64 (the rounding of the one tap), and the fp32 taps bit for bit
  up = down = 1  integer PCM bit-equal, float32 PCM within one ulp, every channel map
  read_multichannel_audio(device=) against the float64 host path, 44.1 -> 48 kHz int16 stereo: 0.063
No case missed its gate.  The module runs in about 6 s.
"""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from resample_formula import downmix, n_out_of, resample_formula, term_indices

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
I16, I32, F32 = 0, 1, 2
NP = {I16: np.int16, I32: np.int32, F32: np.float32}
U = 2.0 ** -24
SAFE = 4.0
GUARD = 1024
CANARY = -1024.0
RATIOS = [(2, 3), (3, 2), (1, 2), (1, 6), (160, 147), (320, 441), (147, 320), (640, 147)]
EXTRA = [(1, 640), (3, 250), (640, 1)]
CHMAPS = [(1, 1), (2, 1), (3, 1), (4, 1), (1, 2), (4, 2), (4, 4)]
WORST = {}


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)._lib


@pytest.fixture(scope="module")
def du():
    return importlib.import_module(PKG + ".dataset.dataset_utils")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nmax err / gate by case (1.0 = at the derived bound)")
        for k in sorted(WORST):
            print(f"  {k:40s} {WORST[k]:.3e}")


class Guards:
    """output buffers: NaN inside, a canary region on both sides, checked by intact()"""

    def __init__(self):
        self.bufs = []

    def new(self, *shape):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.float32, device="cuda")
        buf[GUARD:GUARD + n] = float("nan")
        self.bufs.append((buf, n))
        return buf[GUARD:GUARD + n].view(shape)

    def intact(self):
        torch.cuda.synchronize()
        for buf, n in self.bufs:
            assert bool((buf[:GUARD] == CANARY).all()) and bool((buf[GUARD + n:] == CANARY).all()), "write outside an output buffer"


def gate(what, got, ref, bound):
    got = got.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: an element is NaN/inf (not written)"
    err = (got - ref).abs()
    pos = bound > 0
    assert bool((err[~pos] == 0).all()), f"{what}: an element whose bound is 0 is not exactly the reference"
    r = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    key = what.split(" n_in")[0]
    WORST[key] = max(WORST.get(key, 0.0), r)
    print(f"    {what:64s} max err/gate {r:.3e}")
    assert r <= 1.0, f"{what}: max err/gate {r:.3e} > 1"


def ref_filter(up, down):
    from scipy.signal import firwin
    half = 10 * max(up, down)
    return torch.from_numpy(firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up).cuda()


def make_pcm(rng, dt, B, n, ch):
    """full-range PCM with the full-scale values planted (-32768 / INT32_MIN and the positive maximum, +-1.0f)"""
    if dt == F32:
        x = rng.uniform(-1.0, 1.0, (B, n, ch)).astype(np.float32)
        lo, hi = -1.0, 1.0
    else:
        info = np.iinfo(NP[dt])
        x = rng.integers(info.min, info.max, (B, n, ch), dtype=NP[dt], endpoint=True)
        lo, hi = info.min, info.max
    flat = x.reshape(-1)
    pos = rng.integers(0, flat.size, 6)
    flat[pos[:3]] = lo
    flat[pos[3:]] = hi
    if n >= 2:
        x[:, 0, :] = lo                      # a whole frame at negative full scale: the mean is exactly -1
        x[:, n - 1, :] = hi
    return x


def taps_per_phase(up, down):
    return 20 * max(up, down) // up + 1


def plan(L, up, down):
    tp, tile = C.c_int(0), C.c_int(0)
    assert L.lib().sed_resample_plan(up, down, C.byref(tp), C.byref(tile)) == 0
    return tp.value, tile.value


def call(L, dt, pcm_t, taps_t, out, ch_out, up, down, n_out=None):
    B, n_in, ch_in = pcm_t.shape
    n_out = n_out_of(n_in, up, down) if n_out is None else n_out
    return L.lib().sed_resample_poly(dt, L.ptr(pcm_t), L.ptr(taps_t), L.ptr(out), B, n_in, n_out, ch_in, ch_out, up, down,
                                     torch.cuda.current_stream().cuda_stream)


def check_case(L, what, dt, pcm, ch_out, up, down, taps_t, h64, idx):
    B, n_in, _ = pcm.shape
    G = Guards()
    out = G.new(B, ch_out, n_out_of(n_in, up, down))
    L.check(call(L, dt, torch.from_numpy(pcm).cuda(), taps_t, out, ch_out, up, down), what)
    G.intact()
    x64 = torch.from_numpy(downmix(pcm, ch_out)).cuda()
    ref, S, taps = resample_formula(x64, h64, up, down, idx)
    assert int(taps.min()) >= 1
    gate(what, out, ref, SAFE * (taps.double() + 3.0) * U * S)


@pytest.mark.parametrize("dt", [I16, I32, F32], ids=["i16", "i32", "f32"])
@pytest.mark.parametrize("up,down", RATIOS + EXTRA, ids=lambda v: str(v))
def test_resample_against_float64(L, du, up, down, dt):
    extra = (up, down) in EXTRA
    T = taps_per_phase(up, down)
    sizes = [1, 7, 1000] if (up, down) == (640, 1) else [1, 7, max(1, T - 1), 4097, 20011]
    chmaps = [(1, 1), (2, 1), (4, 2)] if extra else CHMAPS
    taps_t = torch.from_numpy(du.resample_phases(up, down)).cuda()
    h64 = ref_filter(up, down)
    rng = np.random.default_rng(1000 * up + down + 7 * dt)
    for n_in in sizes:
        idx = term_indices(up, down, n_in, "cuda")
        for B in (1, 3):
            for ch_in, ch_out in chmaps:
                pcm = make_pcm(rng, dt, B, n_in, ch_in)
                check_case(L, f"{up}/{down} {('i16', 'i32', 'f32')[dt]} n_in {n_in} B {B} ch {ch_in}->{ch_out}", dt, pcm, ch_out, up, down,
                           taps_t, h64, idx)


@pytest.mark.parametrize("up,down", RATIOS, ids=lambda v: str(v))
def test_unit_impulse_reproduces_the_taps(L, du, up, down):
    """an impulse inside the first, an interior and the last tile (one per row): the fp32 taps, exactly"""
    _, tile = plan(L, up, down)
    n_out = 3 * tile + tile // 2 + 1
    n_in = -(-n_out * down // up)
    n_out = n_out_of(n_in, up, down)
    assert n_out > 3 * tile
    ks = [min(3, n_in - 1), int((1.5 * tile) * down / up), n_in - 2]            # outputs around m = k * up / down
    assert ks[0] * up // down < tile < ks[1] * up // down < 2 * tile and ks[2] * up // down >= (n_out - 1) // tile * tile
    h = du.resample_filter(up, down)
    h32 = torch.from_numpy(h.astype(np.float32)).cuda()
    taps_t = torch.from_numpy(du.resample_phases(up, down)).cuda()
    half = 10 * max(up, down)
    m = torch.arange(n_out, dtype=torch.int64, device="cuda")
    for dt, amp, sign in ((I16, -32768, -1.0), (F32, 1.0, 1.0)):
        pcm = np.zeros((3, n_in, 1), dtype=NP[dt])
        for r, k in enumerate(ks):
            pcm[r, k, 0] = amp
        G = Guards()
        out = G.new(3, 1, n_out)
        L.check(call(L, dt, torch.from_numpy(pcm).cuda(), taps_t, out, 1, up, down), "impulse")
        G.intact()
        x64 = torch.from_numpy(downmix(pcm, 1)).cuda()
        ref, S, taps = resample_formula(x64, ref_filter(up, down), up, down)
        gate(f"{up}/{down} impulse {('i16', 'i32', 'f32')[dt]}", out, ref, SAFE * (taps.double() + 3.0) * U * S)
        for r, k in enumerate(ks):
            j = m * down + half - k * up
            want = torch.where((j >= 0) & (j <= 2 * half), sign * h32[j.clamp(0, 2 * half)], torch.zeros((), device="cuda"))
            assert torch.equal(out[r, 0], want), (dt, k)
            assert bool((want != 0).any())


@pytest.mark.parametrize("dt", [I16, I32, F32], ids=["i16", "i32", "f32"])
def test_decode_and_downmix_alone(L, dt):
    """up == down == 1: no filter (NULL table); integer PCM is float32(host formula) bit for bit, float32 PCM within one ulp"""
    rng = np.random.default_rng(50 + dt)
    for n_in in (1, 255, 257, 4097):
        for B in (1, 3):
            for ch_in, ch_out in CHMAPS:
                pcm = make_pcm(rng, dt, B, n_in, ch_in)
                G = Guards()
                out = G.new(B, ch_out, n_in)
                L.check(call(L, dt, torch.from_numpy(pcm).cuda(), None, out, ch_out, 1, 1), "ingest")
                G.intact()
                want = downmix(pcm, ch_out).astype(np.float32)
                got = out.cpu().numpy()
                if dt == F32:
                    assert np.isfinite(got).all() and (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))).all()
                else:
                    assert np.array_equal(got, want), (n_in, B, ch_in, ch_out)


def test_error_codes_write_nothing(L, du):
    up, down, n_in = 2, 3, 301
    taps_t = torch.from_numpy(du.resample_phases(up, down)).cuda()
    pcm = torch.zeros((2, n_in, 2), dtype=torch.int16, device="cuda")
    G = Guards()
    out = G.new(2, 1, n_out_of(n_in, up, down))
    lib, s = L.lib(), torch.cuda.current_stream().cuda_stream
    ok = dict(dt=I16, pcm=L.ptr(pcm), taps=L.ptr(taps_t), out=L.ptr(out), B=2, n_in=n_in, n_out=out.shape[2], ci=2, co=1, up=up, down=down)
    bad = [dict(dt=3), dict(dt=-1), dict(pcm=None), dict(taps=None), dict(out=None), dict(up=4, down=6), dict(up=641, down=3),
           dict(up=2, down=641), dict(up=0), dict(down=-3), dict(n_out=out.shape[2] - 1), dict(n_out=out.shape[2] + 1), dict(n_in=0),
           dict(B=0), dict(B=65536), dict(ci=0), dict(ci=65), dict(co=0), dict(co=65)]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.sed_resample_poly(a["dt"], a["pcm"], a["taps"], a["out"], a["B"], a["n_in"], a["n_out"], a["ci"], a["co"], a["up"],
                                   a["down"], s)
        assert rc != 0 and lib.sed_last_error(), change
        with pytest.raises(RuntimeError):
            L.check(rc, "resample_poly")
    G.intact()
    assert bool(torch.isnan(out).all()), "an entry point that returned an error wrote to its output"
    L.check(lib.sed_resample_poly(*[ok[k] for k in ("dt", "pcm", "taps", "out", "B", "n_in", "n_out", "ci", "co", "up", "down")], s), "ok")
    G.intact()
    assert bool((out == 0).all())


def test_audio_ingest_is_the_c_abi(L, du):
    rng = np.random.default_rng(9)
    ing = du.AudioIngest("cuda", ch_out=2)
    pcm = make_pcm(rng, I16, 3, 5000, 4)
    for k, (src, dst) in enumerate(((48000, 32000), (44100, 48000), (48000, 32000), (32000, 32000))):
        up, down = du.resample_ratio(src, dst)
        G = Guards()
        want = G.new(3, 2, n_out_of(5000, up, down))
        taps_t = None if up == down == 1 else torch.from_numpy(du.resample_phases(up, down)).cuda()
        L.check(call(L, I16, torch.from_numpy(pcm).cuda(), taps_t, want, 2, up, down), "c abi")
        G.intact()
        got = ing(pcm if k % 2 == 0 else torch.from_numpy(pcm).cuda(), src, dst)
        assert got.dtype == torch.float32 and got.is_cuda and torch.equal(got, want), (src, dst)
        one = ing(pcm[1], src, dst)
        assert one.shape == want.shape[1:] and torch.equal(one, want[1])
    assert sorted(ing._taps) == [(2, 3), (160, 147)]
    with pytest.raises(TypeError):
        ing(pcm.astype(np.float64), 48000, 32000)
    with pytest.raises(ValueError, match="supported range"):
        ing(pcm, 44100, 47999)


def test_read_multichannel_audio_on_the_device(L, du, tmp_path):
    from scipy.io import wavfile
    rng = np.random.default_rng(21)
    pcm = make_pcm(rng, I16, 1, 22050, 2)[0]
    p = str(tmp_path / "half_second.wav")
    wavfile.write(p, 44100, pcm)
    host = du.read_multichannel_audio(p, target_fs=48000)                       # float64, scipy
    dev = du.read_multichannel_audio(p, target_fs=48000, device="cuda")
    assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (1, 24000) == host.T.shape
    x64 = torch.from_numpy(downmix(pcm[None], 1)).cuda()
    _, S, taps = resample_formula(x64, ref_filter(160, 147), 160, 147)
    gate("read_multichannel_audio 44.1 -> 48 kHz", dev[None], torch.from_numpy(host.T.copy()).cuda()[None], SAFE * (taps.double() + 3.0) * U * S)
    same = du.read_multichannel_audio(p, target_fs=44100, device="cuda")
    assert np.array_equal(same.cpu().numpy(), du.read_multichannel_audio(p, target_fs=44100).T.astype(np.float32))
    wavfile.write(p, 44100, (pcm[:2000].astype(np.float64) / 32768.0))           # float64 file: host path, then copied
    f64 = du.read_multichannel_audio(p, target_fs=48000, device="cuda")
    assert np.array_equal(f64.cpu().numpy(), du.read_multichannel_audio(p, target_fs=48000).T.astype(np.float32))


def test_frontend_with_a_source_rate(du):
    pp = importlib.import_module(PKG + ".dataset.spectogram.preprocess")
    sc = importlib.import_module(PKG + ".dataset.spectogram.spectogram_configs")
    w = torch.randn(2, 24000, generator=torch.Generator().manual_seed(3)).cuda() * 0.1
    fe48 = pp.LogMelFrontEnd(sc.BENCH, source_rate=48000)
    fe = pp.LogMelFrontEnd(sc.BENCH)
    resampled = du.AudioIngest("cuda", 1)(w.unsqueeze(-1), 48000, 32000).view(2, -1).clone()
    assert resampled.shape == (2, 16000)
    got = fe48(w)
    assert fe48.num_frames(24000) == sc.BENCH.num_frames(16000) == got.shape[2]
    assert torch.equal(got, fe(resampled))
    assert torch.equal(fe48.stft(w), fe.stft(resampled))
    pf = pp.PrefetchingFrontEnd(fe48)
    pf.submit(w)
    assert torch.equal(pf.get(), got)
    pf.release()
    same = pp.LogMelFrontEnd(sc.BENCH, source_rate=32000)
    assert same.num_frames(24000) == sc.BENCH.num_frames(24000) and torch.equal(same(w), fe(w))


def test_infer_file_resamples_on_the_device(tmp_path):
    """a 48 kHz recording through the 32 kHz bench configuration: device ingest against host_resample=True"""
    from scipy.io import wavfile
    sed = importlib.import_module(PKG)
    infer = importlib.import_module(PKG + ".infer")
    sc = importlib.import_module(PKG + ".dataset.spectogram.spectogram_configs")
    rng = np.random.default_rng(4)
    n = 48000 * 3
    wav = 0.05 * rng.standard_normal(n)
    for s in range(12000, n - 24000, 40000):
        wav[s:s + 12000] += 0.4 * np.sin(2 * np.pi * 700.0 * np.arange(12000) / 48000.0)
    p = str(tmp_path / "clip48k.wav")
    wavfile.write(p, 48000, (np.stack([wav, 0.5 * wav], axis=1).clip(-1, 1) * 32767).astype(np.int16))
    torch.manual_seed(0)
    model = sed.Cnn_AvgPooling(1, [(32, 2), (64, 2), (128, 2), (128, 1)])
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for name, b in model.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g) * 0.3)
            elif name.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g) * 1.5 + 0.3)
    ck = str(tmp_path / "m.pth")
    torch.save({"iterations": 0, "model": model.state_dict()}, ck)
    dev = infer.infer_file(p, ck, precision="fp32", cfg=sc.BENCH)
    host = infer.infer_file(p, ck, precision="fp32", cfg=sc.BENCH, host_resample=True)
    T = sc.BENCH.num_frames(32000 * 3)
    assert dev["log_mel"].shape == host["log_mel"].shape == (T, 64)
    assert dev["probabilities"].shape == host["probabilities"].shape and dev["probabilities"].shape[0] > 0
    assert np.array_equal(dev["decisions"], host["decisions"])
    np.testing.assert_allclose(dev["probabilities"], host["probabilities"], atol=1e-3, rtol=0)     # tests/test_gpu_parity.py, fp32
    infer.main([p, "--ckpt", ck, "--outputs_dir", str(tmp_path / "o"), "--precision", "fp32", "--config", "bench", "--host_resample"])
    z = np.load(tmp_path / "o" / "clip48k.npz")
    assert np.array_equal(z["probabilities"], host["probabilities"])
