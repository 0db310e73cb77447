"""GPU: every route of the log-mel front-end (csrc/sed_frontend.hip: launch_front, sed_complex_to_logmel, sed_logmel_crops) per element
against float64, through the C ABI.  Reference, gate and their derivation: tests/frontend_formula.py (checked without a GPU in
tests/test_frontend_formula_host.py: the gate accepts a plain fp32 radix-2 implementation and rejects every mutated reference).

Constants (derived there, fixed before the first GPU run): C_FFT = 8, C_LEAK = 4, C_BIN = 8 (STFT); C_POW = 2, C_TREE = 8, C_LOG = 5,
C_Z = 3 plus the band length (log-mel); C_ABS2 = 5 plus a quarter of the band length + 2 (sed_complex_to_logmel).

Which case reaches which route of launch_front() -- `route()` below restates its conditions and every case asserts the route it is
listed under:
  batched   frontend1024c_kernel   BATCHED: log-mel, nfft 1024, n_mels <= 64, hop % 4 == 0, hop <= 320, samples % 4 == 0, samples >= 1024,
                                   16-byte aligned wave, SED_FE_KERNEL unset
  fallback  frontend1024_kernel    FALLBACK, each by one condition: hop 250 / 251 (hop % 4), samples 2562 (samples % 4), hop 324 (> 320),
                                   samples 513 / 1023 (< 1024), wave offset by 1 / 2 floats (alignment), SED_FE_KERNEL=1
  generic   frontend_kernel        GENERIC: log-mel at nfft 64 .. 2048 other than 1024, nfft 1024 with n_mels > 64, SED_FE_KERNEL=g at
                                   4096; every STFT below 4096 (STFT cases)
  big       frontend_big_kernel    BIG: nfft >= 4096, log-mel and STFT
  sed_complex_to_logmel and sed_logmel_crops have one kernel each.
Every output element of every case meets its bound; the buffers carry guard words in front and behind.  The sensitivity cases hand
each mutated reference of frontend_formula.py to the gate with the kernel's own output and require it to fail.

Measured on the MI355X, max err / bound per route (run with -s for the table):
  route      check     max err/bound   margin   where the maximum sits
  batched    log-mel   0.256           3.9x     hop 4, Slaney bank, z-score: one- and two-bin bands, where the log-mel ratio IS the STFT ratio
  fallback   log-mel   0.201           5.0x
  generic    log-mel   0.247           4.0x     nfft 1024, 130 filters
  generic    STFT      0.229           4.4x     SED_FE_KERNEL=g at nfft 4096 (radix-2; the plain fp32 radix-2 FFT on the host: 0.10 .. 0.19)
  big        log-mel   0.132           7.6x
  big        STFT      0.218           4.6x
  complex    log-mel   0.597           1.7x     bands of 1 .. 5 bins: the bound counts these few roundings in the worst case (7.25 u for one
  crops      z-score   0.617           1.6x       bin; 3 u for the crops), there is nothing statistical in it to keep a factor 4 over
  crops      plain     0 (bit-equal)
The batched kernel's 3.9 is the STFT bound's margin seen through single-bin bands (the STFT routes measure 4.4 and 4.6 directly).
What the file found: every route wrote -100.00001 for silence (10 * log10f(1e-10f): the device's log10f is an ulp low there), caught
by the all-zero clip and by the empty filters of the "empty" and "lengths" banks; the kernels now floor the logarithm at exactly -10
(fe_log10: one v_max_f32 more per output, every power above the floor computes what it did before).
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import frontend_formula as FF

pytestmark = pytest.mark.gpu

KNOBS = ("SED_FE_KERNEL", "SED_FE_BLOCKS")
GUARD = 64
RATIOS = {}                     # (route, check) -> max err / bound measured


def route(logmel, nfft, hop, samples, n_mels, offset, env):
    """launch_front()'s choice, restated"""
    fek = env.get("SED_FE_KERNEL", "")
    if logmel and nfft == 1024 and n_mels <= 64:
        if hop <= 320 and hop % 4 == 0 and samples % 4 == 0 and offset % 4 == 0 and samples >= 1024 and fek[:1] != "1":
            return "batched"
        return "fallback"
    if nfft >= 4096 and fek[:1] != "g":
        return "big"
    return "generic"


def _c(route_, nfft, hop, samples, B=2, n_mels=64, bank="random", meanstd=False, env=None, offset=0, **kw):
    return dict(route=route_, nfft=nfft, hop=hop, samples=samples, B=B, n_mels=n_mels, bank=bank, meanstd=meanstd, env=env or {},
                offset=offset, **kw)


# frontend1024c_kernel.  T = 1 + samples // hop; a workgroup takes 8 frames (a batch), bpc = ceil(T / 8) batches per clip.
BATCHED = [
    _c("batched", 1024, 4, 1024, n_mels=16),                                   # T = 257 (T % 8 = 1), 33 batches per clip, shortest clip
    _c("batched", 1024, 4, 1028, bank="slaney", meanstd=True),                 # T = 258
    _c("batched", 1024, 128, 2944, n_mels=17),                                 # T = 24 (T % 8 = 0)
    _c("batched", 1024, 128, 2432, n_mels=40, meanstd=True),                   # batch 1: s0 + 7 hop + 1024 == samples, the 16-byte path at its limit
    _c("batched", 1024, 128, 2428, n_mels=40, meanstd=True),                   # 4 samples shorter: the same batch reflects
    _c("batched", 1024, 252, 1512, n_mels=15),                                 # T = 7 (T % 8 = 7): one batch with a dead wave
    _c("batched", 1024, 320, 2560, bank="slaney", meanstd=True),               # T = 9 (T % 8 = 1), the benchmark's constants and bank
    _c("batched", 1024, 320, 2560, bank="slaney"),
    _c("batched", 1024, 320, 4800, n_mels=1),                                  # T = 16
    _c("batched", 1024, 128, 4096, B=3, bank="slaney", meanstd=True),                                   # 15 batches, one workgroup each
    _c("batched", 1024, 128, 4096, B=3, bank="slaney", meanstd=True, env={"SED_FE_BLOCKS": "1"}),       # one workgroup, 15 passes
    _c("batched", 1024, 128, 4096, B=3, bank="slaney", meanstd=True, env={"SED_FE_BLOCKS": "3"}),       # bpc = 5, grid 3: passes cross clips
    _c("batched", 1024, 252, 2048, bank="empty", width=40, meanstd=True),      # tile 1 empty between tiles 0 and 2; single empty filters
    _c("batched", 1024, 252, 2048, n_mels=40, bank="empty", width=40),         # + tile 3 absent
    _c("batched", 1024, 320, 1028, n_mels=17, bank="dense"),                   # 129 k-steps per tile, 3 waves per tile: 43 > FC_NBR = 24
    _c("batched", 1024, 320, 1028, bank="dense", meanstd=True),                # 2 waves per tile: 65 steps; every band reaches bin 512
    _c("batched", 1024, 320, 2048, B=3, n_mels=40, amps=(0.0, 1.0, 1e-3)),     # a silent clip next to a loud one; a clip at 1e-3
    _c("batched", 1024, 320, 2048, B=3, n_mels=40, amps=(0.0, 1.0, 1e-3), meanstd=True),
]
# frontend1024_kernel: four frames (waves) per workgroup
FALLBACK = [
    _c("fallback", 1024, 250, 2000, B=3, n_mels=40, meanstd=True),             # hop % 4; even hop and samples: 8-byte interior loads; B T = 27 (% 4 = 3)
    _c("fallback", 1024, 250, 2000, B=3, n_mels=40, env={"SED_FE_BLOCKS": "2"}),   # 7 workgroups' worth of frames on a grid of 2
    _c("fallback", 1024, 251, 1507, B=3, n_mels=17, meanstd=True),             # odd: scalar loads; B T = 21 (% 4 = 1)
    _c("fallback", 1024, 320, 2562, bank="slaney"),                            # samples % 4 == 2; B T = 18 (% 4 = 2)
    _c("fallback", 1024, 324, 2592, bank="slaney", meanstd=True),              # hop > 320
    _c("fallback", 1024, 128, 513, n_mels=16),                                 # samples < 1024: the shortest legal clip
    _c("fallback", 1024, 128, 1023, n_mels=16, meanstd=True),
    _c("fallback", 1024, 320, 2560, bank="slaney", offset=1),                  # no alignment: scalar loads
    _c("fallback", 1024, 320, 2560, bank="slaney", offset=2, meanstd=True),    # 8-byte, not 16-byte aligned
    _c("fallback", 1024, 320, 2560, bank="slaney", meanstd=True, env={"SED_FE_KERNEL": "1"}),
    _c("fallback", 1024, 250, 1500, bank="sum:1152"),                          # the compact weight list exactly full
    _c("fallback", 1024, 250, 1500, bank="sum:1153", meanstd=True),            # one more: weights stay in global memory
    _c("fallback", 1024, 250, 1500, n_mels=17, bank="dense"),                  # far over; every band ends at bin 513
    _c("fallback", 1024, 250, 2000, B=3, n_mels=40, amps=(0.0, 1.0, 1e-3), meanstd=True),
]
# frontend_kernel<true>: radix-2, one workgroup per frame; the last filter of a random bank ends at the Nyquist bin (kept in Z[0].y)
GENERIC = [_c("generic", n, n // 3 + 1, 3 * n + 17, n_mels=20, meanstd=(n in (128, 512))) for n in (64, 128, 256, 512, 2048)] + [
    _c("generic", 1024, 320, 2048, n_mels=65),                                 # n_mels > 64 leaves the nfft-1024 kernels
    _c("generic", 1024, 320, 2048, n_mels=128, bank="slaney", meanstd=True),
    _c("generic", 1024, 128, 1500, n_mels=130, width=30),
    _c("generic", 4096, 1366, 9001, n_mels=33, meanstd=True, env={"SED_FE_KERNEL": "g"}),
    _c("generic", 64, 1, 90, n_mels=8, meanstd=True),                          # hop 1
    _c("generic", 128, 200, 700, n_mels=8),                                    # hop > nfft
    _c("generic", 512, 171, 1553, n_mels=20, win_len=300),                     # window shorter than the transform
    _c("generic", 256, 50, 129, n_mels=20, bank="slaney"),                     # samples = nfft / 2 + 1
    _c("generic", 2048, 700, 4100, B=3, n_mels=20, amps=(0.0, 1.0, 1e-3), meanstd=True),
]
# frontend_big_kernel: hop nfft / 3 + 1 and 3 nfft + 123 samples give 9 frames: 0, 1 and 8 reflect, 2 .. 7 are interior (8-byte
# loads where the frame's first sample is 8-byte aligned, scalar loads elsewhere); bands of 256 .. 2048 bins run the four-load loop
BIG = [_c("big", n, n // 3 + 1, 3 * n + 123, n_mels=m, meanstd=ms)
       for n, m, ms in [(4096, 1, False), (4096, 17, True), (4096, 64, False), (8192, 16, True), (8192, 33, False), (16384, 17, False),
                        (16384, 64, True)]] + [
    _c("big", 4096, 1366, 12411, n_mels=64, bank="slaney", sr=44100, win_len=3796),
    _c("big", 4096, 1000, 2049, n_mels=16, meanstd=True),                      # samples = nfft / 2 + 1
    _c("big", 32768, 15840, 20000, n_mels=64, bank="slaney", sr=48000, win_len=31680, meanstd=True),     # two frames, the reference's constants
    _c("big", 8192, 2731, 24699, B=3, n_mels=33, amps=(0.0, 1.0, 1e-3), meanstd=True),
]
STFT = [_c("generic", 64, 22, 209), _c("generic", 64, 1, 90), _c("generic", 256, 86, 785, win_len=200), _c("generic", 256, 50, 129),
        _c("generic", 1024, 320, 2560), _c("generic", 1024, 251, 1507, B=3, amps=(0.0, 1.0, 1e-3)), _c("generic", 2048, 700, 4100),
        _c("generic", 128, 200, 700), _c("generic", 4096, 1366, 9001, env={"SED_FE_KERNEL": "g"}),
        _c("big", 4096, 1366, 12411), _c("big", 4096, 1000, 2049), _c("big", 8192, 2731, 24699, B=3, amps=(0.0, 1.0, 1e-3)),
        _c("big", 16384, 5462, 49275), _c("big", 32768, 15840, 20000, win_len=31680)]


def _id(c):
    s = f"{c['route']}-n{c['nfft']}-h{c['hop']}-s{c['samples']}-B{c['B']}-m{c['n_mels']}-{c['bank'].replace(':', '')}"
    s += "-z" if c["meanstd"] else ""
    s += f"-off{c['offset']}" if c["offset"] else ""
    s += "-amps" if c.get("amps") else ""
    s += f"-w{c['win_len']}" if c.get("win_len") else ""
    return s + "".join(f"-{k[7:]}{v}" for k, v in c["env"].items())


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module("soundeventdetection-pytorch_amd")._lib


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if RATIOS:
        print("\nmax err / bound by route and check (1 = the gate)")
        for k in sorted(RATIOS):
            print(f"  {k[0]:10s} {k[1]:8s} {RATIOS[k]:.3f}   " + (f"(margin {1.0 / RATIOS[k]:.1f}x)" if RATIOS[k] > 0 else "(exact)"))


@pytest.fixture
def knobs(monkeypatch, L):
    """set SED_* knobs for one test (the library caches them: sed_config_reload is the test hook); unset again on teardown"""
    def set_(env):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        L.lib().sed_config_reload()
    yield set_
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    L.lib().sed_config_reload()


def _note(route_, check, r):
    r = float(r)
    RATIOS[(route_, check)] = max(RATIOS.get((route_, check), 0.0), r)
    return r


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


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


def _wave_dev(d, offset):
    """the clips on the device, the first sample `offset` floats behind a 256-byte aligned address"""
    B, n = d["waves"].shape
    flat = torch.zeros(B * n + 8, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 256 == 0
    w = flat[offset:offset + B * n]
    w.copy_(torch.from_numpy(d["waves"].reshape(-1)))
    return w


def _inputs(c):
    kw = {k: c[k] for k in ("amps", "win_len", "width") if k in c}
    d = FF.make_inputs(c["nfft"], c["hop"], c["samples"], c["B"], c["n_mels"], c["bank"], 0, meanstd=c["meanstd"], **kw)
    if c["bank"] == "slaney" and "sr" in c:
        d["W"], d["lo"], d["hi"] = FF.make_bank("slaney", c["n_mels"], c["nfft"] // 2 + 1, sr=c["sr"])
    return d


def run_front(L, c, d, logmel):
    """one call of sed_logmel_fwd / sed_stft_fwd -> the output on the host, (B, T, n_mels) float32 or (B, T, bins) complex64"""
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    B, n, nfft, hop = c["B"], c["samples"], c["nfft"], c["hop"]
    T = 1 + n // hop
    w, win = _wave_dev(d, c["offset"]), _dev(d["window"])
    ws = torch.empty(max(1, lib.sed_logmel_ws_bytes(B, n, nfft, hop) // 4), dtype=torch.float32, device="cuda")
    if logmel:
        W, lo, hi, mean, std = (_dev(d[k]) for k in ("W", "lo", "hi", "mean", "std"))
        out = Guarded(B * T * c["n_mels"])
        L.check(lib.sed_logmel_fwd(w.data_ptr(), L.ptr(win), L.ptr(W), L.ptr(lo), L.ptr(hi), L.ptr(mean), L.ptr(std), out.ptr, L.ptr(ws),
                                   B, n, nfft, hop, c["n_mels"], st), "logmel_fwd")
        return out.numpy().reshape(B, T, c["n_mels"])
    out = Guarded(B * T * (nfft // 2 + 1) * 2)
    L.check(lib.sed_stft_fwd(w.data_ptr(), L.ptr(win), out.ptr, L.ptr(ws), B, n, nfft, hop, st), "stft_fwd")
    return out.numpy().view(np.complex64).reshape(B, T, nfft // 2 + 1)


def _logmel_case(L, knobs, c):
    assert route(True, c["nfft"], c["hop"], c["samples"], c["n_mels"], c["offset"], c["env"]) == c["route"]
    d = _inputs(c)
    k = np.arange(d["W"].shape[1])[None, :]
    assert (d["W"][(k < d["lo"][:, None]) | (k >= d["hi"][:, None])] == 0).all()       # the batched kernel relies on it
    knobs(c["env"])
    got = run_front(L, c, d, True)
    mr = FF.logmel_reference(d["waves"], d["window"], c["nfft"], c["hop"], d["W"], d["lo"], d["hi"], d["mean"], d["std"])
    r = FF.logmel_ratio(got, mr)
    print(f"\n{_id(c)}: max err/bound {_note(c['route'], 'logmel', r.max()):.3f}", end="")
    i = np.unravel_index(r.argmax(), r.shape)
    assert r.max() <= 1.0, f"element {i}: err/bound {r[i]}, got {got[i]!r}, reference {mr.z[i]!r} (mel power {mr.p[i]!r})"


@pytest.mark.parametrize("c", BATCHED, ids=_id)
def test_batched_kernel(L, knobs, c):
    _logmel_case(L, knobs, c)


@pytest.mark.parametrize("c", FALLBACK, ids=_id)
def test_one_wave_per_frame_kernel(L, knobs, c):
    _logmel_case(L, knobs, c)


@pytest.mark.parametrize("c", GENERIC, ids=_id)
def test_generic_radix2_kernel(L, knobs, c):
    _logmel_case(L, knobs, c)


@pytest.mark.parametrize("c", BIG, ids=_id)
def test_large_transform_kernel(L, knobs, c):
    _logmel_case(L, knobs, c)


@pytest.mark.parametrize("c", STFT, ids=_id)
def test_stft(L, knobs, c):
    assert route(False, c["nfft"], c["hop"], c["samples"], 0, 0, c["env"]) == c["route"]
    d = _inputs(dict(c, n_mels=0))
    knobs(c["env"])
    got = run_front(L, c, d, False)
    assert np.isfinite(got.view(np.float32)).all()
    r = FF.stft_ratio(got, FF.Reference(d["waves"], d["window"], c["nfft"], c["hop"]))
    print(f"\n{_id(c)}: max err/bound {_note(c['route'], 'stft', r.max()):.3f}", end="")
    assert r.max() <= 1.0, (np.unravel_index(r.argmax(), r.shape), r.max())


def test_rejected_configurations_return_the_error_code(L):
    lib = L.lib()
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    out = Guarded(64)
    p = buf.data_ptr()
    for B, n, nfft, hop in [(1, 512, 1024, 320), (1, 32, 64, 8), (1, 2000, 1000, 320), (1, 2000, 32, 8), (0, 2000, 1024, 320),
                            (1, 2000, 1024, 0)]:                                 # samples <= nfft / 2; nfft not a power of two / too small; B, hop
        assert lib.sed_logmel_fwd(p, p, p, p, p, None, None, out.ptr, p, B, n, nfft, hop, 1, None) != 0
        assert lib.sed_stft_fwd(p, p, out.ptr, p, B, n, nfft, hop, None) != 0
    assert lib.sed_logmel_fwd(p, p, p, p, p, p, None, out.ptr, p, 1, 2000, 1024, 320, 1, None) != 0      # mean without std
    assert np.isnan(out.numpy()).all()                                            # nothing was launched


# ---- sed_complex_to_logmel -----------------------------------------------------------------------------------------------------------
COMPLEX = [(33, 1, "random", False), (33, 64, "lengths", True), (513, 64, "slaney", True), (513, 65, "lengths", False),
           (513, 130, "random", True), (16385, 64, "lengths", False), (16385, 130, "random", True), (16385, 1, "random", False)]


@pytest.mark.parametrize("bins,n_mels,bank,meanstd", COMPLEX)
def test_complex_to_logmel(L, bins, n_mels, bank, meanstd):
    """bins 16385 crosses the 64 KB LDS opt-in by four bytes; band lengths 0 .. 5 at every lo % 4 (bank "lengths"); a dynamic range
    of 10^6 between bins"""
    rng = np.random.default_rng(bins + n_mels)
    nframes = 5
    X = ((rng.standard_normal((nframes, bins)) + 1j * rng.standard_normal((nframes, bins)))
         * 10.0 ** rng.uniform(-3, 3, (nframes, bins))).astype(np.complex64)
    W, lo, hi = FF.make_bank(bank, n_mels, bins, 1)
    mean, std = FF.make_meanstd(n_mels) if meanstd else (None, None)
    out = Guarded(nframes * n_mels)
    dX, dW, dlo, dhi, dm, ds = (_dev(a) for a in (X.view(np.float32), W, lo, hi, mean, std))
    L.check(L.lib().sed_complex_to_logmel(L.ptr(dX), L.ptr(dW), L.ptr(dlo), L.ptr(dhi), L.ptr(dm), L.ptr(ds), out.ptr, nframes, bins, n_mels,
                                          torch.cuda.current_stream().cuda_stream), "complex_to_logmel")
    got = out.numpy().reshape(nframes, n_mels)
    mr = FF.MelReference(X, None, W, lo, hi, mean, std)
    r = FF.complex_logmel_ratio(got, mr)
    print(f"\ncomplex bins {bins} n_mels {n_mels} {bank}: max err/bound {_note('complex', 'logmel', r.max()):.3f}", end="")
    assert r.max() <= 1.0, (np.unravel_index(r.argmax(), r.shape), r.max())
    if n_mels > 1 and bank != "slaney":          # (a Slaney triangle's edge weights are near zero: nothing to see)
        for mut in ("drop_last_bin", "drop_first_bin", "edge_half") + (("meanstd_roll",) if meanstd else ()):
            assert FF.complex_logmel_ratio(got, FF.MelReference(X, None, W, lo, hi, mean, std, mut)).max() > 1.0, mut


# ---- sed_logmel_crops ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", [1, 17, 64])
@pytest.mark.parametrize("meanstd", [False, True])
def test_logmel_crops(L, n_mels, meanstd):
    rng = np.random.default_rng(n_mels)
    frames, crop = 57, 9
    bank = (rng.standard_normal((frames, n_mels)) * 30 - 30).astype(np.float32)
    starts = np.array([0, frames - crop, 13], np.int32)
    mean, std = FF.make_meanstd(n_mels) if meanstd else (None, None)
    dbank, dst, dm, ds = _dev(bank), _dev(starts), _dev(mean), _dev(std)
    st = torch.cuda.current_stream().cuda_stream
    out = Guarded(3 * crop * n_mels)
    L.check(L.lib().sed_logmel_crops(L.ptr(dbank), frames, starts.ctypes.data_as(ctypes.c_void_p), L.ptr(dst), L.ptr(dm), L.ptr(ds), out.ptr,
                                     3, crop, n_mels, st), "logmel_crops")
    got = out.numpy().reshape(3, crop, n_mels)
    r = FF.crops_ratio(got, bank, starts, crop, mean, std)
    print(f"\ncrops n_mels {n_mels} meanstd {meanstd}: max err/bound {_note('crops', 'z' if meanstd else 'exact', r.max()):.3f}", end="")
    assert r.max() <= (1.0 if meanstd else 0.0)
    if meanstd and n_mels > 1:
        assert FF.crops_ratio(got, bank, starts, crop, np.roll(mean, 1), np.roll(std, 1)).max() > 1.0
    assert FF.crops_ratio(got, bank, (starts + 1) % (frames - crop), crop, mean, std).max() > 1.0
    # a start outside the bank: the error code, and nothing is launched
    for bad in (-1, frames - crop + 1):
        hs = np.array([0, bad, 13], np.int32)
        out2 = Guarded(3 * crop * n_mels)
        assert L.lib().sed_logmel_crops(L.ptr(dbank), frames, hs.ctypes.data_as(ctypes.c_void_p), L.ptr(dst), L.ptr(dm), L.ptr(ds), out2.ptr,
                                        3, crop, n_mels, st) != 0
        assert np.isnan(out2.numpy()).all()


# ---- sensitivity: the gate rejects every mutated reference on the kernel's own output -------------------------------------------------
@pytest.mark.parametrize("name", list(FF.SENSITIVITY))
def test_mutated_references_fail_the_gate(L, knobs, name):
    s = FF.SENSITIVITY[name]
    c = _c(name, s["nfft"], s["hop"], s["samples"], B=s["B"], n_mels=s["n_mels"], bank=s["bank"], meanstd=True, width=s["width"])
    assert route(True, c["nfft"], c["hop"], c["samples"], c["n_mels"], 0, {}) == name
    d = FF.make_inputs(**s)
    knobs({})
    got = run_front(L, c, d, True)
    args = (d["waves"], d["window"], d["nfft"], d["hop"])
    bank = (d["W"], d["lo"], d["hi"], d["mean"], d["std"])
    r0 = FF.logmel_ratio(got, FF.logmel_reference(*args, *bank)).max()
    assert _note(name, "logmel", r0) <= 1.0
    spec = run_front(L, c, d, False) if name in ("generic", "big") else None      # (an nfft-1024 STFT is the generic kernel's)
    for mut in FF.MUTATIONS:
        ref = FF.Reference(*args, mutation=mut)
        r = FF.logmel_ratio(got, ref.mel(*bank)).max()
        print(f"\n{name} {mut}: logmel max err/bound {r:.3g}", end="")
        assert r > 1.0, mut
        if spec is not None and mut in FF.STFT_MUTATIONS:
            r = FF.stft_ratio(spec, ref).max()
            print(f"  stft {r:.3g}", end="")
            assert r > 1.0, mut
