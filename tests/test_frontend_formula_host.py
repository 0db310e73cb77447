"""CPU-only checks of tests/frontend_formula.py, the float64 reference and per-element gate of tests/test_gpu_frontend_exact_oracle.py:
the reference agrees with oracle/frontend_oracle.py (precision="f64") to float64 rounding; the gate accepts an independent plain
float32 emulation (radix-2 FFT with a float32 twiddle table, fp32 power and band sums) on every input family of the GPU file; and
every mutated reference -- and the old tolerance's worth of error -- is rejected on the inputs of the sensitivity cases.  A gate that
is too loose, or too tight for a correct fp32 implementation, is found here, before a GPU is involved.

The same for the Complex-mode batch kernel (tests/test_gpu_complex_augment_exact_oracle.py): at every case of that file's list a plain
fp32 numpy emulation passes mix_ratio with the band sums in the kernel's lane order and in plain order, every mutated reference fails
it at the cases it is listed for, and mix_logmel_reference agrees with oracle/dataset_oracle.py's mix_samples / add_noise /
transform_complex run in double precision."""
import numpy as np
import pytest

import frontend_formula as FF
from oracle import dataset_oracle as DO
from oracle import frontend_oracle as FO


def test_reference_agrees_with_the_f64_oracle():
    cfg = FO.FrontEndConfig(32000, 1024, 320, 1024)
    waves = FF.make_waves(2, 4017, 1)
    W, lo, hi = FF.make_bank("slaney", 64, 513)
    assert np.array_equal(W, FO.mel_filter_bank_matrix(cfg).T)
    mean, std = FF.make_meanstd(64)
    win64 = FO.padded_window(cfg)                          # (the oracle's f64 mode keeps the window in double)
    assert np.array_equal(FF.make_window(1024), win64.astype(np.float32))
    ref = FF.Reference(waves, win64, 1024, 320)
    for b in range(2):
        X = FO.stft_channel(waves[b].astype(np.float64), cfg, np.complex128)
        assert np.abs(ref.X[b] - X).max() <= 1e-13 * ref.fnorm[b].max()
    mr = ref.mel(W, lo, hi, mean, std)
    lm = FO.log_mel_from_waveform(waves.T, cfg, mean, std, precision="f64")
    assert lm.shape == mr.z.shape == (2, 1 + 4017 // 320, 64)
    np.testing.assert_allclose(mr.z, lm, rtol=0, atol=1e-11)
    # the short window and another transform size
    cfg2 = FO.FrontEndConfig(44100, 200, 77, 256, mel_bins=20)
    W2, lo2, hi2 = FF.make_bank("slaney", 20, 129, sr=44100)
    mr2 = FF.logmel_reference(waves, FO.padded_window(cfg2), 256, 77, W2, lo2, hi2)
    np.testing.assert_allclose(mr2.z, FO.log_mel_from_waveform(waves.T, cfg2, precision="f64"), rtol=0, atol=1e-11)


def test_bank_kinds_keep_their_promises():
    for kind, n_mels, bins in [("random", 40, 513), ("empty", 64, 513), ("dense", 17, 513), ("sum:1152", 64, 513), ("sum:1153", 64, 513),
                               ("lengths", 130, 16385), ("slaney", 64, 513), ("random", 1, 33), ("random", 33, 8193)]:
        W, lo, hi = FF.make_bank(kind, n_mels, bins)
        k = np.arange(bins)[None, :]
        inside = (k >= lo[:, None]) & (k < hi[:, None])
        assert (W[~inside] == 0).all() and (lo >= 0).all() and (hi <= bins).all() and (hi >= lo).all(), kind
        if kind != "slaney":
            assert (W[inside] >= 0.05).all()
    W, lo, hi = FF.make_bank("random", 40, 513)
    assert lo[0] == 0 and hi[-1] == 513
    W, lo, hi = FF.make_bank("empty", 64, 513)
    assert (hi[16:32] == lo[16:32]).all() and (hi[:3] > lo[:3]).all() and (hi[32:62] > lo[32:62]).all()
    W, lo, hi = FF.make_bank("lengths", 64, 513)
    assert {(int(h - l), int(l % 4)) for l, h in zip(lo, hi)} >= {(n, r) for n in range(6) for r in range(4)}


# the input families of the GPU file at shapes a numpy radix-2 FFT handles in a moment
FAMILIES = {
    "slaney_1024": dict(nfft=1024, hop=320, samples=3204, B=2, n_mels=64, bank="slaney", meanstd=True),
    "random_1024": dict(nfft=1024, hop=128, samples=2432, B=2, n_mels=40, bank="random", width=150),
    "empty_tiles": dict(nfft=1024, hop=252, samples=2048, B=2, n_mels=64, bank="empty", width=40, meanstd=True),
    "dense_bank": dict(nfft=1024, hop=320, samples=1028, B=2, n_mels=17, bank="dense"),
    "silent_loud_quiet": dict(nfft=1024, hop=320, samples=2048, B=3, n_mels=40, bank="random", amps=(0.0, 1.0, 1e-3), meanstd=True),
    "sum_1153": dict(nfft=1024, hop=251, samples=1301, B=2, n_mels=64, bank="sum:1153"),
    "nfft64_hop1": dict(nfft=64, hop=1, samples=90, B=2, n_mels=8, bank="random", meanstd=True),
    "nfft2048_short_window": dict(nfft=2048, hop=700, samples=4100, B=2, n_mels=65, bank="random", win_len=1500),
    "nfft512_minimal_clip": dict(nfft=512, hop=100, samples=257, B=2, n_mels=16, bank="slaney"),
    "nfft4096": dict(nfft=4096, hop=1500, samples=9001, B=2, n_mels=33, bank="random", meanstd=True),
}


@pytest.mark.parametrize("name", list(FAMILIES))
def test_gate_accepts_a_plain_fp32_implementation(name):
    d = FF.make_inputs(**FAMILIES[name])
    ref = FF.Reference(d["waves"], d["window"], d["nfft"], d["hop"])
    rs = FF.stft_ratio(FF.emulate_f32(d["waves"], d["window"], d["nfft"], d["hop"]), ref).max()
    got = FF.emulate_f32(d["waves"], d["window"], d["nfft"], d["hop"], d["W"], d["lo"], d["hi"], d["mean"], d["std"])
    rm = FF.logmel_ratio(got, ref.mel(d["W"], d["lo"], d["hi"], d["mean"], d["std"])).max()
    print(f"\n{name}: fp32 emulation max err/bound  stft {rs:.3f}  logmel {rm:.3f}")
    assert rs <= 1.0 and rm <= 1.0
    assert rs >= 1.0 / 64 or name == "nfft64_hop1"      # the gate is no looser than 64x a plain fp32 FFT's worst element


@pytest.mark.parametrize("route", list(FF.SENSITIVITY))
def test_every_mutation_fails_the_gate(route):
    d = FF.make_inputs(**FF.SENSITIVITY[route])
    args = (d["waves"], d["window"], d["nfft"], d["hop"])
    bank = (d["W"], d["lo"], d["hi"], d["mean"], d["std"])
    spec = FF.emulate_f32(*args)
    got = FF.emulate_f32(*args, *bank)
    assert FF.logmel_ratio(got, FF.logmel_reference(*args, *bank)).max() <= 1.0
    for mut in FF.MUTATIONS:
        ref = FF.Reference(*args, mutation=mut)
        r = FF.logmel_ratio(got, ref.mel(*bank)).max()
        print(f"\n{route} {mut}: logmel max err/bound {r:.3g}", end="")
        assert r > 1.0, mut
        if mut in FF.STFT_MUTATIONS:
            r = FF.stft_ratio(spec, ref).max()
            print(f"  stft {r:.3g}", end="")
            assert r > 1.0, mut


def test_complex_and_crop_gates():
    rng = np.random.default_rng(5)
    bins, n_mels = 513, 64
    X = ((rng.standard_normal((7, bins)) + 1j * rng.standard_normal((7, bins))) * 10.0 ** rng.uniform(-3, 3, (7, bins))).astype(np.complex64)
    W, lo, hi = FF.make_bank("lengths", n_mels, bins)
    mean, std = FF.make_meanstd(n_mels)
    f32 = np.float32
    a = np.sqrt(X.real * X.real + X.imag * X.imag)
    P = a * a
    out = np.empty((7, n_mels), f32)
    for m in range(n_mels):
        acc = np.zeros(7, f32)
        for j in range(lo[m], hi[m]):
            acc = acc + W[m, j] * P[:, j]
        out[:, m] = f32(10) * FF.log10_f32(np.maximum(f32(1e-10), acc))
    assert out.dtype == f32
    z = (out - mean) / std
    assert FF.complex_logmel_ratio(out, FF.MelReference(X, None, W, lo, hi)).max() <= 1.0
    assert FF.complex_logmel_ratio(z, FF.MelReference(X, None, W, lo, hi, mean, std)).max() <= 1.0
    for mut in ("drop_last_bin", "drop_first_bin", "meanstd_roll", "edge_half"):
        assert FF.complex_logmel_ratio(z, FF.MelReference(X, None, W, lo, hi, mean, std, mut)).max() > 1.0, mut
    bank = rng.standard_normal((50, n_mels)).astype(f32) * 30
    starts = [0, 50 - 8, 13]
    crops = np.stack([bank[s:s + 8] for s in starts])
    assert FF.crops_ratio(crops, bank, starts, 8).max() == 0
    assert FF.crops_ratio((crops - mean) / std, bank, starts, 8, mean, std).max() <= 1.0
    assert FF.crops_ratio(np.nextafter(crops, f32(np.inf)), bank, starts, 8).max() == np.inf
    assert FF.crops_ratio((crops - np.roll(mean, 1)) / std, bank, starts, 8, mean, std).max() > 1.0


# ---- sed_complex_augment_logmel --------------------------------------------------------------------------------------------------------
def _emulate(d, order):
    return FF.emulate_mix_f32(d["bank"], d["starts"], d["nmix"], d["nstd"], d["z"], d["cmean"], d["cstd"], d["W"], d["lo"], d["hi"], d["crop"],
                              d["seed"] if d["noise"] == "gen" else None, order)


def test_mix_case_list_covers_what_it_promises():
    C = FF.MIX_CASES
    assert {c["bins"] for c in C} == {33, 257, 513, 16385, 32769} and {c["n_mels"] for c in C} >= {1, 17, 64, 65, 130}
    assert {c["crop"] for c in C} >= {1, 9} and max(len(c["nmix"]) for c in C) <= 5
    assert {c["bank"] for c in C} >= {"slaney", "lengths", "empty", "dense"} and {c["kind"] for c in C} == {"noise", "amps", "zero"}
    assert {(c["noise"], c["zscore"]) for c in C} >= {(n, z) for n in (None, "explicit", "gen") for z in (False, True)} | {("off", False)}
    assert any(set(c["nmix"]) == {1, 2, 3, 4} for c in C)
    assert all(len(c["nmix"]) * c["crop"] <= 2 and c["n_mels"] <= 17 for c in C if c["bins"] > 16384)
    assert any(0.0 in c["nstd"] and max(c["nstd"]) > 0 for c in C if c["nstd"])
    listed = {m for c in C for m in FF.mix_mutations_for(c)}
    assert listed == set(FF.MIX_MUTATIONS)
    for c in C:
        d = FF.make_mix_inputs(c)
        st, nm, last = d["starts"], d["nmix"], c["frames"] - c["crop"]
        assert (st[0, 0] == 0 or (d["B"], nm[0]) == (1, 1)) and st[-1, nm[-1] - 1] == last      # (one clip of one crop: the last start)
        used = [st[b, :nm[b]] for b in range(d["B"])]
        assert all(((u >= 0) & (u <= last)).all() for u in used)
        assert all(set(st[b, nm[b]:]) <= {-1, FF.INT_MAX} for b in range(d["B"]))
        assert all(len(set(u)) < len(u) for u in used if len(u) >= 3)           # a start held twice


@pytest.mark.parametrize("c", FF.MIX_CASES, ids=FF.mix_id)
def test_mix_gate_accepts_fp32_and_rejects_every_mutation(c):
    d = FF.make_mix_inputs(c)
    ref = FF.mix_reference_of(d)
    got = {order: _emulate(d, order) for order in ("lanes", "plain")}
    r = {order: FF.mix_ratio(g, ref).max() for order, g in got.items()}
    print(f"\n{FF.mix_id(c)}: fp32 emulation max err/bound  lanes {r['lanes']:.3f}  plain {r['plain']:.3f}", end="")
    assert r["lanes"] <= 1.0 and r["plain"] <= 1.0
    if c["kind"] == "zero" and not c["zscore"]:
        assert (got["lanes"] == -100.0).all() and (ref.p == 0).all()
    for m in range(c["n_mels"]):                                                # an empty band is exactly -100
        if d["hi"][m] == d["lo"][m]:
            assert (got["lanes"][..., m] == -100.0).all() and (ref.p[..., m] == 0).all()
    for mut in FF.mix_mutations_for(c):
        rm = FF.mix_ratio(got["lanes"], FF.mix_reference_of(d, mut)).max()
        print(f"  {mut} {rm:.3g}", end="")
        assert rm > 1.0, mut


def test_mix_gate_is_not_slack():
    """one ulp-scale error that the flat 2e-3 dB tolerance let through by a factor of hundreds: a loud single-bin band 1e-4 dB off"""
    c = FF.MIX_CASES[1]
    d = FF.make_mix_inputs(c)
    ref = FF.mix_reference_of(d)
    got = _emulate(d, "lanes")
    one = np.flatnonzero(d["hi"] - d["lo"] == 1)[0]
    bad = got.copy()
    bad[0, 0, one] += np.float32(1e-4)
    assert FF.mix_ratio(got, ref).max() <= 1.0 < FF.mix_ratio(bad, ref)[0, 0, one]
    bad = got.copy()
    bad[0, 0, np.flatnonzero(d["hi"] == d["lo"])[0]] = np.float32(-100.00001)   # silence has to be exact
    assert FF.mix_ratio(bad, ref).max() == np.inf


def test_mix_reference_agrees_with_the_dataset_oracle():
    for c in (FF.MIX_CASES[6], FF.MIX_CASES[7], FF.MIX_CASES[3]):               # noise + z-score; noise alone; neither
        d = FF.make_mix_inputs(c)
        ref = FF.mix_reference_of(d)
        bank = d["bank"].astype(np.complex128)[None]
        mel = d["W"].astype(np.float64).T
        for b in range(d["B"]):
            f, _ = DO.mix_samples(bank, np.zeros((c["frames"], 1)), list(d["starts"][b, :d["nmix"][b]]), c["crop"])
            if d["nstd"] is not None and d["nstd"][b] > 0:
                f = DO.add_noise(f, float(d["nstd"][b]), d["z"][b][None].astype(np.float64))
            if c["zscore"]:
                f = (f - d["cmean"].astype(np.complex128)) / d["cstd"].astype(np.float64)
            np.testing.assert_allclose(f[0], ref.V[b], rtol=0, atol=1e-13 * np.abs(ref.V[b]).max())
            p = np.abs(f[0]) ** 2 @ mel
            np.testing.assert_allclose(p, ref.p[b], rtol=1e-13, atol=0)
            if c["zscore"]:                                                     # the oracle's own last step (it returns float32)
                lm = DO.transform_complex(f - 0, 0.0, 1.0, mel)[0]
                np.testing.assert_allclose(lm, ref.v[b], rtol=0, atol=2.0 ** -24 * np.abs(ref.v[b]).max())
    # the generator: the float64 draw rounds to the oracle's fp32 one, and the bound C_GEN holds for a plain fp32 Box-Muller
    ctr = np.arange(100000, dtype=np.uint64)
    z64 = FF.counter_normal64(77, ctr)
    assert np.array_equal(z64.astype(np.float32), DO.counter_normal(77, ctr)) and np.abs(z64).max() <= FF.R_GEN
    h = DO.counter_bits(77, ctr)
    u1 = (((h >> np.uint64(40)) & np.uint64(0xFFFFFF)).astype(np.float32) + np.float32(1)) * np.float32(1 / 16777216)
    u2 = ((h >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float32) * np.float32(1 / 16777216)
    z32 = np.sqrt(np.float32(-2) * np.log(u1)) * np.cos(np.float32(2 * np.pi) * u2)
    assert z32.dtype == np.float32 and 0 < np.abs(z32 - z64).max() <= FF.C_GEN * FF.U
