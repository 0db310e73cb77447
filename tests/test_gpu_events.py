"""GPU: the event-decoding kernels of csrc/sed_events.hip through the C ABI -- sed_median_time, sed_decode_events,
sed_segment_counts -- and the layers on top of them (utils.event_utils, infer_file, train.eval_events).

References: scipy.ndimage.median_filter(mode='reflect') for the filter and tests/events_formula.py (plain loops, checked on the host in
tests/test_events_host.py) for the decoder and the segment counts.  No kernel of this library serves as a reference.  Every output is
a selection or an integer, so every comparison is np.array_equal: there is no tolerance anywhere in this module.  Every output buffer
starts filled with a sentinel and lies between two guard regions that must be untouched afterwards.

Sizes: T around the filter's tile (sed_median_time_tile), around the decoder's chunk (sed_decode_events_chunk) and around its 64-frame
ballot word, besides 1, 2, odd lengths and several tiles / chunks."""
import importlib
import pickle

import numpy as np
import pytest
import torch

from events_formula import decode_formula, median_formula, segment_counts_formula

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
GUARD = 1024
FILL = {torch.float32: (float("nan"), -1024.0), torch.int32: (-77, 0x5A5A5A5A), torch.uint8: (0x77, 0xA5),
        torch.int64: (-77, 0x5A5A5A5A5A5A)}


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)._lib


@pytest.fixture(scope="module")
def eu():
    return importlib.import_module(PKG + ".utils.event_utils")


class Guards:
    """output buffers: a sentinel inside, a canary region on both sides, checked by intact()"""

    def __init__(self):
        self.bufs = []

    def new(self, dtype, *shape):
        n = int(np.prod(shape))
        inside, canary = FILL[dtype]
        buf = torch.full((n + 2 * GUARD,), canary, dtype=dtype, device="cuda")
        buf[GUARD:GUARD + n] = inside
        self.bufs.append((buf, n, canary))
        return buf[GUARD:GUARD + n].view(shape)

    def intact(self):
        torch.cuda.synchronize()
        for buf, n, canary in self.bufs:
            assert bool((buf[:GUARD] == canary).all()) and bool((buf[GUARD + n:] == canary).all()), "write outside an output buffer"


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_median(L, x, win):
    """x: numpy (B, T, K) fp32 -> numpy, through the C ABI into a guarded buffer"""
    g = Guards()
    xin = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = g.new(torch.float32, *x.shape)
    L.check(L.lib().sed_median_time(L.ptr(xin), L.ptr(out), x.shape[0], x.shape[1], x.shape[2], win, stream()), "median_time")
    g.intact()
    assert bool((xin.cpu() == torch.from_numpy(x)).all()), "the input was modified"
    return out.cpu().numpy()


def run_decode(L, prob, th_hi, th_lo, max_gap, min_len, max_events=None, with_decisions=True):
    """prob: numpy (B, T, K) fp32 -> (events (max_events, 4), row_counts, total, decisions) as numpy, whole buffers"""
    B, T, K = prob.shape
    cap = B * K * ((T + 1) // 2) if max_events is None else max_events
    g = Guards()
    p = torch.from_numpy(np.ascontiguousarray(prob)).cuda()
    ev = g.new(torch.int32, cap, 4)
    rc = g.new(torch.int32, B * K)
    tot = g.new(torch.int32, 1)
    dec = g.new(torch.uint8, B, T, K) if with_decisions else None
    lib = L.lib()
    nws = lib.sed_decode_events_ws_bytes(B, T, K)
    assert nws == 4 * B * K
    ws = g.new(torch.int32, nws // 4)
    L.check(lib.sed_decode_events(L.ptr(p), B, T, K, th_hi, th_lo, max_gap, min_len, L.ptr(dec), L.ptr(ev), cap, L.ptr(rc),
                                  L.ptr(tot), L.ptr(ws), stream()), "decode_events")
    g.intact()
    return ev.cpu().numpy(), rc.cpu().numpy(), int(tot.item()), (dec.cpu().numpy() if with_decisions else None)


def check_decode(L, prob, th_hi, th_lo, max_gap, min_len, what=""):
    ev, rc, tot, dec = run_decode(L, prob, th_hi, th_lo, max_gap, min_len)
    rev, rrc, rtot, rdec = decode_formula(prob, th_hi, th_lo, max_gap, min_len)
    tag = (what, prob.shape, th_hi, th_lo, max_gap, min_len)
    assert tot == rtot, tag
    assert np.array_equal(rc, rrc), tag
    assert np.array_equal(ev[:tot], rev), tag
    assert bool((ev[tot:] == FILL[torch.int32][0]).all()), ("rows past the total were written", tag)
    assert np.array_equal(dec, rdec), tag
    return ev[:tot], tot


# ---- median filter ---------------------------------------------------------------------------------------------------------------
WINS = [1, 3, 5, 9, 101, 511]


def median_lengths(L):
    tile = L.lib().sed_median_time_tile()
    return sorted({1, 2, 4, 7, 255, 256, 257, 1000, 4099, tile - 1, tile, tile + 1})


def scipy_reflect_breaks(T, win):
    """scipy 1.15.3's median_filter(mode='reflect') leaves the reflection r(i) of the filter's definition (i mod 2T, then i or
    2T - 1 - i) when T is even and the window reaches 4T frames to one side (win >= 8T + 1): among this module's cases T = 2 and
    T = 4 with win = 101 and 511.  tests/test_events_host.py shows formula == scipy up to that edge; at those four (T, win) pairs
    the reference is the formula, tests/events_formula.median_formula, which states the definition directly."""
    return T % 2 == 0 and win >= 8 * T + 1


def median_inputs(T):
    rng = np.random.default_rng(1000 + T)
    gauss = rng.standard_normal((2, T, 3)).astype(np.float32)
    levels = (np.floor(rng.uniform(0, 8, (2, T, 3))) / 8 + 0.0625).astype(np.float32)          # 8 values: heavy ties, no zero
    return {"gaussian": gauss, "8 levels": levels}


@pytest.mark.parametrize("T", [1, 2, 4, 7, 255, 256, 257, 511, 512, 513, 1000, 4099])
def test_median_time_is_scipy_reflect(L, T):
    """B in {1, 2} x K in {1, 3} x every window, Gaussian and 8-level inputs: scipy's bits (the formula's where scipy leaves the
    definition, scipy_reflect_breaks); a second run gives the same bits"""
    from scipy.ndimage import median_filter
    assert T in median_lengths(L), "the lengths of this test must include the kernel's tile - 1, tile, tile + 1"
    for kind, x in median_inputs(T).items():
        for win in WINS:
            ref = median_formula(x, win) if scipy_reflect_breaks(T, win) else median_filter(x, size=(1, win, 1), mode="reflect")
            if T <= 7:
                assert np.array_equal(ref, median_formula(x, win))
            for B in (1, 2):
                for K in (1, 3):
                    xs = np.ascontiguousarray(x[:B, :, :K])
                    got = run_median(L, xs, win)
                    assert np.array_equal(got.view(np.uint32), ref[:B, :, :K].view(np.uint32)), (kind, T, win, B, K)
            again = run_median(L, x, win)
            assert np.array_equal(again.view(np.uint32), got.view(np.uint32)), ("two runs differ", kind, T, win)


def test_median_lengths_cover_the_tile(L):
    assert set(median_lengths(L)) == {1, 2, 4, 7, 255, 256, 257, 511, 512, 513, 1000, 4099}


def test_median_known_answers_and_formula(L):
    x = np.array([0, 1, 2, 3], dtype=np.float32).reshape(1, 4, 1)
    assert run_median(L, x, 9).reshape(-1).tolist() == [2, 2, 1, 1]
    one = np.array([[[0.25]]], dtype=np.float32)
    assert run_median(L, one, 511).tolist() == one.tolist()
    rng = np.random.default_rng(3)
    y = rng.standard_normal((2, 77, 3)).astype(np.float32)
    y[0, 5, 1], y[1, 70, 2] = np.float32(3.0e38), np.float32(-3.0e38)                  # the extremes of the order
    assert np.array_equal(run_median(L, y, 1), y)                                       # win = 1 copies
    for win in (3, 101):
        assert np.array_equal(run_median(L, y, win), median_formula(y, win))


# ---- decoder: one seeded input -------------------------------------------------------------------------------------------------------
def decode_lengths(L):
    chunk = L.lib().sed_decode_events_chunk()
    return sorted({1, 2, 9, 63, 64, 65, 256, 257, 1000, 4099, chunk - 1, chunk, chunk + 1})


def random_walk_probs(T, B=2, K=3, seed=0):
    rng = np.random.default_rng(seed + T)
    walk = np.cumsum(rng.standard_normal((B, T, K)), axis=1) * 0.6
    return (1.0 / (1.0 + np.exp(-walk))).astype(np.float32)


@pytest.mark.parametrize("T", [1, 2, 9, 63, 64, 65, 256, 257, 511, 512, 513, 1000, 4099])
def test_decode_events_seeded(L, T):
    assert T in decode_lengths(L), "the lengths of this test must include the kernel's chunk - 1, chunk, chunk + 1"
    prob = random_walk_probs(T)
    n_events = 0
    for th_hi, th_lo in ((0.5, 0.5), (0.7, 0.3)):
        for max_gap in (0, 1, 5):
            for min_len in (1, 2, 10):
                n_events += check_decode(L, prob, th_hi, th_lo, max_gap, min_len, "seeded")[1]
    assert n_events > 0 or T < 9


def test_decode_lengths_cover_the_chunk(L):
    assert set(decode_lengths(L)) == {1, 2, 9, 63, 64, 65, 256, 257, 511, 512, 513, 1000, 4099}


# ---- decoder: constructed rows -------------------------------------------------------------------------------------------------------
def rows_to_prob(rows):
    """list of equally long (T,) rows -> (1, T, len(rows)) fp32"""
    return np.ascontiguousarray(np.stack([np.asarray(r, dtype=np.float32) for r in rows], axis=1)[None])


def test_decode_constructed_rows(L):
    chunk = L.lib().sed_decode_events_chunk()
    T = 3 * chunk + 37
    lo_v, mid, hi_v = 0.1, 0.5, 0.9                      # with (th_hi, th_lo) = (0.7, 0.3): inactive, above lo only, above hi
    base = np.full(T, lo_v, dtype=np.float32)
    rows = []
    rows.append(np.full(T, hi_v, dtype=np.float32))                                   # all active
    rows.append(base.copy())                                                          # all inactive
    r = base.copy(); r[:5] = hi_v; rows.append(r)                                     # a run from frame 0
    r = base.copy(); r[T - 5:] = hi_v; rows.append(r)                                 # a run to frame T - 1
    r = base.copy()                                                                   # a run across every chunk and word boundary
    for edge in range(64, T, 64):
        r[edge - 2:edge + 2] = hi_v
    rows.append(r)
    r = base.copy(); r[chunk - 20:2 * chunk + 5] = mid; r[2 * chunk + 3] = hi_v; rows.append(r)   # the only hi frame two chunks after the onset
    r = base.copy(); r[chunk - 20:2 * chunk + 5] = mid; rows.append(r)                # the same run without it: no event
    r = base.copy(); r[10:30] = mid; r[29] = hi_v; rows.append(r)                     # kept by a hi frame at its last position
    for gap in (4, 5):                                                                # a gap that straddles a chunk boundary
        r = base.copy(); r[chunk - 12:chunk - 2] = hi_v; r[chunk - 2 + gap:chunk + 20] = hi_v; rows.append(r)
    r = base.copy(); r[100:110] = mid; r[3] = hi_v; r[200:203] = hi_v; rows.append(r)  # a dropped candidate inside a gap
    prob = rows_to_prob(rows)
    for max_gap, min_len in ((0, 1), (4, 1), (5, 1), (4, 11), (200, 1), (0, 4)):
        ev, _ = check_decode(L, prob, 0.7, 0.3, max_gap, min_len, "constructed")
        if (max_gap, min_len) == (4, 1):
            k4 = ev[ev[:, 1] == 8][:, 2:].tolist()
            k5 = ev[ev[:, 1] == 9][:, 2:].tolist()
            assert k4 == [[chunk - 12, chunk + 20]], "a gap of exactly max_gap across the chunk boundary must merge"
            assert k5 == [[chunk - 12, chunk - 2], [chunk + 3, chunk + 20]], "a gap of max_gap + 1 must not"
            assert ev[ev[:, 1] == 5][:, 2:].tolist() == [[chunk - 20, 2 * chunk + 5]]
            assert ev[ev[:, 1] == 6].size == 0
    check_decode(L, prob, 0.5, 0.5, 0, 1, "constructed, one threshold")


def test_decode_probabilities_equal_to_a_threshold(L):
    T = 130
    r1 = np.full(T, 0.7, dtype=np.float32)                         # == th_hi everywhere: above lo, never above hi
    r2 = np.full(T, 0.3, dtype=np.float32)                         # == th_lo: inactive
    r3 = r2.copy(); r3[60:70] = 0.7; r3[64] = 0.9                   # a run bounded by frames that equal th_lo
    r4 = np.full(T, 0.5, dtype=np.float32)
    prob = rows_to_prob([r1, r2, r3, r4])
    ev, tot = check_decode(L, prob, 0.7, 0.3, 0, 1, "p == th")
    assert ev.tolist() == [[0, 2, 60, 70]]
    ev, tot = check_decode(L, prob, 0.5, 0.5, 0, 1, "p == th")
    assert ev[ev[:, 1] == 3].size == 0 and tot == 2                # 0.5 is not > 0.5; rows 0 and 2 are one run each


@pytest.mark.parametrize("T", [1, 2, 7, 64, 65, 1000])
def test_decode_alternating_fills_the_capacity(L, T):
    """alternating 1/0: every row holds ceil(T/2) events, the most a row can: total = B*K*ceil(T/2) = the wrapper's capacity"""
    B, K = 2, 3
    prob = np.zeros((B, T, K), dtype=np.float32)
    prob[:, 0::2, :] = 1.0
    ev, tot = check_decode(L, prob, 0.5, 0.5, 0, 1, "alternating")
    assert tot == B * K * ((T + 1) // 2) == len(ev)
    ev, tot = check_decode(L, prob, 0.5, 0.5, 1, 1, "alternating, merged")
    assert tot == B * K and ev[:, 3].tolist() == [T if T % 2 else T - 1] * (B * K)


def test_decode_capacity_and_order(L):
    prob = random_walk_probs(4099, seed=5)
    rev, rrc, rtot, rdec = decode_formula(prob, 0.5, 0.5, 0, 1)
    assert rtot > 40
    key = (rev[:, 0].astype(np.int64) * 3 + rev[:, 1]) * 10000 + rev[:, 2]
    assert bool((np.diff(key) > 0).all()), "the formula's events are in ascending (b, k, onset) order"
    for max_events in (rtot - 1, rtot // 2, 1, 0):
        ev, rc, tot, dec = run_decode(L, prob, 0.5, 0.5, 0, 1, max_events=max_events)            # guards: nothing past row max_events
        assert tot == rtot and np.array_equal(rc, rrc) and np.array_equal(dec, rdec)
        assert ev.shape == (max_events, 4) and np.array_equal(ev, rev[:max_events])
    ev1, rc1, tot1, _ = run_decode(L, prob, 0.5, 0.5, 0, 1, with_decisions=False)               # decisions may be NULL
    ev2, rc2, tot2, dec2 = run_decode(L, prob, 0.5, 0.5, 0, 1)
    assert tot1 == tot2 == rtot and np.array_equal(ev1, ev2) and np.array_equal(rc1, rc2), "two runs differ"
    assert np.array_equal(ev1[:rtot], rev)


# ---- segment counts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,Tt", [(1000, 995), (257, 300), (9, 7)])
def test_segment_counts(L, T, Tt):
    rng = np.random.default_rng(T)
    B, K = 2, 3
    _, _, _, dec = decode_formula(random_walk_probs(T, seed=9), 0.5, 0.5, 0, 1)
    _, _, _, tgt = decode_formula(random_walk_probs(Tt, seed=10), 0.6, 0.4, 2, 3)
    tgt = tgt.astype(np.float32)
    tgt[rng.uniform(size=tgt.shape) < 0.01] = 0.5                  # 0.5 is not active (strict)
    for seg in (1, 3, 100):
        g = Guards()
        counts = g.new(torch.int64, K, 3)
        d, t = torch.from_numpy(dec).cuda(), torch.from_numpy(tgt).cuda()
        L.check(L.lib().sed_segment_counts(L.ptr(d), L.ptr(t), B, T, Tt, K, seg, L.ptr(counts), stream()), "segment_counts")
        g.intact()
        want = segment_counts_formula(dec, tgt, seg)
        assert np.array_equal(counts.cpu().numpy(), want), (T, Tt, seg)
        assert min(T, Tt) % seg != 0 or seg == 1, "the cases include a last partial segment"
        assert int(want.sum()) > 0


# ---- layers ------------------------------------------------------------------------------------------------------------------------
def test_decode_events_wrapper(eu):
    prob = random_walk_probs(1000, seed=21)
    p = torch.from_numpy(prob).cuda()
    filt = eu.median_filter_time(p, 5)
    assert np.array_equal(filt.cpu().numpy(), median_formula(prob, 5))
    d = eu.decode_events(p, threshold=0.7, low_threshold=0.3, median_window=5, max_gap=2, min_len=3)
    rev, rrc, rtot, rdec = decode_formula(filt.cpu().numpy(), 0.7, 0.3, 2, 3)
    assert np.array_equal(d.numpy(), rev) and int(d.total.item()) == rtot
    assert np.array_equal(d.row_counts.cpu().numpy(), rrc) and np.array_equal(d.decisions.cpu().numpy(), rdec)
    assert d.events.shape == (2 * 3 * 500, 4) and d.events.is_cuda
    sec = d.seconds(10.0, b=1)
    r1 = rev[rev[:, 0] == 1]
    assert np.array_equal(sec, np.stack([r1[:, 1], r1[:, 2] / 10.0, r1[:, 3] / 10.0], axis=1))
    # (T, K) in, (T, K) out; low_threshold=None is plain thresholding
    d2 = eu.decode_events(p[0], threshold=0.5)
    rev2, _, _, rdec2 = decode_formula(prob[:1], 0.5, 0.5, 0, 1)
    assert np.array_equal(d2.numpy(), rev2) and np.array_equal(d2.decisions.cpu().numpy(), rdec2[0])
    assert eu.median_filter_time(p[0], 3).shape == (1000, 3)
    # reference events of a 0/1 matrix, and the segment metrics on top of the counts
    tgt = torch.from_numpy(rdec.astype(np.float64)).cuda()
    assert np.array_equal(eu.events_from_targets(tgt).numpy(), rev)
    m = eu.segment_metrics_device(d2.decisions, tgt[0, :990], 7)
    want = segment_counts_formula(rdec2, rdec[:1, :990].astype(np.float32), 7)
    assert np.array_equal(m["counts"], want)
    tp, fp, fn = (int(v) for v in want.sum(axis=0))
    assert m["micro"]["precision"] == tp / (tp + fp) and m["micro"]["recall"] == tp / (tp + fn)
    assert m["micro"]["error_rate"] == max(fp, fn) / (tp + fn)
    with pytest.raises(ValueError):
        eu.decode_events(p, threshold=0.3, low_threshold=0.7)
    with pytest.raises(ValueError):
        eu.median_filter_time(p, 4)


def small_model(sed, seed=0):
    torch.manual_seed(seed)
    model = sed.Cnn_AvgPooling(1, [(32, 2), (64, 2), (128, 2), (128, 1)])
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for name, b in model.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g) * 0.3)
            elif name.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g) * 1.5 + 0.3)
    return model


def test_infer_file_events(tmp_path):
    from scipy.io import wavfile
    sed = importlib.import_module(PKG)
    infer = importlib.import_module(PKG + ".infer")
    sc = importlib.import_module(PKG + ".dataset.spectogram.spectogram_configs")
    rng = np.random.default_rng(4)
    n = 32000 * 3
    wav = 0.05 * rng.standard_normal(n)
    for s in range(8000, n - 16000, 26000):
        wav[s:s + 8000] += 0.4 * np.sin(2 * np.pi * 700.0 * np.arange(8000) / 32000.0)
    p = str(tmp_path / "clip.wav")
    wavfile.write(p, 32000, (wav.clip(-1, 1) * 32767).astype(np.int16))
    ck = str(tmp_path / "m.pth")
    torch.save({"iterations": 0, "model": small_model(sed).state_dict()}, ck)
    fps = sc.BENCH.frames_per_second
    # z-score the features with the clip's own statistics, so that the untrained model's probabilities move with the signal
    mel = infer.infer_file(p, ck, precision="fp32", cfg=sc.BENCH)["log_mel"]
    ms = str(tmp_path / "mean_std.pkl")
    with open(ms, "wb") as f:
        pickle.dump({"mean": mel.mean(axis=0), "std": mel.std(axis=0) + 1e-3}, f)
    kw = dict(precision="fp32", cfg=sc.BENCH, mean_std=ms)
    plain = infer.infer_file(p, ck, **kw)
    probs = plain["probabilities"]
    th = float(np.median(probs))                                    # a threshold the probabilities actually cross
    plain = infer.infer_file(p, ck, threshold=th, **kw)
    assert np.array_equal(plain["probabilities"], probs)
    # without the new arguments: the decisions and onsets are what they always were
    assert plain["decisions"].dtype == bool and np.array_equal(plain["decisions"], probs > th)
    for k in range(probs.shape[1]):
        d = (probs[:, k] > th).astype(np.int8)
        assert np.array_equal(plain["onset_frames"][k], np.flatnonzero(np.diff(np.concatenate(([0], d))) == 1))
    rev, _, _, _ = decode_formula(probs[None], th, th, 0, 1)
    assert len(rev) > 1 and np.array_equal(plain["event_frames"], rev[:, 1:])
    assert np.array_equal(plain["event_frames"][:, 1], np.concatenate(plain["onset_frames"]))
    # with them: the events are the formula's on the returned probabilities
    lo = float(np.quantile(probs, 0.35))
    full = infer.infer_file(p, ck, threshold=th, median_window=5, low_threshold=lo, max_gap=3, min_len=4, **kw)
    assert np.array_equal(full["probabilities"], probs)
    rev, _, _, rdec = decode_formula(median_formula(probs[None], 5), th, lo, 3, 4)
    assert np.array_equal(full["event_frames"], rev[:, 1:]) and full["event_frames"].dtype == np.int64
    assert np.array_equal(full["events"], np.stack([rev[:, 1], rev[:, 2] / fps, rev[:, 3] / fps], axis=1))
    assert np.array_equal(full["decisions"], rdec[0].astype(bool))
    assert np.array_equal(np.concatenate(full["onset_frames"]), rev[:, 2])
    out = tmp_path / "o"
    base = [p, "--ckpt", ck, "--outputs_dir", str(out), "--precision", "fp32", "--config", "bench", "--mean_std", ms, "--threshold", repr(th)]
    infer.main(base)                                                # no event flag: the file holds what it always held
    z = np.load(out / "clip.npz")
    assert sorted(z.files) == ["decisions", "onset_frames", "onset_seconds", "probabilities"]
    assert np.array_equal(z["decisions"], plain["decisions"]) and np.array_equal(z["onset_frames"], np.concatenate(plain["onset_frames"]))
    infer.main(base + ["--median_window", repr(5.0 / fps), "--low_threshold", repr(lo), "--max_gap", repr(3.0 / fps), "--min_event",
                repr(4.0 / fps)])
    z = np.load(out / "clip.npz")
    assert np.array_equal(z["events"], full["events"]) and np.array_equal(z["event_frames"], full["event_frames"])
    assert np.array_equal(z["decisions"], full["decisions"])


def test_eval_events_matches_the_formula(eu):
    sed = importlib.import_module(PKG)
    train = importlib.import_module(PKG + ".train")
    syn = importlib.import_module(PKG + ".dataset.synthetic")

    class Loader:
        dataset = syn.SyntheticSedDataset(n_train_crops=1, n_val=3, val_frames=808, classes=1, seed=2)

    model = small_model(sed, seed=3).cuda()
    model.set_precision("fp32")
    # the probabilities, once, on the host: what eval_events must decode
    probs, tgts = [], []
    for inp, target, _ in Loader.dataset.get_validation_sampler(None):
        model.eval()
        with torch.no_grad():
            out = model(inp.cuda().float())[0]
        n = min(out.shape[0], target.shape[1])
        probs.append(torch.sigmoid(out[:n]).cpu().numpy()[None])
        tgts.append(target[0, :n].numpy().astype(np.float32)[None])
    th = float(np.median(np.concatenate(probs, axis=1)))            # thresholds the untrained model's probabilities do cross
    lo = float(np.quantile(np.concatenate(probs, axis=1), 0.4))
    opts = dict(threshold=th, low_threshold=lo, median_window=5, max_gap=2, min_len=3, seg_frames=10, collar_frames=4)
    P, R, seg = [], [], np.zeros((1, 3), dtype=np.int64)
    for idx, (prob, tgt) in enumerate(zip(probs, tgts)):
        ev, _, _, dec = decode_formula(median_formula(prob, 5), th, lo, 2, 3)
        rv, _, _, _ = decode_formula(tgt, 0.5, 0.5, 0, 1)
        seg += segment_counts_formula(dec, tgt, 10)
        ev[:, 0], rv[:, 0] = idx, idx
        P.append(ev)
        R.append(rv)
    P, R = np.concatenate(P), np.concatenate(R)
    got = train.eval_events(model, Loader, torch.device("cuda:0"), **opts)
    want_seg = eu.metrics_from_segment_counts(seg)
    want_ev = eu.event_based_metrics(P, R, 4)
    assert got["segment_counts"] == seg.tolist()
    assert got["segment_f1"] == want_seg["micro"]["f1"] and got["segment_error_rate"] == want_seg["micro"]["error_rate"]
    assert got["event_f1"] == want_ev["micro"]["f1"]
    assert got["event_counts"] == [want_ev["micro"]["tp"], want_ev["micro"]["fp"], want_ev["micro"]["fn"]]
    assert got["n_pred_events"] == len(P) and got["n_ref_events"] == len(R) and len(R) > 0 and len(P) > 0
    import json
    json.dumps(got)
    two = train.eval_events(model, Loader, torch.device("cuda:0"), limit_val_samples=2, **opts)
    assert two["n_ref_events"] == int((R[:, 0] < 2).sum())
