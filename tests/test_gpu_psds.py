"""GPU: the PSDS counting kernel of csrc/sed_psds.hip through the C ABI -- sed_psds_counts, sed_psds_max_frames -- and the layers on
top of it (utils.psds_utils, train.eval_psds, train(psds_eval=...)).

Reference: tests/psds_formula.py (plain loops over event lists that count frames; checked on the host in tests/test_psds_host.py).
No kernel of this library serves as a reference.  Every output is an integer, so every comparison is np.array_equal: there is no
tolerance anywhere in this module.  The output buffers start filled with a known non-zero base (the call ADDS), lie between two
guard regions that must be untouched afterwards, and the inputs must be unmodified.

Sizes: 1, 2, around the 64-frame ballot word and its multiples, several words plus a tail, and the largest length the call serves
(sed_psds_max_frames); one past it must be refused with nothing written.  Every random case first asserts ON THE FORMULA'S OUTPUT that
one (threshold, class) row has tp > 0, fp > 0, a cross-trigger > 0 (K > 1: with one class there is no other class to trigger) and
tp < n_gt: the seeds below were chosen so, and a comparison of zeros with zeros would prove nothing."""
import functools
import importlib
import json

import numpy as np
import pytest
import torch

from psds_formula import psds_counts

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
GUARD = 1024
CANARY = 0x5A5A5A5A5A5A
BASE = 7                       # what the output buffers hold before a call: the call must ADD to it
PRESETS = {1: dict(dtc=(7, 10), gtc=(7, 10), cttc=(3, 10)), 2: dict(dtc=(1, 10), gtc=(1, 10), cttc=(3, 10))}
TINY_CFG = [(4, 2), (8, 2), (8, 2), (8, 1)]


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)._lib


@pytest.fixture(scope="module")
def pu():
    return importlib.import_module(PKG + ".utils.psds_utils")


class Guards:
    """int64 output buffers: BASE inside, a canary region on both sides, checked by intact()"""

    def __init__(self):
        self.bufs = []

    def new(self, *shape):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.int64, device="cuda")
        buf[GUARD:GUARD + n] = BASE
        self.bufs.append((buf, n))
        return buf[GUARD:GUARD + n].view(shape)

    def intact(self):
        torch.cuda.synchronize()
        for buf, n in self.bufs:
            assert bool((buf[:GUARD] == CANARY).all()) and bool((buf[GUARD + n:] == CANARY).all()), "write outside an output buffer"


def stream():
    return torch.cuda.current_stream().cuda_stream


def c_floats(th):
    import ctypes as C
    th = np.asarray(th, dtype=np.float32).reshape(-1)
    return (C.c_float * len(th))(*th.tolist())


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def run_counts(L, prob, target, th, crit, calls=1, expect_rc0=True):
    """prob (B, T, K), target (B, Tt, K) numpy fp32 -> (counts, gt) numpy int64 MINUS the base, after `calls` identical calls into
    the same guarded buffers"""
    B, T, K = prob.shape
    g = Guards()
    p = torch.from_numpy(np.array(prob)).cuda()                    # a copy: the shared references are read-only
    t = torch.from_numpy(np.array(target)).cuda()
    counts = g.new(len(th), K, K + 3)
    gt = g.new(K, 2)
    cth = c_floats(th)
    for _ in range(calls):
        rc = L.lib().sed_psds_counts(L.ptr(p), L.ptr(t), B, T, target.shape[1], K, cth, len(th), *crit["dtc"], *crit["gtc"],
                                     *crit["cttc"], L.ptr(counts), L.ptr(gt), stream())
        if expect_rc0:
            L.check(rc, "psds_counts")
    g.intact()
    assert same_bits(p.cpu().numpy(), prob) and same_bits(t.cpu().numpy(), target), "an input was modified"
    return counts.cpu().numpy() - BASE, gt.cpu().numpy() - BASE, rc


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def random_runs(rng, n, mean_len, density):
    """a 0/1 row of length n: alternating off / on runs with geometric lengths"""
    row = np.zeros(n, dtype=np.float32)
    pos = 0 if rng.random() < density else int(rng.geometric(1.0 / max(1.0, mean_len * (1 - density) / density)))
    while pos < n:
        on = int(rng.geometric(1.0 / mean_len))
        row[pos:pos + on] = 1.0
        pos += on + int(rng.geometric(1.0 / max(1.0, mean_len * (1 - density) / density)))
    return row


def make_case(seed, B, T, Tt, K):
    """prob (B, T, K): a sigmoid of low-pass-filtered noise plus the class's target and some of the next class's (cross-talk), so
    that detections span many frames, cross word boundaries, and sometimes follow the wrong class; target (B, Tt, K): random runs."""
    rng = np.random.default_rng(seed)
    n = max(T, Tt)
    mean_len = float(min(40, max(1, n // 6)))
    full = np.stack([np.stack([random_runs(rng, n, mean_len, 0.35) for _ in range(K)], axis=1) for _ in range(B)])
    win = min(9, n)
    noise = rng.standard_normal((B, n + win - 1, K))
    csum = np.concatenate([np.zeros((B, 1, K)), np.cumsum(noise, axis=1)], axis=1)
    smooth = (csum[:, win:] - csum[:, :-win]) / np.sqrt(win)                    # (B, n, K), unit variance, low-pass
    logits = 1.3 * smooth + 2.2 * (full - 0.5) + 1.6 * np.roll(full, -1, axis=2) * (K > 1) - 0.4
    prob = (1.0 / (1.0 + np.exp(-logits))).astype(np.float32)
    return np.ascontiguousarray(prob[:, :T]), np.ascontiguousarray(full[:, :Tt])


def thresholds(nth):
    if nth == 1:
        return np.array([0.5], dtype=np.float32)
    return np.linspace(0.01, 0.99, nth).astype(np.float32)


def non_vacuous(counts, gt, K):
    """some (threshold, class) row with tp > 0, fp > 0, tp < n_gt and (K > 1) a cross-trigger"""
    tp, fp, ct = counts[:, :, 0], counts[:, :, 1], counts[:, :, 3:].sum(axis=2)
    ok = (tp > 0) & (fp > 0) & (tp < gt[None, :, 0])
    return bool((ok & (ct > 0)).any()) if K > 1 else bool(ok.any())


@functools.lru_cache(maxsize=None)
def case_and_reference(seed, B, T, Tt, K, nth, scenario):
    """the inputs and the formula's counts of one random case, computed once and shared"""
    prob, target = make_case(seed, B, T, Tt, K)
    th = thresholds(nth)
    crit = PRESETS[scenario]
    counts, gt = psds_counts(prob, target, th, crit["dtc"], crit["gtc"], crit["cttc"])
    for a in (prob, target, th, counts, gt):
        a.setflags(write=False)
    return prob, target, th, counts, gt


# (T, Tt, K, nth, B, seed): T over 1, 2, around one and two words, several words with a tail; Tt below, at and above T; K 1, 3, 14;
# nth 1, 50, 64; B 1, 3.  The seeds make both presets non-vacuous (checked below on the formula's output).
CASES = [(1, 1, 3, 50, 3, 2), (2, 3, 3, 64, 3, 0), (63, 63, 1, 1, 1, 9), (64, 60, 3, 50, 1, 0), (65, 65, 14, 1, 3, 0),
         (127, 130, 3, 64, 1, 0), (128, 128, 14, 50, 1, 0), (129, 100, 1, 50, 3, 0), (200, 200, 3, 1, 3, 2),
         (1000, 1000, 14, 50, 1, 0)]


@pytest.mark.parametrize("scenario", [1, 2])
@pytest.mark.parametrize("T,Tt,K,nth,B,seed", CASES)
def test_counts_match_the_formula(L, T, Tt, K, nth, B, seed, scenario):
    prob, target, th, want, want_gt = case_and_reference(seed, B, T, Tt, K, nth, scenario)
    assert non_vacuous(want, want_gt, K), "the case is vacuous: choose another seed"
    assert (want[:, np.arange(K), 3 + np.arange(K)] == 0).all()
    got, got_gt, _ = run_counts(L, prob, target, th, PRESETS[scenario])
    assert np.array_equal(got_gt, want_gt)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("scenario", [1, 2])
def test_longest_recording_and_one_past_it(L, scenario):
    K, nth = 14, 1
    T = L.lib().sed_psds_max_frames(K, nth)
    assert T >= 8192 and T % 64 == 0
    prob, target, th, want, want_gt = case_and_reference(0, 1, T, T, K, nth, scenario)
    assert non_vacuous(want, want_gt, K)
    got, got_gt, _ = run_counts(L, prob, target, th, PRESETS[scenario])
    assert np.array_equal(got_gt, want_gt) and np.array_equal(got, want)
    if scenario == 1:
        longer = np.zeros((1, T + 1, K), dtype=np.float32)
        got, got_gt, rc = run_counts(L, longer + 0.9, longer + 1.0, th, PRESETS[1], expect_rc0=False)
        assert rc != 0 and b"sed_psds_max_frames" in L.lib().sed_last_error()
        assert not got.any() and not got_gt.any(), "a refused call wrote"
        # a longer TARGET is fine: only min(T, Tt) frames are scored
        got, got_gt, _ = run_counts(L, prob, np.concatenate([target, target[:, :5]], axis=1), th, PRESETS[1])
        assert np.array_equal(got_gt, want_gt) and np.array_equal(got, want)


# ---- hand-made rows --------------------------------------------------------------------------------------------------------------
def check(L, prob, target, th, scenario=1):
    crit = PRESETS[scenario]
    want, want_gt = psds_counts(prob, target, th, crit["dtc"], crit["gtc"], crit["cttc"])
    got, got_gt, _ = run_counts(L, prob, target, np.asarray(th, dtype=np.float32), crit)
    assert np.array_equal(got_gt, want_gt) and np.array_equal(got, want), (prob.shape, th, scenario)
    return want, want_gt


@pytest.mark.parametrize("n", [64, 100, 128, 191])
def test_all_none_nan_and_extreme_thresholds(L, n):
    K = 3
    prob = np.empty((2, n, K), dtype=np.float32)
    prob[:, :, 0] = 0.9                         # above every threshold: one run that covers the whole recording
    prob[:, :, 1] = 0.1                         # below every threshold
    prob[:, :, 2] = 0.9
    prob[0, n // 2, 2] = np.nan                 # a NaN frame splits the run
    prob[1, n - 1, 2] = np.nan
    target = np.zeros((2, n, K), dtype=np.float32)
    target[0, :, 0] = 1.0                       # ground truth over the whole recording
    target[1, 10:n - 1, 0] = 1.0
    target[:, 5:n // 2 + 9, 2] = 1.0
    target[1, n // 3:, 1] = 1.0
    for scenario in (1, 2):
        want, want_gt = check(L, prob, target, [0.2, 0.5, 0.8], scenario)
        assert want[:, 0, 2].tolist() == [2, 2, 2] and want[:, 1, :].sum() == 0 and want[:, 2, 2].tolist() == [3, 3, 3]
        assert want_gt[0].tolist() == [2, n + n - 11]
    # a threshold of 0 detects every frame with p > 0 (not p == 0, not -0); thresholds >= 1 detect nothing, 1.0 itself included
    prob[:, :, 0] = 1.0
    prob[0, 3:7, 0] = 0.0
    prob[0, 20, 0] = -0.0
    prob[:, :, 1] = 0.0
    want, _ = check(L, prob, target, [0.0, 1.0, 1.5, 0.5, np.nextafter(np.float32(1.0), np.float32(0.0))])
    assert want[:, 0, 2].tolist() == [4, 0, 0, 4, 4] and want[:, 1, 2].sum() == 0


def test_runs_at_word_boundaries_and_the_last_frame(L):
    n, K = 150, 3

    def rows(spans):
        x = np.zeros((len(spans), n, K), dtype=np.float32)
        for b, per_class in enumerate(spans):
            for k, runs_ in enumerate(per_class):
                for a, e in runs_:
                    x[b, a:e, k] = 1.0
        return x

    det = rows([[[(60, 64), (64 + 1, 70), (128, 150)], [(0, 64), (65, 128)], [(63, 65), (127, 129), (149, 150)]],
                [[(0, 63), (64, 128), (129, 149)], [(63, 64), (64 + 63, 64 + 64)], [(0, 150)]],
                [[(64, 150)], [(0, 128)], [(1, 149)]]])
    tgt = rows([[[(60, 64), (66, 70), (120, 150)], [(0, 63), (64, 127)], [(64, 65), (128, 129), (148, 150)]],
                [[(0, 64), (64, 127), (128, 150)], [(62, 66)], [(63, 64), (149, 150)]],
                [[(0, 64)], [(64, 150)], [(0, 1), (149, 150)]]])
    prob = 0.1 + 0.8 * det
    for scenario in (1, 2):
        want, want_gt = check(L, prob, tgt, [0.5, 0.05, 0.95], scenario)
        assert want[0, :, 2].tolist() == [7, 5, 5] and want[1, :, 2].tolist() == [3, 3, 3] and not want[2].any()
        assert want_gt[:, 0].tolist() == [6, 4, 7]          # [0, 64) and [64, 127) are one event
    for cut in (149, 129, 128, 65, 64, 63):          # the same rows cut at a tail word, at a word's end and just past it
        check(L, prob[:, :cut], tgt, [0.5])
        check(L, prob, tgt[:, :cut], [0.5], 2)


def test_criteria_at_equality(L):
    n, K = 140, 3
    prob = np.full((1, n, K), 0.1, dtype=np.float32)
    target = np.zeros((1, n, K), dtype=np.float32)
    prob[0, 60:70, 0] = 0.9                     # DTC: 7 of 10 frames -> relevant (equality); it covers 7 of ground truth [57, 67),
    target[0, 57:67, 0] = 1.0                   # GTC: 7 * 10 >= 7 * 10 -> a true positive (equality)
    prob[0, 120:130, 0] = 0.9                   # DTC: 6 of 10 -> a false positive;
    target[0, 124:130, 0] = 1.0
    target[0, 120:123, 1] = 1.0                 # CTTC: 3 of 10 -> a cross-trigger (equality)
    target[0, 128:130, 2] = 1.0                 # CTTC: 2 of 10 -> none
    want, want_gt = check(L, prob, target, [0.5])
    assert want[0, 0].tolist() == [1, 1, 2, 0, 1, 0] and want_gt.tolist() == [[2, 16], [1, 3], [1, 2]]
    prob[0, 69, 0] = 0.1                        # [60, 69): 7 of 9 frames passes DTC and still covers 7 of the 10: unchanged
    want, _ = check(L, prob, target, [0.5])
    assert want[0, 0].tolist() == [1, 1, 2, 0, 1, 0]
    prob[0, 60, 0] = 0.1                        # [61, 69): 6 of 8 passes DTC but covers 6 of 10: 60 < 70 fails GTC
    want, _ = check(L, prob, target, [0.5])
    assert want[0, 0].tolist() == [0, 1, 2, 0, 1, 0]


# ---- accumulation ------------------------------------------------------------------------------------------------------------------
def test_two_calls_add_and_gt_grows_once_per_call(L):
    prob, target, th, want, want_gt = case_and_reference(2, 3, 200, 200, 3, 1, 1)
    prob50, target50, th50, want50, want_gt50 = case_and_reference(0, 1, 128, 128, 14, 50, 2)
    assert want_gt.sum() > 0 and np.array_equal(want_gt, want_gt50) is False
    got, got_gt, _ = run_counts(L, prob, target, th, PRESETS[1], calls=2)
    assert np.array_equal(got, 2 * want) and np.array_equal(got_gt, 2 * want_gt)
    got, got_gt, _ = run_counts(L, prob50, target50, th50, PRESETS[2], calls=3)
    assert np.array_equal(got, 3 * want50) and np.array_equal(got_gt, 3 * want_gt50)       # 3 x, not 3 x 50 x


def test_two_different_calls_sum(L):
    a = case_and_reference(0, 1, 127, 130, 3, 64, 1)
    b = case_and_reference(0, 1, 64, 60, 3, 50, 1)
    th = a[2]
    wb, wb_gt = psds_counts(b[0], b[1], th, *PRESETS[1].values())
    g = Guards()
    counts, gt = g.new(64, 3, 6), g.new(3, 2)
    for prob, target in ((a[0], a[1]), (b[0], b[1])):
        p, t = torch.from_numpy(np.array(prob)).cuda(), torch.from_numpy(np.array(target)).cuda()
        L.check(L.lib().sed_psds_counts(L.ptr(p), L.ptr(t), 1, prob.shape[1], target.shape[1], 3, c_floats(th), 64, 7, 10, 7, 10, 3,
                                        10, L.ptr(counts), L.ptr(gt), stream()), "psds_counts")
    g.intact()
    assert np.array_equal(counts.cpu().numpy() - BASE, a[3] + wb) and np.array_equal(gt.cpu().numpy() - BASE, a[4] + wb_gt)


def test_shuffled_thresholds_give_the_rows_in_that_order(L):
    prob, target, th, want, want_gt = case_and_reference(0, 1, 127, 130, 3, 64, 2)
    order = np.random.default_rng(5).permutation(len(th))
    assert not np.array_equal(want[order], want)
    got, got_gt, _ = run_counts(L, prob, target, th[order], PRESETS[2])
    assert np.array_equal(got, want[order]) and np.array_equal(got_gt, want_gt)


def test_same_bits_on_every_run(L):
    prob, target, th, want, _ = case_and_reference(0, 1, 1000, 1000, 14, 50, 2)
    for _ in range(3):
        assert np.array_equal(run_counts(L, prob, target, th, PRESETS[2])[0], want)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_accumulator_over_batches_of_different_lengths(L, pu):
    batches = [case_and_reference(2, 3, 200, 200, 3, 1, 1)[:2], make_case(31, 2, 127, 130, 3), make_case(32, 1, 64, 60, 3)]
    acc = pu.PsdsAccumulator(3, "cuda", scenario=2)
    th = acc.thresholds
    assert len(th) == 50 and th.dtype == np.float32
    want, want_gt, frames = 0, 0, 0
    for prob, target in batches:
        acc.update(torch.from_numpy(np.array(prob)).cuda(), torch.from_numpy(np.array(target)).cuda())
        c, g = psds_counts(prob, target, th, (1, 10), (1, 10), (3, 10))
        want, want_gt, frames = want + c, want_gt + g, frames + prob.shape[0] * min(prob.shape[1], target.shape[1])
    acc.update(torch.from_numpy(batches[2][0][0]).cuda(), torch.from_numpy(batches[2][1][0]).cuda())        # (T, K): one recording
    c, g = psds_counts(batches[2][0], batches[2][1], th, (1, 10), (1, 10), (3, 10))
    want, want_gt, frames = want + c, want_gt + g, frames + 60
    counts, gt = acc.compute_raw()
    assert counts.dtype == np.int64 and np.array_equal(counts, want) and np.array_equal(gt, want_gt) and acc.total_frames == frames
    fps = 0.05              # these few hundred frames then last hours: some operating points lie below e_max = 100 per hour
    res = acc.compute(fps)
    ref = pu.psds_from_counts(want, want_gt, frames, fps, 0.5, 1.0, 100.0)
    for key in ref:
        assert json.dumps(res[key]) == json.dumps(ref[key]), key                   # bit for bit: the same floats print the same
    assert res["classes_scored"] == 3 and 0.0 < res["psds"] < 1.0 and res["best_macro_f1_threshold"] == float(th[res["best_macro_f1_index"]])
    acc.reset()
    assert acc.total_frames == 0 and not acc.compute_raw()[0].any() and not acc.compute_raw()[1].any()
    with pytest.raises(ValueError):
        acc.update(torch.zeros(2, 10, 4, device="cuda"), torch.zeros(2, 10, 4, device="cuda"))
    with pytest.raises(ValueError):
        acc.update(torch.zeros(2, 10, 3, device="cuda"), torch.zeros(1, 10, 3, device="cuda"))
    with pytest.raises(RuntimeError, match="CUDA|no CPU path"):
        acc.update(torch.zeros(2, 10, 3), torch.zeros(2, 10, 3))


def test_median_window_and_the_one_shot_form(L, pu):
    from scipy.ndimage import median_filter
    prob, target = make_case(33, 2, 129, 129, 3)
    th = np.array([0.3, 0.5, 0.7], dtype=np.float32)
    filtered = median_filter(prob, size=(1, 5, 1), mode="reflect")
    assert not np.array_equal(filtered, prob)
    want, want_gt = psds_counts(filtered, target, th, (7, 10), (7, 10), (3, 10))
    plain, _ = psds_counts(prob, target, th, (7, 10), (7, 10), (3, 10))
    assert not np.array_equal(want, plain)
    acc = pu.PsdsAccumulator(3, "cuda", thresholds=th, scenario=1, median_window=5)
    acc.update(torch.from_numpy(prob).cuda(), torch.from_numpy(target).cuda())
    counts, gt = acc.compute_raw()
    assert np.array_equal(counts, want) and np.array_equal(gt, want_gt)
    res = pu.psds_device(torch.from_numpy(prob).cuda(), torch.from_numpy(target).cuda(), 50.0, thresholds=th, scenario=1,
                         median_window=5)
    ref = pu.psds_from_counts(want, want_gt, 2 * 129, 50.0, 0.0, 1.0, 100.0)
    assert json.dumps(res["psds"]) == json.dumps(ref["psds"]) and json.dumps(res["per_class"]) == json.dumps(ref["per_class"])
    custom = pu.psds_device(torch.from_numpy(prob).cuda(), torch.from_numpy(target).cuda(), 50.0, thresholds=th,
                            scenario=dict(dtc=0.5, gtc=0.5, cttc=0.3, alpha_ct=1.0, alpha_st=0.0, e_max=50))
    c, g = psds_counts(prob, target, th, (1, 2), (1, 2), (3, 10))
    assert json.dumps(custom["psds"]) == json.dumps(pu.psds_from_counts(c, g, 2 * 129, 50.0, 1.0, 0.0, 50.0)["psds"])


# ---- training ----------------------------------------------------------------------------------------------------------------------
def tiny_model_and_loader(seed=2):
    sed = importlib.import_module(PKG)
    syn = importlib.import_module(PKG + ".dataset.synthetic")

    from torch.utils.data import DataLoader
    loader = DataLoader(syn.SyntheticSedDataset(n_train_crops=8, crop=32, n_val=3, val_frames=200, classes=3, seed=seed), batch_size=4)
    torch.manual_seed(seed)
    model = sed.Cnn_AvgPooling(3, TINY_CFG, precision="fp32").cuda()
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for name, b in model.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g) * 0.3)
            elif name.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g) * 1.5 + 0.3)
    return sed, model, loader


def test_eval_psds_matches_the_formula(pu):
    sed, model, loader = tiny_model_and_loader()
    mu = importlib.import_module(PKG + ".utils.metric_utils")
    dev = torch.device("cuda:0")
    th = pu.check_thresholds(None)
    want, want_gt, frames = 0, 0, 0
    for inp, target, _ in loader.dataset.get_validation_sampler(None):
        model.eval()
        with torch.no_grad():
            out = model(inp.cuda().float())[0]
        tg = target[0].cuda().float()
        p = mu.metric_counts_device(out, tg, raw_logits=True, return_probs=True)[3]
        c, g = psds_counts(p.cpu().numpy()[None], tg.cpu().numpy()[None], th, (1, 10), (1, 10), (3, 10))
        want, want_gt, frames = want + c, want_gt + g, frames + min(p.shape[0], tg.shape[0])
    got = sed.train.eval_psds(model, loader, dev, scenario=2, fps=50.0)
    assert set(got) >= {"psds", "classes_scored", "best_macro_f1", "best_macro_f1_threshold"} and got["n_recordings"] == 3
    ref = pu.psds_from_counts(want, want_gt, frames, 50.0, 0.5, 1.0, 100.0)
    assert want_gt[:, 0].sum() > 0 and want[:, :, 2].sum() > 0
    assert json.dumps([got["psds"], got["classes_scored"], got["best_macro_f1"]]) == \
        json.dumps([ref["psds"], ref["classes_scored"], ref["best_macro_f1"]])
    assert got["best_macro_f1_threshold"] == float(th[ref["best_macro_f1_index"]])
    json.dumps(got)
    two = sed.train.eval_psds(model, loader, dev, fps=50.0, limit_val_samples=2, thresholds=[0.5], median_window=3)
    assert two["n_recordings"] == 2 and two["best_macro_f1_threshold"] == 0.5
    with pytest.raises(ValueError):
        sed.train.eval_psds(model, loader, dev, fps=50.0, scenario=3)


def test_train_logs_the_psds_record(tmp_path):
    sed, model, loader = tiny_model_and_loader(seed=4)
    crit = sed.WeightedBCE(5, True)
    sed.train.train(model, loader, crit, 2, 1e-3, 2, str(tmp_path), "cuda", psds_eval={"fps": 50.0, "scenario": 2})
    rec = json.loads(open(tmp_path / "progress.jsonl").read().strip().splitlines()[-1])
    assert "ranking" not in rec and {"psds", "classes_scored", "best_macro_f1", "best_macro_f1_threshold"} <= set(rec["psds"])
    assert rec["psds"]["n_recordings"] == 3 and rec["psds"]["scenario"] == 2
