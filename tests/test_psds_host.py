"""CPU-only checks of the PSDS layer: the plain-loop formula (tests/psds_formula.py) on hand-worked cases whose counts are written out
here, psds_from_counts against exact Fraction integration of the same step functions, the criterion-fraction helper, option
validation, and the CLI / train() refusals.  No kernel is launched."""
import importlib
import inspect
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from psds_formula import curve_value, psds_counts, psds_exact, runs

PKG = "soundeventdetection-pytorch_amd"
LIB = os.path.join(ROOT, PKG, "libsed_hip.so")
S1 = dict(dtc=(7, 10), gtc=(7, 10), cttc=(3, 10))
# psds_from_counts is a few dozen float64 operations on values in [0, 1] and widths in [0, e_max] divided by e_max: every result
# is within a few units of 2^-53 of the exact one; 2^-40 leaves room for the length of the sums and is far below any real difference
TOL = 2.0 ** -40


@pytest.fixture(scope="module")
def sed():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def pu():
    return importlib.import_module(PKG + ".utils.psds_utils")


def rows(n, K, det=(), tgt=()):
    """prob / target (1, n, K) with prob 0.9 inside the (k, onset, offset) runs of `det` (0.1 elsewhere) and target 1 inside `tgt`"""
    p = np.full((1, n, K), 0.1, dtype=np.float32)
    t = np.zeros((1, n, K), dtype=np.float32)
    for k, a, e in det:
        p[0, a:e, k] = 0.9
    for k, a, e in tgt:
        t[0, a:e, k] = 1.0
    return p, t


def one(p, t, crit=S1):
    c, g = psds_counts(p, t, [0.5], crit["dtc"], crit["gtc"], crit["cttc"])
    return c[0].tolist(), g.tolist()


# ---- the formula on hand-worked cases ---------------------------------------------------------------------------------------------
def test_runs():
    assert runs(np.array([], dtype=bool)) == []
    assert runs(np.array([1, 1, 0, 1, 0, 0, 1], dtype=bool)) == [(0, 2), (3, 4), (6, 7)]
    assert runs(np.ones(5, dtype=bool)) == [(0, 5)]


def test_dtc_boundary_and_an_irrelevant_detection_does_not_help_gtc():
    # detection [0, 10) holds 7 target frames: 7 * 10 >= 7 * 10, relevant; detection [20, 30) holds 6: 60 < 70, a false positive.
    # ground truth [0, 7) is covered over all 7 frames by the relevant detection: TP; ground truth [20, 26) is covered only by the
    # false positive, which does not count: J = 0, not a TP.
    p, t = rows(40, 1, det=[(0, 0, 10), (0, 20, 30)], tgt=[(0, 0, 7), (0, 20, 26)])
    counts, gt = one(p, t)
    assert counts == [[1, 1, 2, 0]] and gt == [[2, 13]]
    # with DTC = GTC = 1/10 (scenario 2) the second detection is relevant too and both events are found
    counts, _ = one(p, t, dict(dtc=(1, 10), gtc=(1, 10), cttc=(3, 10)))
    assert counts == [[2, 0, 2, 0]]


def test_ground_truth_covered_by_two_relevant_detections():
    # ground truth [0, 20); detections [0, 8) and [10, 16) lie inside it (relevant): J = 8 + 6 = 14, 14 * 10 >= 7 * 20: TP at equality
    p, t = rows(30, 1, det=[(0, 0, 8), (0, 10, 16)], tgt=[(0, 0, 20)])
    assert one(p, t) == ([[1, 0, 2, 0]], [[1, 20]])
    # one frame less: J = 13, 130 < 140: neither detection alone nor both together reach the criterion
    p, t = rows(30, 1, det=[(0, 0, 8), (0, 10, 15)], tgt=[(0, 0, 20)])
    assert one(p, t) == ([[0, 0, 2, 0]], [[1, 20]])


def test_false_positive_cross_triggers_two_classes_and_counts_once():
    # class 0 is detected over [0, 10) with no class-0 target: one false positive.  Class 1 is on for 3 of its frames (3 * 10 >= 3 * 10,
    # equality) and class 2 for 8: two cross-triggers, ct[0] stays 0.
    p, t = rows(20, 3, det=[(0, 0, 10)], tgt=[(1, 0, 3), (2, 2, 10)])
    counts, gt = one(p, t)
    assert counts == [[0, 1, 1, 0, 1, 1], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]]
    assert gt == [[0, 0], [1, 3], [1, 8]]
    # 2 of 10 frames is below CTTC: class 1 is no longer cross-triggered
    p, t = rows(20, 3, det=[(0, 0, 10)], tgt=[(1, 0, 2), (2, 2, 10)])
    assert one(p, t)[0][0] == [0, 1, 1, 0, 0, 1]
    # a RELEVANT detection never cross-triggers, whatever the other classes do
    p, t = rows(20, 3, det=[(0, 0, 10)], tgt=[(0, 0, 10), (1, 0, 10), (2, 0, 10)])
    assert one(p, t)[0][0] == [1, 0, 1, 0, 0, 0]


def test_truncation_nan_and_threshold_order():
    p, t = rows(12, 1, det=[(0, 2, 12)], tgt=[(0, 2, 8)])
    t = t[:, :8]                                                  # n = 8: detection [2, 8), ground truth [2, 8)
    assert one(p, t) == ([[1, 0, 1, 0]], [[1, 6]])
    p[0, 4, 0] = np.nan                                           # a NaN never detects: two detections [2, 4) and [5, 8)
    assert one(p, t) == ([[1, 0, 2, 0]], [[1, 6]])
    c, g = psds_counts(p, t, [0.95, 0.5, 0.0], *S1.values())
    assert c[:, 0, 2].tolist() == [0, 2, 2] and g.tolist() == [[1, 6]]      # rows follow the thresholds' order; gt counted once


# ---- psds_from_counts against exact fractions ---------------------------------------------------------------------------------------
FPS = 10.0
HOUR = 36000                  # frames: hours = 1, so fp is the fpr


def make_counts(points, n_gt, ct=None):
    """points[k] = [(fp, tp)] per threshold -> counts (nth, K, K + 3), gt (K, 2) with gt frames = HOUR / 2 per scored class"""
    K, nth = len(points), len(points[0])
    counts = np.zeros((nth, K, K + 3), dtype=np.int64)
    for k in range(K):
        for i, (fp, tp) in enumerate(points[k]):
            counts[i, k, 0], counts[i, k, 1], counts[i, k, 2] = tp, fp, tp + fp
    if ct is not None:
        counts[:, :, 3:] = ct
    gt = np.array([[n, HOUR // 2 if n else 0] for n in n_gt], dtype=np.int64)
    return counts, gt


def exact(points, n_gt, alpha_st, e_max):
    scored = [k for k in range(len(points)) if n_gt[k] > 0]
    return psds_exact([[(Fraction(fp), Fraction(tp, n_gt[k])) for fp, tp in points[k]] for k in scored], alpha_st, e_max)


def test_perfect_detector_scores_one_and_no_detections_zero(pu):
    counts, gt = make_counts([[(0, 4), (0, 4), (0, 3)], [(0, 5), (0, 2), (0, 0)]], [4, 5])
    res = pu.psds_from_counts(counts, gt, HOUR, FPS, 0.0, 1.0, 100)
    assert res["psds"] == 1.0 and res["classes_scored"] == 2 and res["reason"] is None
    assert [c["area"] for c in res["per_class"]] == [1.0, 1.0]
    assert res["macro_f1"][0] == 1.0 and res["best_macro_f1"] == 1.0 and res["best_macro_f1_index"] == 0
    counts, gt = make_counts([[(0, 0)] * 3, [(0, 0)] * 3], [4, 5])
    res = pu.psds_from_counts(counts, gt, HOUR, FPS, 0.0, 1.0, 100)
    assert res["psds"] == 0.0 and res["macro_f1"] == [0.0, 0.0, 0.0]


def test_alpha_st_pulls_the_score_down_when_classes_differ(pu):
    # class 0 finds everything at once; class 1 finds half at efpr 0 and all at efpr 50: mean 3/4, std 1/4 on [0, 50)
    points, n_gt = [[(0, 4), (0, 4)], [(0, 2), (50, 4)]], [4, 4]
    counts, gt = make_counts(points, n_gt)
    want1, areas = exact(points, n_gt, 1, 100)
    want0, _ = exact(points, n_gt, 0, 100)
    assert want1 == Fraction(3, 4) and want0 == Fraction(7, 8) and areas == [1, Fraction(3, 4)]
    r1 = pu.psds_from_counts(counts, gt, HOUR, FPS, 0.0, 1.0, 100)
    r0 = pu.psds_from_counts(counts, gt, HOUR, FPS, 0.0, 0.0, 100)
    assert abs(r1["psds"] - float(want1)) <= TOL and abs(r0["psds"] - float(want0)) <= TOL and r1["psds"] < r0["psds"]
    assert all(abs(c["area"] - float(a)) <= TOL for c, a in zip(r1["per_class"], areas))
    assert r1["axis"] == [0.0, 50.0, 100.0] and r1["eff"] == [0.5, 1.0]


def test_class_without_ground_truth_is_excluded(pu):
    points, n_gt = [[(0, 4), (0, 4)], [(0, 2), (50, 4)], [(900, 0), (70, 0)]], [4, 4, 0]
    counts, gt = make_counts(points, n_gt)
    res = pu.psds_from_counts(counts, gt, HOUR, FPS, 0.0, 1.0, 100)
    assert res["classes_scored"] == 2 and abs(res["psds"] - 0.75) <= TOL
    assert res["per_class"][2]["scored"] is False and math.isnan(res["per_class"][2]["area"])
    assert res["axis"] == [0.0, 50.0, 100.0]                       # the unscored class adds no point to the axis
    none = pu.psds_from_counts(*make_counts([[(3, 0)], [(1, 0)]], [0, 0]), HOUR, FPS, 0.0, 1.0, 100)
    assert math.isnan(none["psds"]) and none["classes_scored"] == 0 and "ground-truth" in none["reason"]


def test_points_beyond_e_max_are_ignored(pu):
    # 2/5 found at efpr 10, everything only at efpr 150 > e_max: area = 0.4 * 90 / 100
    points, n_gt = [[(10, 2), (150, 5)]], [5]
    counts, gt = make_counts(points, n_gt)
    want, _ = exact(points, n_gt, 1, 100)
    assert want == Fraction(9, 25)
    res = pu.psds_from_counts(counts, gt, HOUR, FPS, 0.0, 1.0, 100)
    assert abs(res["psds"] - 0.36) <= TOL and res["axis"] == [10.0, 100.0]
    # the running maximum: a later threshold with MORE false positives and FEWER hits does not lower the curve
    points = [[(10, 3), (20, 1), (30, 5)]]
    counts, gt = make_counts(points, n_gt)
    res = pu.psds_from_counts(counts, gt, HOUR, FPS, 0.0, 1.0, 100)
    assert res["per_class"][0]["tpr"] == [0.6, 0.6, 1.0] and abs(res["psds"] - float(exact(points, n_gt, 1, 100)[0])) <= TOL
    assert curve_value([(10, Fraction(3, 5)), (20, Fraction(1, 5))], 25) == Fraction(3, 5)


def test_cross_trigger_cost(pu):
    # class 0 at one threshold: 4 false positives and 5 cross-triggers against class 1, whose ground truth lasts half an hour:
    # efpr = 4 + 0.5 * (5 / 0.5) = 9; class 1 has no false positive and no cross-trigger: efpr 0
    counts, gt = make_counts([[(4, 2)], [(0, 3)]], [2, 3])
    counts[0, 0, 3 + 1] = 5
    res = pu.psds_from_counts(counts, gt, HOUR, FPS, 0.5, 1.0, 100)
    assert res["per_class"][0]["efpr"] == [9.0] and res["per_class"][1]["efpr"] == [0.0]
    res0 = pu.psds_from_counts(counts, gt, HOUR, FPS, 0.0, 1.0, 100)
    assert res0["per_class"][0]["efpr"] == [4.0]
    one_class = pu.psds_from_counts(counts[:, :1, :4], gt[:1], HOUR, FPS, 0.5, 1.0, 100)      # no other scored class: no term
    assert one_class["per_class"][0]["efpr"] == [4.0]


def test_psds_from_counts_refuses_bad_shapes(pu):
    counts, gt = make_counts([[(0, 1)]], [1])
    with pytest.raises(ValueError):
        pu.psds_from_counts(counts[:, :, :3], gt, HOUR, FPS, 0.0, 1.0, 100)
    with pytest.raises(ValueError):
        pu.psds_from_counts(counts, gt, HOUR, 0.0, 0.0, 1.0, 100)
    empty = pu.psds_from_counts(counts, gt, 0, FPS, 0.0, 1.0, 100)
    assert math.isnan(empty["psds"]) and "frame" in empty["reason"]


# ---- helper, options, CLI -----------------------------------------------------------------------------------------------------------
def test_criterion_fraction_and_scenarios(pu):
    assert pu.criterion_fraction(0.7) == (7, 10) and pu.criterion_fraction(0.1) == (1, 10) and pu.criterion_fraction(1) == (1, 1)
    assert pu.criterion_fraction(0.3) == (3, 10) and pu.criterion_fraction((2, 3)) == (2, 3) and pu.criterion_fraction("0.25") == (1, 4)
    assert pu.criterion_fraction(1 / 3) == (1, 3)
    for bad in (0, 0.0, 1.5, -0.1, (3, 2), (0, 5), (1, 2 ** 15 + 1), float("nan"), (1, 2, 3)):
        with pytest.raises(ValueError):
            pu.criterion_fraction(bad)
    assert pu.SCENARIOS == {1: dict(dtc=(7, 10), gtc=(7, 10), cttc=(3, 10), alpha_ct=0.0, alpha_st=1.0, e_max=100),
                            2: dict(dtc=(1, 10), gtc=(1, 10), cttc=(3, 10), alpha_ct=0.5, alpha_st=1.0, e_max=100)}
    s = pu.resolve_scenario(dict(dtc=0.5, gtc=(7, 10), cttc=0.3, alpha_ct=1, alpha_st=0, e_max=50))
    assert s["dtc"] == (1, 2) and s["cttc"] == (3, 10) and s["e_max"] == 50.0
    assert pu.resolve_scenario(2)["alpha_ct"] == 0.5
    for bad in (0, 3, "1", True, dict(dtc=0.5), dict(pu.SCENARIOS[1], e_max=0), dict(pu.SCENARIOS[1], alpha_st=-1)):
        with pytest.raises(ValueError):
            pu.resolve_scenario(bad)
    th = pu.check_thresholds(None)
    assert th.dtype == np.float32 and len(th) == 50 and th[0] == np.float32(0.01) and th[-1] == np.float32(0.99)
    for bad in ([], np.zeros(65), [0.5, float("nan")]):
        with pytest.raises(ValueError):
            pu.check_thresholds(bad)


def test_device_functions_refuse_cpu_tensors(pu):
    import torch
    with pytest.raises(RuntimeError, match="CUDA|no CPU path"):
        pu.PsdsAccumulator(3, "cpu")
    with pytest.raises(RuntimeError, match="CUDA|no CPU path"):
        pu.psds_device(torch.zeros(1, 4, 2), torch.zeros(1, 4, 2), 10.0)
    for kw in (dict(K=0), dict(K=65), dict(median_window=4), dict(scenario=3), dict(thresholds=[])):
        with pytest.raises(ValueError):
            pu.PsdsAccumulator(**dict(dict(K=3, device="cpu"), **kw))


def test_argument_validation_without_gpu(sed):
    import ctypes as C
    lib = sed._lib.lib()
    assert lib.sed_psds_max_frames(16, 64) >= 8192 and lib.sed_psds_max_frames(14, 50) >= 8192
    assert lib.sed_psds_max_frames(14, 50) % 64 == 0
    assert lib.sed_psds_max_frames(0, 1) == 0 and lib.sed_psds_max_frames(65, 1) == 0
    assert lib.sed_psds_max_frames(1, 0) == 0 and lib.sed_psds_max_frames(1, 65) == 0
    th = (C.c_float * 2)(0.5, 0.6)

    def call(B=1, T=10, Tt=10, K=3, th=th, nth=2, crit=(7, 10, 7, 10, 3, 10)):
        return lib.sed_psds_counts(None, None, B, T, Tt, K, th, nth, *crit, None, None, None)

    for kw, text in ((dict(K=0), b"K in 1..64"), (dict(K=65), b"K in 1..64"), (dict(nth=0), b"nth"), (dict(nth=65), b"nth"),
                     (dict(B=65536), b"B in 0..65535"), (dict(T=-1), b"T >= 0"), (dict(crit=(0, 10, 7, 10, 3, 10)), b"fractions"),
                     (dict(crit=(7, 10, 11, 10, 3, 10)), b"fractions"), (dict(crit=(7, 10, 7, 10, 3, 2 ** 15 + 1)), b"fractions"),
                     (dict(T=lib.sed_psds_max_frames(3, 2) + 1, Tt=2 ** 30), b"sed_psds_max_frames"), (dict(th=None), b"null pointer"),
                     (dict(), b"null pointer")):
        assert call(**kw) != 0 and text in lib.sed_last_error(), kw
    assert call(T=0) == 0 and call(Tt=0) == 0 and call(B=0) == 0            # nothing to score: no launch
    with pytest.raises(RuntimeError, match="null pointer"):
        sed._lib.check(call(), "psds_counts")


def test_cli_flags_and_train_refusals(sed):
    main = importlib.import_module(PKG + ".main")
    train = importlib.import_module(PKG + ".train")
    a = main.build_full_parser().parse_args([])
    assert a.eval_psds is False and a.psds_scenario == 1 and a.psds_median_window == 0.0 and main.psds_eval_options(a, 50.0) is None
    assert vars(a).items() >= vars(main.build_parser().parse_args([])).items()          # every training flag, same defaults
    assert vars(main.build_psds_parser().parse_args([])).keys() == {"eval_psds", "psds_scenario", "psds_median_window"}
    spec = ["--train_features", "Spectogram", "--dataset_name", "synthetic"]
    a = main.build_full_parser().parse_args(spec + ["--eval_psds", "--psds_scenario", "2", "--psds_median_window", "0.14"])
    main.validate_args(a)
    assert main.psds_eval_options(a, 50.0) == {"scenario": 2, "fps": 50.0, "median_window": 7}
    assert main.psds_eval_options(main.build_full_parser().parse_args(spec + ["--eval_psds"]), 50.0)["median_window"] == 1
    with pytest.raises(SystemExit):
        main.build_full_parser().parse_args(spec + ["--psds_scenario", "3"])
    with pytest.raises(ValueError, match="psds_median_window"):
        main.validate_args(main.build_full_parser().parse_args(spec + ["--eval_psds", "--psds_median_window", "-1"]))
    with pytest.raises(ValueError, match="M5"):
        main.validate_args(main.build_full_parser().parse_args(["--train_features", "Waveform", "--eval_psds"]))
    prm = inspect.signature(train.train).parameters["psds_eval"]
    assert prm.default is None and prm.kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(train.eval_psds).parameters) == ["model", "dataloader", "device", "scenario", "thresholds",
                                                                   "median_window", "fps", "limit_val_samples"]
    assert inspect.signature(train.eval_psds).parameters["fps"].default is inspect.Parameter.empty
    # train() refuses before it touches a device or the loader
    cnn = sed.Cnn_AvgPooling(1, [(4, 2), (8, 2), (8, 2), (8, 1)])
    crit = sed.WeightedBCE(5, True)
    for bad in ({}, {"fps": 50.0, "collar": 1}, {"fps": 0.0}, {"fps": 50.0, "scenario": 3}, {"fps": 50.0, "median_window": 2},
                {"fps": 50.0, "thresholds": list(range(65))}):
        with pytest.raises(ValueError):
            train.train(cnn, None, crit, 1, 1e-3, 1, "unused", "cpu", psds_eval=bad)
    m5 = importlib.import_module(PKG + ".models.waveform_models").M5(1)
    with pytest.raises(ValueError, match="no time axis"):
        train.train(m5, None, sed.WeightedBCE(5, False), 1, 1e-3, 1, "unused", "cpu", psds_eval={"fps": 50.0})
    with pytest.raises(ValueError, match="no time axis"):
        train.check_psds_options(model=m5)
    assert train.check_psds_options(2, [0.5], 5, cnn)["dtc"] == (1, 10)
