"""Host side of the rank metrics (no GPU): the tests' own formula (tests/ranking_formula.py) against the pairwise definition of AUC,
against average precision in exact fractions and against sklearn; metrics_from_rank_counts (NaN rules, macro means, d', the strict
threshold); the C ABI's argument validation without a launch; the CLI flags and the signatures of the new layers."""
import importlib
import inspect
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from ranking_formula import auc_pairwise, counts_row, curve_formula, key_score, pack_formula, rank_formula

PKG = "soundeventdetection-pytorch_amd"
LIB = os.path.join(ROOT, PKG, "libsed_hip.so")


@pytest.fixture(scope="module")
def sed():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def ru():
    return importlib.import_module(PKG + ".utils.ranking_utils")


def tied_inputs(seed, n, levels, pos_rate=0.3):
    rng = np.random.default_rng(seed)
    score = (np.floor(rng.uniform(0, levels, n)) / levels).astype(np.float32)
    label = rng.uniform(size=n) < pos_rate
    return score, label


CASES = [(1, 7, 3), (2, 50, 4), (3, 200, 8), (4, 300, 2), (5, 300, 1000), (6, 123, 1)]


# ---- the formula itself ------------------------------------------------------------------------------------------------------------
def test_pack_formula_keys_order_like_score_then_label():
    score = np.array([[0.0], [-0.0], [1.0], [0.5], [0.5], [np.nan], [1.5], [-1e-9], [np.float32(1e-45)]], dtype=np.float32)
    target = np.array([[0], [1], [1], [0], [0.5000001], [1], [1], [1], [0.5]], dtype=np.float32)
    keys, invalid = pack_formula(score, target)
    assert invalid.tolist() == [3]
    one = int(np.float32(1.0).view(np.uint32))
    half = int(np.float32(0.5).view(np.uint32))
    assert keys[0].tolist() == [0, 1, 2 * one + 1, 2 * half, 2 * half + 1, 0, 0, 0, 2]      # -0 packs as +0; 0.5 is not positive
    assert int(keys.max()) < 2 ** 31
    assert key_score(2 * half + 1) == np.float32(0.5)
    # fewer target rows than score rows: the first min(rows) are scored
    k2, _ = pack_formula(score[:5], target[:3])
    assert k2.shape == (1, 3) and k2[0].tolist() == keys[0, :3].tolist()
    rng = np.random.default_rng(0)
    s = rng.uniform(0, 1, 200).astype(np.float32)
    l = (rng.uniform(size=200) < 0.5).astype(np.float32)
    k3, _ = pack_formula(s[:, None], l[:, None])
    order = np.argsort(k3[0], kind="stable")
    pairs = [(float(s[i]), float(l[i])) for i in order]
    assert pairs == sorted(pairs)


@pytest.mark.parametrize("seed,n,levels", CASES)
def test_auc_is_the_pairwise_probability(seed, n, levels):
    score, label = tied_inputs(seed, n, levels)
    res = rank_formula(score[:, None], label.astype(np.float32)[:, None])[0]
    P, neg = res["P"], res["n"] - res["P"]
    assert P == int(label.sum()) and res["n"] == n
    want = auc_pairwise(score, label)
    if want is None:
        assert P == 0 or neg == 0
    else:
        assert Fraction(res["auc2"], 2 * P * neg) == want
    assert res["groups"] == len(set(score.tolist()))


@pytest.mark.parametrize("seed,n,levels", CASES)
def test_ap_against_exact_fractions(seed, n, levels):
    score, label = tied_inputs(seed, n, levels)
    res = rank_formula(score[:, None], label.astype(np.float32)[:, None])[0]
    P = int(label.sum())
    if P == 0:
        assert math.isnan(res["AP"]) and counts_row(res)[3:5] == [0, 0] and res["best_score"] == np.float32(1.0)
        return
    exact, best = Fraction(0), None
    for th in sorted(set(score.tolist()), reverse=True):
        sel = score >= np.float32(th)
        here = score == np.float32(th)
        tp_g, TP, npred = int((label & here).sum()), int((label & sel).sum()), int(sel.sum())
        exact += Fraction(tp_g, P) * Fraction(TP, npred)
        f1 = Fraction(2 * TP, npred + P)
        if best is None or f1 > best[0]:
            best = (f1, TP, npred, th)
    G = res["groups"]
    assert abs(res["AP"] - float(exact)) <= (G + 8) * 2.0 ** -53 * float(exact)
    assert (res["best_tp"], res["best_npred"], float(res["best_score"])) == best[1:]


def test_f1_tie_goes_to_the_higher_score():
    # P = 2.  p >= 0.9: TP 1, 1 predicted, F1 = 2/3.  p >= 0.6: TP 1 of 2, F1 = 1/2.  p >= 0.3: TP 2 of 4, F1 = 2/3: a tie with the
    # first group, which must win
    keys, _ = pack_formula(np.array([[0.9], [0.6], [0.3], [0.3], [0.1]], dtype=np.float32),
                           np.array([[1], [0], [1], [0], [0]], dtype=np.float32))
    res = curve_formula(keys[0])
    assert (res["best_tp"], res["best_npred"], res["best_score"]) == (1, 1, np.float32(0.9))
    assert res["auc2"] == 2 * 3 * 2 - (2 + 1)              # 6 pairs; lost: (0.3+, 0.6-) fully, (0.3+, 0.3-) half
    assert curve_formula(np.zeros(0, dtype=np.uint32))["n"] == 0 and math.isnan(curve_formula([])["AP"])


@pytest.mark.parametrize("seed,n,levels", CASES[:5])
def test_formula_against_sklearn(seed, n, levels):
    sk = pytest.importorskip("sklearn.metrics")
    score, label = tied_inputs(seed, n, levels)
    res = rank_formula(score[:, None], label.astype(np.float32)[:, None])[0]
    P, neg = res["P"], res["n"] - res["P"]
    assert P > 0 and neg > 0, "the seeded cases hold both classes"
    assert res["AP"] == pytest.approx(sk.average_precision_score(label, score), rel=1e-12)
    assert res["auc2"] / (2 * P * neg) == pytest.approx(sk.roc_auc_score(label, score), rel=1e-12)
    prec, rec, th = sk.precision_recall_curve(label, score)
    f1 = 2 * prec[:-1] * rec[:-1] / np.maximum(prec[:-1] + rec[:-1], 1e-300)
    assert 2 * res["best_tp"] / (res["best_npred"] + P) == pytest.approx(f1.max(), rel=1e-12)


# ---- the GPU tests' data at corpus size: would a 32-bit product be noticed? -------------------------------------------------------
def walk_with_products_modulo(keys_sorted, bits):
    """(auc2, best_tp, best_npred) of an ascending row of keys by curve_formula's walk, with every integer PRODUCT taken modulo
    2^bits before it is added or compared -- bits = 32 is a kernel that lost a (u64) cast, bits = 64 the formula itself"""
    mask = (1 << bits) - 1
    k = np.asarray(keys_sorted, dtype=np.uint32)[::-1]
    start = np.flatnonzero(np.r_[True, (k[1:] >> np.uint32(1)) != (k[:-1] >> np.uint32(1))])
    size = np.diff(np.r_[start, k.size]).tolist()
    tp = np.add.reduceat((k & np.uint32(1)).astype(np.int64), start).tolist()
    P = sum(tp)
    auc2, TP, seen, best = 0, 0, 0, (0, 0)
    for tp_g, n_g in zip(tp, size):
        auc2 += ((n_g - tp_g) * (2 * TP + tp_g)) & mask
        TP += tp_g
        seen += n_g
        if best == (0, 0) or (TP * (best[1] + P)) & mask > (best[0] * (seen + P)) & mask:
            best = (TP, seen)
    return auc2, best[0], best[1]


def test_the_largest_gpu_size_would_notice_a_32_bit_product():
    """tests/test_gpu_ranking.py asserts that its reference rows pass 2^32 at CORPUS_SIZES[-1]; here the same rows go through the walk
    with 32-bit products, and the counts the GPU tests compare exactly come out different -- while at the largest of SIZES they
    come out the same, so the tests at those sizes could not tell.  Which rows tell: auc2 on every row with a group that holds
    many negatives ('distinct' has fp_g <= 1, so its products stay small and only its 64-bit SUM is at stake); the best-F1 point on
    'saturated' and 'f1 tie', whose candidates lie far apart -- on '8 levels' and 'distinct' the winner is next to 'predict
    everything', both sides of a comparison wrap alike, and the walk's choice survives."""
    gpu = importlib.import_module("test_gpu_ranking")
    big, small = gpu.CORPUS_SIZES[-1], gpu.SIZES[-1]
    keys, refs = gpu.corpus_case(big)
    assert gpu.CURVE_ROWS[5:7] == ("saturated", "f1 tie") and gpu.CURVE_ROWS[2] == "distinct"
    for row in range(len(refs)):
        want = tuple(counts_row(refs[row])[2:5])
        if refs[row]["P"]:
            assert walk_with_products_modulo(keys[row], 64) == want, "the walk is the formula's"
        lost = walk_with_products_modulo(keys[row], 32)
        if row in (0, 1, 5, 6, 7):
            assert lost[0] != want[0], (row, "auc2 survives 32-bit products")
        if row in (5, 6):
            assert lost[1:] != want[1:], (row, "the best-F1 point survives 32-bit products")
        if row in (0, 1, 2, 5, 6, 7):
            assert want[0] > 2 ** 32, (row, "auc2 survives a 32-bit sum")
    keys, refs = gpu.curve_case(small)
    for row in range(len(refs)):
        if refs[row]["P"]:
            assert walk_with_products_modulo(keys[row], 32) == tuple(counts_row(refs[row])[2:5]), (row, small)


# ---- host arithmetic of the package ------------------------------------------------------------------------------------------------
def test_metrics_from_rank_counts(ru):
    from scipy.stats import norm
    half = np.float32(0.5)
    #         P  n   auc2 btp bnp groups
    counts = [[2, 5, 9, 1, 1, 4],          # AUC 9 / 12
              [0, 5, 0, 0, 0, 3],          # no positive: everything NaN
              [5, 5, 0, 5, 5, 2],          # no negative: AP and F1 defined, AUC NaN
              [3, 10, 42, 3, 3, 10]]       # perfect ranking
    ap = [0.75, float("nan"), 1.0, 1.0]
    best = np.array([0.9, 1.0, 0.25, 0.5], dtype=np.float32)
    m = ru.metrics_from_rank_counts(ap, counts, best)
    c = m["per_class"]
    assert c[0]["AUC"] == 0.75 and c[0]["AP"] == 0.75 and c[0]["best_f1"] == 2 / 3 and c[0]["positives"] == 2 and c[0]["n"] == 5
    assert c[0]["d_prime"] == math.sqrt(2.0) * norm.ppf(0.75)
    assert all(math.isnan(c[1][k]) for k in ("AP", "AUC", "d_prime", "best_f1")) and c[1]["best_threshold"] == 1.0
    assert c[2]["AP"] == 1.0 and c[2]["best_f1"] == 1.0 and math.isnan(c[2]["AUC"]) and math.isnan(c[2]["d_prime"])
    assert c[3]["AUC"] == 1.0 and c[3]["d_prime"] == float("inf")
    assert c[3]["best_threshold"] == 0.5 and c[3]["best_threshold_strict"] == float(np.nextafter(half, np.float32(-1)))
    assert np.float32(c[3]["best_threshold_strict"]) < half and not (half > np.float32(c[3]["best_threshold"]))
    assert m["classes_scored"] == 3 and m["classes_scored_auc"] == 2
    assert m["mAP"] == pytest.approx((0.75 + 1.0 + 1.0) / 3) and m["mAUC"] == pytest.approx((0.75 + 1.0) / 2)
    assert m["mean_best_f1"] == pytest.approx((2 / 3 + 1 + 1) / 3) and m["mean_d_prime"] == float("inf")
    import json
    json.dumps(m)
    none = ru.metrics_from_rank_counts([float("nan")], [[0, 0, 0, 0, 0, 0]], [1.0])
    assert math.isnan(none["mAP"]) and math.isnan(none["mAUC"]) and none["classes_scored"] == 0
    with pytest.raises(ValueError):
        ru.metrics_from_rank_counts([0.5, 0.5], [[1, 2, 1, 1, 1, 2]], [0.5])


def test_metrics_from_rank_counts_follow_the_formula(ru):
    score, label = tied_inputs(11, 200, 8)
    res = rank_formula(score[:, None], label.astype(np.float32)[:, None])[0]
    m = ru.metrics_from_rank_counts([res["AP"]], [counts_row(res)], [res["best_score"]])["per_class"][0]
    assert Fraction(m["AUC"]) == Fraction(float(auc_pairwise(score, label)))
    dec = score >= np.float32(m["best_threshold"])
    strict = score > np.float32(m["best_threshold_strict"])
    assert np.array_equal(dec, strict) and int(dec.sum()) == res["best_npred"] and int((dec & label).sum()) == res["best_tp"]


def test_device_functions_refuse_cpu_tensors(ru):
    import torch
    with pytest.raises(RuntimeError, match="CUDA|no CPU path"):
        ru.RankingAccumulator(3, "cpu")
    with pytest.raises(RuntimeError, match="CUDA|no CPU path"):
        ru.ranking_metrics_device(torch.zeros(4, 2), torch.zeros(4, 2))


# ---- C ABI: argument validation without a launch ---------------------------------------------------------------------------------
def test_argument_validation_without_gpu(sed):
    lib = sed._lib.lib()
    tile = lib.sed_rank_tile()
    assert tile >= 64 and tile % 64 == 0
    assert lib.sed_rank_ws_bytes(0, 10) == 0 and lib.sed_rank_ws_bytes(65536, 10) == 0 and lib.sed_rank_ws_bytes(1, 2 ** 30 + 1) == 0
    assert lib.sed_rank_ws_bytes(14, 600100) >= 14 * 600100 * 4 and lib.sed_rank_ws_bytes(1, 0) > 0
    assert lib.sed_rank_ws_bytes(3, 2 * tile + 5) >= lib.sed_rank_ws_bytes(3, tile)
    rc = lib.sed_rank_pack(None, None, 5, 7, 3, None, 8, 4, None, None)            # 4 + min(5, 7) > 8
    assert rc != 0 and b"capacity" in lib.sed_last_error()
    with pytest.raises(RuntimeError, match="capacity"):
        sed._lib.check(rc, "rank_pack")
    rc = lib.sed_rank_pack(None, None, 5, 5, 0, None, 8, 0, None, None)
    assert rc != 0 and b"K in 1..65535" in lib.sed_last_error()
    rc = lib.sed_rank_pack(None, None, 5, 5, 3, None, 8, 0, None, None)
    assert rc != 0 and b"null pointer" in lib.sed_last_error()
    assert lib.sed_rank_pack(None, None, 0, 5, 3, None, 8, 8, None, None) == 0     # nothing to append: no launch
    rc = lib.sed_rank_sort(None, 3, 9, 8, None, None)
    assert rc != 0 and b"capacity" in lib.sed_last_error()
    rc = lib.sed_rank_sort(None, 3, 2 ** 30 + 1, 2 ** 31, None, None)
    assert rc != 0 and b"2^30" in lib.sed_last_error()
    rc = lib.sed_rank_sort(None, 3, 8, 8, None, None)
    assert rc != 0 and b"null pointer" in lib.sed_last_error()
    assert lib.sed_rank_sort(None, 3, 0, 0, None, None) == 0                       # empty rows: no launch
    rc = lib.sed_rank_curve(None, 3, 9, 8, None, None, None, None, None)
    assert rc != 0 and b"capacity" in lib.sed_last_error()
    rc = lib.sed_rank_curve(None, 70000, 8, 8, None, None, None, None, None)
    assert rc != 0 and b"K in 1..65535" in lib.sed_last_error()
    rc = lib.sed_rank_curve(None, 3, 0, 0, None, None, None, None, None)
    assert rc != 0 and b"null pointer" in lib.sed_last_error()


# ---- CLI and signatures --------------------------------------------------------------------------------------------------------------
def test_cli_flags_and_signatures(sed):
    main = importlib.import_module(PKG + ".main")
    train = importlib.import_module(PKG + ".train")
    a = main.build_full_parser().parse_args([])
    assert a.eval_ranking is False and a.eval_clip_pooling is None and main.ranking_eval_options(a) is None
    assert vars(a).items() >= vars(main.build_parser().parse_args([])).items()          # every training flag, same defaults
    assert vars(main.build_ranking_parser().parse_args([])).keys() == {"eval_ranking", "eval_clip_pooling"}
    spec = ["--train_features", "Spectogram", "--dataset_name", "synthetic"]
    a = main.build_full_parser().parse_args(spec + ["--eval_ranking"])
    main.validate_args(a)
    assert main.ranking_eval_options(a) == {}
    a = main.build_full_parser().parse_args(spec + ["--eval_ranking", "--eval_clip_pooling", "linear"])
    main.validate_args(a)
    assert main.ranking_eval_options(a) == {"clip_pooling": "linear"}
    with pytest.raises(SystemExit):
        main.build_full_parser().parse_args(spec + ["--eval_clip_pooling", "median"])
    with pytest.raises(ValueError, match="eval_ranking"):
        main.validate_args(main.build_full_parser().parse_args(spec + ["--eval_clip_pooling", "max"]))
    with pytest.raises(ValueError, match="M5"):
        main.validate_args(main.build_full_parser().parse_args(["--train_features", "Waveform", "--eval_ranking",
                                                                "--eval_clip_pooling", "max"]))
    main.validate_args(main.build_full_parser().parse_args(["--train_features", "Waveform", "--eval_ranking"]))
    prm = inspect.signature(train.train).parameters["ranking_eval"]
    assert prm.default is None and prm.kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(train.eval_ranking).parameters) == ["model", "dataloader", "device", "clip_pooling",
                                                                      "limit_val_samples"]
    with pytest.raises(ValueError):
        train.check_ranking_options("median")
    assert train.check_ranking_options(None) is None and train.check_ranking_options("exp") == "exp"
