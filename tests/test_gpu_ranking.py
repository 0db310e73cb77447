"""GPU: the rank-metric kernels of csrc/sed_rank.hip through the C ABI -- sed_rank_pack, sed_rank_sort, sed_rank_curve -- and the
layers on top of them (utils.ranking_utils, train.eval_ranking, train(ranking_eval=...)).

References: numpy's bit packing and np.sort for the first two steps, tests/ranking_formula.py (plain loops, checked on the host in
tests/test_ranking_host.py) for the curve.  No kernel of this library serves as a reference.  Keys, counts and the best score are
integers or selections: np.array_equal, no tolerance.  AP is a sum of G non-negative double terms, each with at most three roundings
(two divisions, one product), added in a fixed tree (at most G - 1 more): |AP - ref| <= (G + 8) * 2^-53 * ref against the formula's
math.fsum, G the number of tie groups.  Every output buffer starts filled with a sentinel and lies between two guard regions that
must be untouched afterwards.

Sizes: 1, 2, around the 64-lane ballot word, around the tile (sed_rank_tile) and several tiles plus a remainder (SIZES); and the
corpus sizes of train.eval_ranking, 5, 37 and 258 tiles (CORPUS_SIZES), at which the per-row loops over tiles of the table scan,
the row scan and the finishing kernel take more than one step and the 64-bit integers need their upper halves."""
import functools
import importlib
import json
import math

import numpy as np
import pytest
import torch

from ranking_formula import COUNT_NAMES, counts_row, curve_formula, pack_formula, rank_formula

pytestmark = pytest.mark.gpu

PKG = "soundeventdetection-pytorch_amd"
GUARD = 1024
FILL = {torch.float32: (float("nan"), -1024.0), torch.float64: (float("nan"), -1024.0), torch.int32: (-77, 0x5A5A5A5A),
        torch.uint8: (0x77, 0xA5), torch.int64: (-77, 0x5A5A5A5A5A5A)}
SIZES = [1, 2, 63, 64, 65, 2047, 2048, 2049, 6161]
CORPUS_SIZES = [8193, 73828, 526353]     # 5, 37 and 258 tiles: test_corpus_sizes_cover_the_tile_loops
WORST = {"ratio": 0.0}                   # worst |AP - ref| / (2^-53 * ref) seen by this module, in units of the (G + 8) bound


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG)._lib


@pytest.fixture(scope="module")
def ru():
    return importlib.import_module(PKG + ".utils.ranking_utils")


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


def u32(t):
    """an int32 device tensor as a numpy uint32 array"""
    return t.cpu().numpy().view(np.uint32)


def as_dev_keys(keys):
    return torch.from_numpy(np.array(keys, dtype=np.uint32, order="C", copy=True).view(np.int32)).cuda()


def workspace(L, g, K, n):
    nb = L.lib().sed_rank_ws_bytes(K, n)
    assert nb > 0 and nb % 16 == 0
    ws = g.new(torch.uint8, nb)
    assert ws.data_ptr() % 16 == 0
    return ws


def test_sizes_cover_the_tile(L):
    tile = L.lib().sed_rank_tile()
    assert set(SIZES) == {1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 17}


def test_corpus_sizes_cover_the_tile_loops(L):
    """what each of CORPUS_SIZES is for, from the constants of csrc/sed_rank.hip: 4 scan groups (RK_SCAN_GROUPS), an unroll of 8 in
    rank_scan_kernel, 256 threads over the tiles of a row in rank_rowscan_kernel and rank_finish_kernel"""
    tile = L.lib().sed_rank_tile()
    assert CORPUS_SIZES == [4 * tile + 1, 36 * tile + 100, 257 * tile + 17]

    def groups(tiles):                   # rank_scan_kernel: tiles per scan group
        per = -(-tiles // 4)
        return [min(g * per + per, tiles) - min(g * per, tiles) for g in range(4)]

    tiles = [-(-n // tile) for n in CORPUS_SIZES]
    assert tiles == [5, 37, 258]
    assert groups(5) == [2, 2, 1, 0]                        # in-group loops run twice, a carry between groups, an empty group
    assert groups(37) == [10, 10, 10, 7]                    # the unrolled body (8) and its remainder (2, and 7 alone)
    assert max(groups(-(-n // tile)) for n in SIZES) == [1, 1, 1, 1], "SIZES never reach any of this"
    per = -(-258 // 256)                                    # rank_rowscan_kernel: tiles per thread
    assert per == 2 and [t for t in range(256) if min(t * per, 258) < 258][-1] == 128      # threads 129..255 own nothing
    assert [t for t in range(256) if t + 256 < 258] == [0, 1]                               # rank_finish_kernel: a second step
    assert CORPUS_SIZES[-1] ** 2 // 8 > 2 ** 32 > SIZES[-1] ** 2           # n^2 / 8, the scale of auc2 at 30 % positives


# ---- pack --------------------------------------------------------------------------------------------------------------------------
def pack_inputs(rows_s, rows_t, K, seed):
    rng = np.random.default_rng(seed)
    score = rng.uniform(0, 1, (rows_s, K)).astype(np.float32)
    score[rng.uniform(size=score.shape) < 0.1] = np.float32(0.0)
    score[rng.uniform(size=score.shape) < 0.1] = np.float32(1.0)
    score[rng.uniform(size=score.shape) < 0.05] = np.float32(-0.0)
    target = (rng.uniform(size=(rows_t, K)) < 0.3).astype(np.float32)
    target[rng.uniform(size=target.shape) < 0.05] = np.float32(0.5)          # 0.5 is not positive (strict)
    return score, target


def packed_by_numpy(score, target):
    """the packing as array operations -- the bit-for-bit reference of the kernel; tests/ranking_formula.pack_formula is the loop"""
    n = min(len(score), len(target))
    s, t = score[:n], target[:n]
    with np.errstate(invalid="ignore"):
        ok = (s >= 0) & (s <= 1)
    bits = (s + np.float32(0.0)).view(np.uint32).astype(np.uint64)
    keys = np.where(ok, (bits << np.uint64(1)) | (t > np.float32(0.5)), 0).astype(np.uint32)
    return np.ascontiguousarray(keys.T), (~ok).sum(axis=0).astype(np.int64)


def run_pack(L, keys_dev, invalid_dev, score, target, K, capacity, offset):
    s, t = torch.from_numpy(score).cuda(), torch.from_numpy(target).cuda()
    L.check(L.lib().sed_rank_pack(L.ptr(s), L.ptr(t), score.shape[0], target.shape[0], K, L.ptr(keys_dev), capacity, offset,
                                  L.ptr(invalid_dev), stream()), "rank_pack")


@pytest.mark.parametrize("K", [1, 3, 14, 40, 527])
def test_pack_is_the_numpy_packing(L, K):
    """K = 527: 17 column blocks of PK_COLS = 32 classes in rank_pack_kernel, the last one 15 wide (blockIdx.y up to 16)"""
    for rows_s, rows_t, offset, extra in ((1, 1, 0, 0), (255, 300, 7, 5), (256, 256, 0, 1), (700, 513, 300, 64), (257, 257, 1, 0)):
        score, target = pack_inputs(rows_s, rows_t, K, seed=K * 1000 + rows_s)
        n = min(rows_s, rows_t)
        capacity = offset + n + extra
        g = Guards()
        keys = g.new(torch.int32, K, capacity)
        invalid = g.new(torch.int64, K)
        invalid.zero_()
        run_pack(L, keys, invalid, score, target, K, capacity, offset)
        g.intact()
        want, winv = packed_by_numpy(score, target)
        got = u32(keys)
        assert np.array_equal(got[:, offset:offset + n], want), (K, rows_s, rows_t, offset)
        if n <= 300 and n * K <= 300 * 40:                                    # the loop form, where it is quick
            assert np.array_equal(want, pack_formula(score, target)[0])
        sentinel = np.uint32(FILL[torch.int32][0] & 0xFFFFFFFF)
        assert bool((got[:, :offset] == sentinel).all()) and bool((got[:, offset + n:] == sentinel).all()), "columns outside"
        assert np.array_equal(invalid.cpu().numpy(), winv) and int(winv.sum()) == 0


def test_pack_two_appends_equal_one(L):
    K, n1, n2 = 14, 300, 411
    score, target = pack_inputs(n1 + n2, n1 + n2, K, seed=5)
    g = Guards()
    one, two = g.new(torch.int32, K, n1 + n2), g.new(torch.int32, K, n1 + n2)
    inv1, inv2 = g.new(torch.int64, K), g.new(torch.int64, K)
    inv1.zero_(); inv2.zero_()
    run_pack(L, one, inv1, score, target, K, n1 + n2, 0)
    run_pack(L, two, inv2, score[:n1], target[:n1], K, n1 + n2, 0)
    run_pack(L, two, inv2, np.ascontiguousarray(score[n1:]), np.ascontiguousarray(target[n1:]), K, n1 + n2, n1)
    g.intact()
    assert np.array_equal(u32(one), u32(two)) and np.array_equal(u32(one), packed_by_numpy(score, target)[0])


def test_pack_special_values_and_invalid_counts(L):
    K = 3
    score = np.zeros((70, K), dtype=np.float32)
    score[:, 0] = [-0.0, 0.0, 1.0, np.nan, 1.5, -1e-9, np.float32(1e-45), 0.5, np.inf, -np.inf] * 7
    score[:, 1] = 0.25
    score[:, 2] = np.nextafter(np.float32(1.0), np.float32(2.0))             # just above 1: invalid everywhere
    target = np.ones((70, K), dtype=np.float32)
    g = Guards()
    keys, invalid = g.new(torch.int32, K, 70), g.new(torch.int64, K)
    invalid.fill_(10)                                                         # the counts are ADDED
    run_pack(L, keys, invalid, score, target, K, 70, 0)
    g.intact()
    want, winv = packed_by_numpy(score, target)
    fk, finv = pack_formula(score, target)
    assert np.array_equal(want, fk) and np.array_equal(winv, finv) and winv.tolist() == [35, 0, 70]
    assert np.array_equal(u32(keys), want) and invalid.cpu().tolist() == [45, 10, 80]
    assert u32(keys)[0, :3].tolist() == [1, 1, (0x3F800000 << 1) | 1] and u32(keys)[0, 3:6].tolist() == [0, 0, 0]


# ---- sort --------------------------------------------------------------------------------------------------------------------------
def sort_key_sets(n, seed):
    """rows: keys that differ only in the lowest byte, only in the highest used byte (bits 24..30), all equal, two values, random"""
    rng = np.random.default_rng(seed)
    low = (np.uint32(0x3F123400) + rng.integers(0, 256, n).astype(np.uint32)).astype(np.uint32)
    high = ((rng.integers(0, 128, n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00ABCDEF)).astype(np.uint32)
    equal = np.full(n, 0x7F000001, dtype=np.uint32)
    two = np.where(rng.uniform(size=n) < 0.5, np.uint32(0x7FFFFFFF), np.uint32(0)).astype(np.uint32)
    rand = rng.integers(0, 2 ** 31, n).astype(np.uint32)
    return np.stack([low, high, equal, two, rand])


def run_sort(L, keys, n):
    """keys numpy (K, capacity) uint32 -> the whole buffer after sorting the first n of every row"""
    K, capacity = keys.shape
    g = Guards()
    buf = g.new(torch.int32, K, capacity)
    buf.copy_(as_dev_keys(keys))
    ws = workspace(L, g, K, n)
    L.check(L.lib().sed_rank_sort(L.ptr(buf), K, n, capacity, L.ptr(ws), stream()), "rank_sort")
    g.intact()
    return u32(buf)


@pytest.mark.parametrize("n", SIZES)
def test_sort_is_np_sort(L, n):
    for extra in (0, 37):
        keys = np.concatenate([sort_key_sets(n, n), np.full((5, extra), 0xDEADBEEF, dtype=np.uint32)], axis=1)
        got = run_sort(L, keys, n)
        assert np.array_equal(got[:, :n], np.sort(keys[:, :n], axis=1)), (n, extra)
        assert np.array_equal(got[:, n:], keys[:, n:]), "the tail of a row was touched"
    one = run_sort(L, keys[4:5], n)                                           # K = 1
    assert np.array_equal(one[:, :n], np.sort(keys[4:5, :n], axis=1))
    part = run_sort(L, keys, n // 2)                                          # n < capacity by a lot: the rest is left alone
    assert np.array_equal(part[:, :n // 2], np.sort(keys[:, :n // 2], axis=1)) and np.array_equal(part[:, n // 2:], keys[:, n // 2:])


@pytest.mark.parametrize("n", CORPUS_SIZES)
def test_sort_is_np_sort_at_corpus_size(L, n):
    """rank_scan_kernel with more than one tile per scan group: 5 tiles (groups of 2, 2, 1, 0: the in-group loops twice, the
    gsum carry, an empty group), 37 tiles (10, 10, 10, 7: the unrolled body and its remainder), 258 tiles.  The rows 'equal' and
    'two' put one digit in every tile, so every tile's base is a carry over all the tiles before it, and the order of equal digits
    across tiles (the stability the LSD passes rest on) is decided by this scan alone."""
    keys = np.concatenate([sort_key_sets(n, n), np.full((5, 37), 0xDEADBEEF, dtype=np.uint32)], axis=1)
    got = run_sort(L, keys, n)
    assert np.array_equal(got[:, :n], np.sort(keys[:, :n], axis=1)), n
    assert np.array_equal(got[:, n:], keys[:, n:]), "the tail of a row was touched"
    one = run_sort(L, keys[4:5], n)                                           # K = 1
    assert np.array_equal(one[:, :n], np.sort(keys[4:5, :n], axis=1)) and np.array_equal(one[:, n:], keys[4:5, n:])


# ---- curve -------------------------------------------------------------------------------------------------------------------------
CURVE_ROWS = ("8 levels", "one group over tiles", "distinct", "no positive", "only positives", "saturated", "f1 tie")


def curve_scores(n, seed):
    """(n, 7) scores and targets, one column per row of CURVE_ROWS"""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 7), dtype=np.float32)
    t = (rng.uniform(size=(n, 7)) < 0.3).astype(np.float32)
    s[:, 0] = np.floor(rng.uniform(0, 8, n)) / 8
    s[:, 1] = np.where(rng.uniform(size=n) < 0.9, 0.5, rng.uniform(0, 1, n))          # one tie group holds ~90 % of the row
    s[:, 2] = (rng.permutation(n) + 1.0) / (n + 2.0)
    s[:, 3] = rng.uniform(0, 1, n); t[:, 3] = 0.0
    s[:, 4] = np.floor(rng.uniform(0, 50, n)) / 50; t[:, 4] = 1.0
    s[:, 5] = (rng.uniform(size=n) < 0.5)
    a = n // 5                                                               # a+ at 0.9, a- at 0.6, a+ and a- at 0.3, the rest - at 0.1:
    s[:, 6] = 0.1; t[:, 6] = 0.0                                             # F1(0.9) = 2a / 3a = F1(0.3) = 4a / 6a > F1(0.6) = 1/2
    s[:a, 6] = 0.9; t[:a, 6] = 1.0
    s[a:2 * a, 6] = 0.6
    s[2 * a:4 * a, 6] = 0.3; t[2 * a:3 * a, 6] = 1.0
    perm = rng.permutation(n)
    return np.ascontiguousarray(s[perm]), np.ascontiguousarray(t[perm])


@functools.lru_cache(maxsize=None)
def curve_case(n):
    """(sorted keys (7, n), the formula's per-row results): computed once per size, shared, never modified"""
    score, target = curve_scores(n, seed=77 + n)
    keys, invalid = packed_by_numpy(score, target)
    assert int(invalid.sum()) == 0
    keys = np.sort(keys, axis=1)
    keys.setflags(write=False)
    return keys, tuple(curve_formula(row) for row in keys)


def run_curve(L, keys_sorted, n, capacity=None):
    """keys_sorted numpy (K, >= n) -> (ap (K,), counts (K, 6), best_score (K,)) as numpy, through guarded buffers"""
    K = keys_sorted.shape[0]
    capacity = keys_sorted.shape[1] if capacity is None else capacity
    g = Guards()
    ap, counts, best = g.new(torch.float64, K), g.new(torch.int64, K, 6), g.new(torch.float32, K)
    ws = workspace(L, g, K, n)
    kd = as_dev_keys(keys_sorted) if keys_sorted.size else None
    L.check(L.lib().sed_rank_curve(L.ptr(kd), K, n, capacity, L.ptr(ap), L.ptr(counts), L.ptr(best), L.ptr(ws), stream()),
            "rank_curve")
    g.intact()
    if kd is not None:
        assert np.array_equal(u32(kd), keys_sorted), "the keys were modified"
    return ap.cpu().numpy(), counts.cpu().numpy(), best.cpu().numpy()


def check_curve(got, refs, what):
    ap, counts, best = got
    for k, ref in enumerate(refs):
        tag = (what, k, {name: ref[name] for name in COUNT_NAMES})
        assert counts[k].tolist() == counts_row(ref), tag
        assert best[k].view(np.uint32) == np.float32(ref["best_score"]).view(np.uint32), tag
        if ref["P"] == 0:
            assert math.isnan(ap[k]), tag
            continue
        err = abs(float(ap[k]) - ref["AP"])
        unit = 2.0 ** -53 * ref["AP"]
        ratio = err / unit / (ref["groups"] + 8)
        WORST["ratio"] = max(WORST["ratio"], ratio)
        print(f"AP {what} row {k}: G = {ref['groups']}, |err| = {err / unit:.2f} * 2^-53 * ref = {ratio:.4f} of the bound")
        assert err <= (ref["groups"] + 8) * unit, tag


@pytest.mark.parametrize("n", SIZES)
def test_curve_is_the_formula(L, n):
    keys, refs = curve_case(n)
    check_curve(run_curve(L, keys, n), refs, f"n = {n}")
    if n >= 5:
        assert counts_row(refs[6])[3:5] == [n // 5, n // 5] and refs[6]["best_score"] == np.float32(0.9), "the tie case ties"
    assert refs[3]["P"] == 0 and refs[4]["P"] == n
    if n >= 2048:
        assert refs[1]["groups"] < n // 5 and refs[2]["groups"] == n
    # rows longer than n (capacity > n) and a single row
    wide = np.concatenate([keys, np.full((7, 19), 0xFFFFFFFF, dtype=np.uint32)], axis=1)
    check_curve(run_curve(L, wide, n), refs, f"n = {n}, capacity = n + 19")
    check_curve(run_curve(L, np.ascontiguousarray(keys[1:2]), n), refs[1:2], f"n = {n}, K = 1")
    print(f"worst AP error so far: {WORST['ratio']:.4f} of the (G + 8) * 2^-53 * ref bound")


EQUAL_SCORE = np.float32(0.375)


@functools.lru_cache(maxsize=None)
def corpus_case(n):
    """curve_case(n) and an eighth row, 'all equal': every score EQUAL_SCORE, mixed labels -- one tie group over the whole row.
    (sorted keys (8, n), the formula's per-row results): computed once per size, shared, never modified"""
    keys7, refs7 = curve_case(n)
    labels = (np.random.default_rng(1000 + n).uniform(size=n) < 0.3).astype(np.uint32)
    row = np.sort((np.uint32(EQUAL_SCORE.view(np.uint32)) << np.uint32(1)) | labels)
    keys = np.concatenate([keys7, row[None]], axis=0)
    keys.setflags(write=False)
    return keys, refs7 + (curve_formula(row),)


@pytest.mark.parametrize("n", CORPUS_SIZES)
def test_curve_is_the_formula_at_corpus_size(L, n):
    """the suffix scan over many tiles: rank_rowscan_kernel with per = 2 tiles per thread and threads 129..255 empty, and
    rank_finish_kernel's strided loop taking a second step in threads 0 and 1 (both at 258 tiles, the largest size); tie groups
    that span hundreds of tiles ('one group over tiles', 'all equal'); and, at the largest size, 64-bit products that need their
    upper halves: auc2 = sum fp_g (2 S(i') + tp_g) and better_point's tp (npred + P) pass 2^32, which the reference rows are
    asserted to do below (tests/test_ranking_host.py takes the same rows through 32-bit products: auc2 changes on every row with
    many negatives in a group, the best point on 'saturated' and 'f1 tie')."""
    tile = L.lib().sed_rank_tile()
    keys, refs = corpus_case(n)
    assert len(refs) == len(CURVE_ROWS) + 1
    # the eighth row: 1 group, so AP is the single term (P / P) * (P / n), auc2 the single product fp * tp, the best point the whole row
    e = refs[7]
    P = e["P"]
    assert 0 < P < n and counts_row(e) == [P, n, P * (n - P), P, n, 1] and e["best_score"] == EQUAL_SCORE
    assert e["AP"] == P / n
    assert refs[3]["P"] == 0 and refs[4]["P"] == n and refs[2]["groups"] == n and refs[1]["groups"] < n // 5
    assert counts_row(refs[6])[3:5] == [n // 5, n // 5] and refs[6]["best_score"] == np.float32(0.9), "the tie case ties"
    if n == CORPUS_SIZES[-1]:
        assert e["auc2"] > 2 ** 32, "one term of auc2 above 2^32"
        for r in (refs[0], refs[2], refs[5], refs[6]):                        # '8 levels', 'distinct', 'saturated', 'f1 tie'
            assert r["auc2"] > 2 ** 32 and r["best_tp"] * (r["best_npred"] + r["P"]) > 2 ** 32
        half = np.uint32(np.float32(0.5).view(np.uint32))
        assert int(((keys[1] >> np.uint32(1)) == half).sum()) > 200 * tile, "'one group over tiles': a tie group over 200 tiles"
    check_curve(run_curve(L, keys, n), refs, f"n = {n}")
    # rows longer than n (capacity > n) and a single row
    wide = np.concatenate([keys, np.full((8, 19), 0xFFFFFFFF, dtype=np.uint32)], axis=1)
    check_curve(run_curve(L, wide, n), refs, f"n = {n}, capacity = n + 19")
    check_curve(run_curve(L, np.ascontiguousarray(keys[1:2]), n), refs[1:2], f"n = {n}, K = 1")
    print(f"worst AP error so far: {WORST['ratio']:.4f} of the (G + 8) * 2^-53 * ref bound")


def test_curve_of_nothing(L):
    ap, counts, best = run_curve(L, np.zeros((3, 0), dtype=np.uint32), 0)
    assert np.isnan(ap).all() and counts.tolist() == [[0] * 6] * 3 and best.tolist() == [1.0] * 3
    refs = (curve_formula([]),) * 3
    check_curve((ap, counts, best), refs, "n = 0")


def test_pack_sort_curve_together(L):
    """the three calls in a row on raw scores, K = 14 with two appends, against the formula on the scores"""
    K, n1, n2 = 14, 2500, 1700
    score, target = pack_inputs(n1 + n2, n1 + n2, K, seed=9)
    score[:, 3] = np.round(score[:, 3] * 16) / 16
    n, cap = n1 + n2, n1 + n2 + 100
    g = Guards()
    keys, invalid = g.new(torch.int32, K, cap), g.new(torch.int64, K)
    invalid.zero_()
    ws = workspace(L, g, K, n)
    ap, counts, best = g.new(torch.float64, K), g.new(torch.int64, K, 6), g.new(torch.float32, K)
    run_pack(L, keys, invalid, score[:n1], target[:n1], K, cap, 0)
    run_pack(L, keys, invalid, np.ascontiguousarray(score[n1:]), np.ascontiguousarray(target[n1:]), K, cap, n1)
    L.check(L.lib().sed_rank_sort(L.ptr(keys), K, n, cap, L.ptr(ws), stream()), "rank_sort")
    L.check(L.lib().sed_rank_curve(L.ptr(keys), K, n, cap, L.ptr(ap), L.ptr(counts), L.ptr(best), L.ptr(ws), stream()), "rank_curve")
    g.intact()
    check_curve((ap.cpu().numpy(), counts.cpu().numpy(), best.cpu().numpy()), rank_formula(score, target), "pack + sort + curve")


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 2049, 6161, CORPUS_SIZES[-1]])
def test_two_runs_give_the_same_bits(L, n):
    """at the largest size: 258 tiles, every loop over tiles with more than one step"""
    keys, _ = corpus_case(n) if n in CORPUS_SIZES else curve_case(n)
    shuffled = np.ascontiguousarray(np.random.default_rng(n).permuted(keys, axis=1))
    a, b = run_sort(L, shuffled, n), run_sort(L, shuffled, n)
    assert np.array_equal(a, b) and np.array_equal(a, keys)
    r1, r2 = run_curve(L, a, n), run_curve(L, a, n)
    for x, y in zip(r1, r2):
        assert x.tobytes() == y.tobytes()


# ---- layers ------------------------------------------------------------------------------------------------------------------------
def same_raw(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_accumulator_grows_and_equals_the_one_shot_call(ru):
    K = 3
    score, target = pack_inputs(9000, 9000, K, seed=21)
    s, t = torch.from_numpy(score).cuda(), torch.from_numpy(target).cuda()
    acc = ru.RankingAccumulator(K, "cuda", capacity=0)
    cuts = [0, 1, 700, 4097, 4100, 9000]
    for a, b in zip(cuts[:-2], cuts[1:-1]):
        acc.update(s[a:b], t[a:b])
    assert acc.n == 4100 and acc.capacity >= 4100
    first = acc.compute_raw()
    assert same_raw(first, acc.compute_raw()), "compute() twice"
    shot = ru.RankingAccumulator(K, "cuda", capacity=4100)
    shot.update(s[:4100], t[:4100])
    assert same_raw(first, shot.compute_raw())
    check_curve(first[:3], rank_formula(score[:4100], target[:4100]), "accumulator, 4100")
    acc.update(s[4100:], t[4100:8000])                                        # fewer target rows: 3900 more
    assert acc.n == 8000
    m = acc.compute()
    refs = rank_formula(score[:8000], target[:8000])
    check_curve(acc.compute_raw()[:3], refs, "accumulator, 8000")
    want = ru.metrics_from_rank_counts([r["AP"] for r in refs], [counts_row(r) for r in refs], [r["best_score"] for r in refs])
    for got_c, want_c in zip(m["per_class"], want["per_class"]):
        assert {k: v for k, v in got_c.items() if k != "AP"} == {k: v for k, v in want_c.items() if k != "AP"}
        assert got_c["AP"] == pytest.approx(want_c["AP"], rel=1e-12)
    assert m["classes_scored"] == K and m["mAUC"] == want["mAUC"]
    one = ru.ranking_metrics_device(s[:8000], t[:8000])
    assert json.dumps(one) == json.dumps(m)
    acc.reset()
    assert acc.n == 0
    acc.update(s[:700], t[:700])
    assert json.dumps(acc.compute()) == json.dumps(ru.ranking_metrics_device(s[:700], t[:700]))
    empty = ru.RankingAccumulator(K, "cuda").compute()
    assert empty["classes_scored"] == 0 and math.isnan(empty["mAP"]) and empty["per_class"][0]["n"] == 0


def test_accumulator_at_corpus_size(L, ru):
    """pack, sort and curve through RankingAccumulator(K = 2, capacity = 0) at 257 * tile + 17 elements per class (258 tiles: the
    multi-step loops of rank_scan_kernel, rank_rowscan_kernel and rank_finish_kernel, integers above 2^32), fed in uneven batches
    whose ends are multiples neither of rank_pack_kernel's 256 rows nor of the tile, so that the key buffer grows (with its copy)
    seven times and most appends start in the middle of a pack block"""
    tile = L.lib().sed_rank_tile()
    K, n = 2, 257 * tile + 17
    assert n == CORPUS_SIZES[-1]
    score, target = pack_inputs(n, n, K, seed=31)
    score[:, 1] = np.round(score[:, 1] * 64) / 64                             # 65 tie groups beside a nearly distinct column
    cuts = [0, 1, 700, 4097, 9001, 20003, 70001, 150001, 300003, n]
    assert all(c % 256 and c % tile for c in cuts[1:])
    s, t = torch.from_numpy(score).cuda(), torch.from_numpy(target).cuda()
    acc = ru.RankingAccumulator(K, "cuda", capacity=0)
    grown = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        before = acc.capacity
        acc.update(s[a:b], t[a:b])
        grown += acc.capacity != before
    assert acc.n == n and acc.capacity >= n and grown >= 7
    keys, invalid = packed_by_numpy(score, target)                            # (pack_formula is a Python loop over every element)
    assert int(invalid.sum()) == 0 and np.array_equal(u32(acc.keys[:, :n]), keys), "the appended keys"
    first = acc.compute_raw()
    shot = ru.RankingAccumulator(K, "cuda", capacity=n)
    shot.update(s, t)
    assert same_raw(first, shot.compute_raw()), "uneven appends and one append give different bits"
    assert np.array_equal(s.cpu().numpy(), score) and np.array_equal(t.cpu().numpy(), target), "an input was modified"
    refs = [curve_formula(row) for row in keys]
    assert all(r["auc2"] > 2 ** 32 and r["best_tp"] * (r["best_npred"] + r["P"]) > 2 ** 32 for r in refs)
    assert refs[1]["groups"] == 65 and refs[0]["groups"] > n // 2
    check_curve(first[:3], refs, f"accumulator, {n}")
    assert first[3].tolist() == [0, 0]


def test_accumulator_reports_invalid_scores(ru):
    s = torch.rand(100, 2, device="cuda")
    t = (torch.rand(100, 2, device="cuda") < 0.5).float()
    s[7, 1] = float("nan")
    s[9, 1] = 1.5
    acc = ru.RankingAccumulator(2, "cuda")
    acc.update(s, t)
    with pytest.raises(ValueError, match=r"\[0, 2\]"):
        acc.compute()
    with pytest.raises(ValueError):
        acc.update(s[:, :1], t[:, :1])
    with pytest.raises(RuntimeError):
        acc.update(s.cpu(), t.cpu())


TINY_CFG = [(4, 2), (8, 2), (8, 2), (8, 1)]


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


def check_metrics(got, refs, ru):
    want = ru.metrics_from_rank_counts([r["AP"] for r in refs], [counts_row(r) for r in refs], [r["best_score"] for r in refs])
    for got_c, want_c, r in zip(got["per_class"], want["per_class"], refs):
        assert json.dumps({k: v for k, v in got_c.items() if k != "AP"}) == json.dumps({k: v for k, v in want_c.items() if k != "AP"})
        if r["P"] == 0:
            assert math.isnan(got_c["AP"])
        else:
            assert abs(got_c["AP"] - r["AP"]) <= (r["groups"] + 8) * 2.0 ** -53 * r["AP"]
    assert got["classes_scored"] == want["classes_scored"] and json.dumps(got["mAUC"]) == json.dumps(want["mAUC"])


def test_eval_ranking_matches_the_formula(ru):
    sed, model, loader = tiny_model_and_loader()
    mu = importlib.import_module(PKG + ".utils.metric_utils")
    crit = sed.WeightedBCE(5, True)
    dev = torch.device("cuda:0")
    before = sed.train.eval(model, loader, crit, None, 0, dev)
    # the probabilities the evaluation produces, once, on the host
    probs, tgts, clip_p, clip_t = [], [], [], []
    for inp, target, _ in loader.dataset.get_validation_sampler(None):
        model.eval()
        with torch.no_grad():
            out = model(inp.cuda().float())[0]
        tg = target[0].cuda().float()
        p = mu.metric_counts_device(out, tg, raw_logits=True, return_probs=True)[3]
        plan = model.engine.plan(inp.shape[0], inp.shape[2], inp.shape[3], out.device)
        clip_p.append(model.engine.clip_probs(plan, "linear")[:1].cpu().numpy().copy())
        probs.append(p.cpu().numpy())
        tgts.append(tg[:p.shape[0]].cpu().numpy())
        clip_t.append(tgts[-1].max(axis=0, keepdims=True))
    got = sed.train.eval_ranking(model, loader, dev)
    assert "clip" not in got and got["n_recordings"] == 3
    refs = rank_formula(np.concatenate(probs), np.concatenate(tgts))
    assert refs[0]["n"] == sum(len(p) for p in probs) and sum(r["P"] for r in refs) > 0
    check_metrics(got, refs, ru)
    json.dumps(got)
    with_clip = sed.train.eval_ranking(model, loader, dev, clip_pooling="linear")
    check_metrics(with_clip, refs, ru)
    crefs = rank_formula(np.concatenate(clip_p), np.concatenate(clip_t))
    assert crefs[0]["n"] == 3 and with_clip["clip"]["pooling"] == "linear"
    check_metrics(with_clip["clip"], crefs, ru)
    two = sed.train.eval_ranking(model, loader, dev, limit_val_samples=2)
    assert two["n_recordings"] == 2 and two["per_class"][0]["n"] == len(probs[0]) + len(probs[1])
    with pytest.raises(ValueError):
        sed.train.eval_ranking(model, loader, dev, clip_pooling="median")
    # the reference evaluation is what it was
    after = sed.train.eval(model, loader, crit, None, 0, dev)
    assert before[0] == after[0] and before[3] == after[3]
    assert all(np.array_equal(a, b) for a, b in zip(before[1] + before[2], after[1] + after[2]))


def test_train_logs_the_ranking_record(tmp_path):
    sed, model0, loader = tiny_model_and_loader(seed=4)
    _, model, _ = tiny_model_and_loader(seed=4)
    crit = sed.WeightedBCE(5, True)
    plain, ranked = tmp_path / "plain", tmp_path / "ranked"
    sed.train.train(model0, loader, crit, 2, 1e-3, 2, str(plain), "cuda")
    sed.train.train(model, loader, crit, 2, 1e-3, 2, str(ranked), "cuda", ranking_eval={"clip_pooling": "max"})
    rec0 = json.loads(open(plain / "progress.jsonl").read().strip().splitlines()[-1])
    rec = json.loads(open(ranked / "progress.jsonl").read().strip().splitlines()[-1])
    assert "ranking" not in rec0 and set(rec) == set(rec0) | {"ranking"}
    r = rec["ranking"]
    assert {"per_class", "mAP", "mAUC", "mean_d_prime", "mean_best_f1", "classes_scored", "clip", "n_recordings"} <= set(r)
    assert set(r["per_class"][0]) == {"AP", "AUC", "d_prime", "best_f1", "best_threshold", "best_threshold_strict", "positives", "n"}
    assert len(r["per_class"]) == 3 and r["n_recordings"] == 3 and r["clip"]["per_class"][0]["n"] == 3
    with pytest.raises(ValueError):
        sed.train.train(model, loader, crit, 2, 1e-3, 2, str(ranked), "cuda", ranking_eval={"threshold": 0.5})
