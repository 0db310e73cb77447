"""Corpus-level rank metrics on the MI355X (csrc/sed_rank.hip): average precision, ROC-AUC, d' and the best-F1 operating point per
class, over everything a validation pass scored -- the numbers sound-event papers report, which the reference's 21-threshold,
per-recording metric (utils/metric_utils.py) is not.

The probabilities never leave the device: every (frames, K) batch is packed into one 32-bit key per element, key = (bits(p) << 1) |
(target > 0.5), appended class-major; compute() sorts the rows (a segmented radix sort, keys only) and scans them once, and brings
K * (8 + 48 + 4 + 8) bytes to the host.  The definitions (tie groups, AP as sklearn's average_precision_score, AUC with ties counted
half, the F1 tie rule) are those of include/sed_hip.h; every count is an integer, so the results are the same bits on every run.
The device functions take CUDA tensors and raise on CPU tensors: there is no CPU path.  metrics_from_rank_counts is host arithmetic."""
from __future__ import annotations

import math

import numpy as np

MAX_ELEMENTS = 1 << 30
MIN_CAPACITY = 4096


def metrics_from_rank_counts(ap, counts, best_score):
    """ap (K,) float64, counts (K, 6) integers (P, n, auc2, best_tp, best_npred, groups), best_score (K,) fp32 -- what
    sed_rank_curve writes -> the JSON-ready dict
      {'per_class': [{AP, AUC, d_prime, best_f1, best_threshold, best_threshold_strict, positives, n}],
       'mAP', 'mAUC', 'mean_d_prime', 'mean_best_f1', 'classes_scored', 'classes_scored_auc'}.
    AUC = auc2 / (2 P Nneg), d' = sqrt(2) * norm.ppf(AUC).  A class without a positive has AP and best_f1 NaN; one without a positive
    or without a negative has AUC and d' NaN.  The macro means run over the classes whose value is not NaN (NaN if there is none);
    classes_scored counts the classes with an AP, classes_scored_auc those with an AUC.  The decision rule of the best point is
    p >= best_threshold; best_threshold_strict = nextafter(best_threshold, -inf) in fp32 gives the same decisions under the
    package's strict p > th (infer.py --threshold)."""
    from scipy.stats import norm
    ap = np.asarray(ap, dtype=np.float64).reshape(-1)
    counts = np.asarray(counts).reshape(-1, 6)
    best_score = np.asarray(best_score, dtype=np.float32).reshape(-1)
    if not (len(ap) == len(counts) == len(best_score)):
        raise ValueError("ap, counts and best_score must describe the same classes")
    nan = float("nan")
    per_class = []
    for k in range(len(ap)):
        P, n, auc2, btp, bnp, _ = (int(v) for v in counts[k])
        neg = n - P
        auc = auc2 / (2 * P * neg) if P > 0 and neg > 0 else nan
        per_class.append({
            "AP": float(ap[k]) if P > 0 else nan,
            "AUC": auc,
            "d_prime": float(math.sqrt(2.0) * norm.ppf(auc)) if auc == auc else nan,
            "best_f1": 2.0 * btp / (bnp + P) if P > 0 else nan,
            "best_threshold": float(best_score[k]),
            "best_threshold_strict": float(np.nextafter(best_score[k], np.float32(-np.inf))),
            "positives": P, "n": n})

    def mean(name):
        vals = [c[name] for c in per_class if c[name] == c[name]]
        return float(np.mean(vals)) if vals else nan

    return {"per_class": per_class, "mAP": mean("AP"), "mAUC": mean("AUC"), "mean_d_prime": mean("d_prime"),
            "mean_best_f1": mean("best_f1"), "classes_scored": sum(1 for c in per_class if c["AP"] == c["AP"]),
            "classes_scored_auc": sum(1 for c in per_class if c["AUC"] == c["AUC"])}


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class RankingAccumulator:
    """Collects (score, label) keys of K classes on `device` over any number of update() calls.  keys: int32 tensor (K, capacity)
    holding the uint32 keys, the first `n` columns filled; invalid: (K,) int64 counts of NaN / out-of-range scores."""

    def __init__(self, K, device, capacity=0):
        import torch
        self.K, self.device = int(K), torch.device(device)
        if self.K < 1 or self.K > 65535:
            raise ValueError(f"K must be in 1..65535 (got {K})")
        if self.device.type != "cuda":
            raise RuntimeError("RankingAccumulator needs a CUDA device (there is no CPU path)")
        if int(capacity) < 0 or int(capacity) > MAX_ELEMENTS:
            raise ValueError(f"capacity must be in 0..2^30 (got {capacity})")
        self.capacity, self.n = int(capacity), 0
        self.keys = torch.empty(self.K, self.capacity, dtype=torch.int32, device=self.device)
        self.invalid = torch.zeros(self.K, dtype=torch.int64, device=self.device)

    def reset(self):
        """forget what was appended; the buffer keeps its capacity"""
        self.n = 0
        self.invalid.zero_()

    def _reserve(self, need):
        import torch
        if need <= self.capacity:
            return
        if need > MAX_ELEMENTS:
            raise ValueError(f"more than 2^30 scored elements per class ({need})")
        cap = min(MAX_ELEMENTS, max(need, 2 * self.capacity, MIN_CAPACITY))
        keys = torch.empty(self.K, cap, dtype=torch.int32, device=self.device)
        if self.n:
            keys[:, :self.n].copy_(self.keys[:, :self.n])
        self.keys, self.capacity = keys, cap

    def update(self, scores, target):
        """scores (rows, K) probabilities and target (rows', K) labels, CUDA tensors: the first min(rows, rows') rows are appended
        (one sed_rank_pack launch; no host synchronisation)."""
        import torch
        from .. import _lib as L
        if not (isinstance(scores, torch.Tensor) and isinstance(target, torch.Tensor) and scores.is_cuda and target.is_cuda):
            raise RuntimeError("RankingAccumulator.update needs CUDA tensors (there is no CPU path)")
        if scores.dim() != 2 or target.dim() != 2 or scores.shape[1] != self.K or target.shape[1] != self.K:
            raise ValueError(f"expected (rows, {self.K}) tensors, got {tuple(scores.shape)} / {tuple(target.shape)}")
        s = scores.detach().float().contiguous()
        t = target.detach().float().contiguous()
        n = min(s.shape[0], t.shape[0])
        if n == 0:
            return
        self._reserve(self.n + n)
        L.check(L.lib().sed_rank_pack(L.ptr(s), L.ptr(t), s.shape[0], t.shape[0], self.K, L.ptr(self.keys), self.capacity, self.n,
                                      L.ptr(self.invalid), _stream()), "rank_pack")
        self.n += n

    def compute_raw(self):
        """(ap float64 (K,), counts int64 (K, 6), best_score fp32 (K,), invalid int64 (K,)) as numpy arrays: sort and scan of a
        scratch copy (more updates may follow), then ONE device-to-host copy."""
        import torch
        from .. import _lib as L
        lib, K, n = L.lib(), self.K, self.n
        scratch = self.keys[:, :n].contiguous() if n else torch.empty(K, 0, dtype=torch.int32, device=self.device)
        if n and scratch.data_ptr() == self.keys.data_ptr():
            scratch = scratch.clone()
        ws_bytes = lib.sed_rank_ws_bytes(K, n)
        if ws_bytes == 0:
            raise ValueError(f"rank metrics: shape K={K}, n={n} is out of range")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        ap = torch.empty(K, dtype=torch.float64, device=self.device)
        counts = torch.empty(K, 6, dtype=torch.int64, device=self.device)
        best = torch.empty(K, dtype=torch.float32, device=self.device)
        st = _stream()
        L.check(lib.sed_rank_sort(L.ptr(scratch) if n else None, K, n, n, L.ptr(ws), st), "rank_sort")
        L.check(lib.sed_rank_curve(L.ptr(scratch) if n else None, K, n, n, L.ptr(ap), L.ptr(counts), L.ptr(best), L.ptr(ws), st),
                "rank_curve")
        host = torch.cat([ap.view(torch.uint8), counts.view(torch.uint8).reshape(-1), self.invalid.view(torch.uint8),
                          best.view(torch.uint8)]).cpu().numpy()
        a, b, c = 8 * K, 56 * K, 64 * K
        return (host[:a].view(np.float64).copy(), host[a:b].view(np.int64).reshape(K, 6).copy(), host[c:].view(np.float32).copy(),
                host[b:c].view(np.int64).copy())

    def compute(self):
        """the metrics_from_rank_counts dict of everything appended so far; raises ValueError if any score was NaN or outside
        [0, 1] (the per-class counts are in the message)"""
        ap, counts, best, invalid = self.compute_raw()
        if invalid.any():
            raise ValueError(f"rank metrics: scores that are NaN or outside [0, 1], per class: {invalid.tolist()}")
        return metrics_from_rank_counts(ap, counts, best)


def ranking_metrics_device(scores, target):
    """The rank metrics of one (rows, K) pair of CUDA tensors (RankingAccumulator: one update, one compute)."""
    n = min(int(scores.shape[0]), int(target.shape[0])) if scores.dim() == 2 and target.dim() == 2 else 0
    acc = RankingAccumulator(scores.shape[-1], scores.device, capacity=n)
    acc.update(scores, target)
    return acc.compute()
