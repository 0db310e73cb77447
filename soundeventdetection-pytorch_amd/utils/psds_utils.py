"""The polyphonic sound detection score (PSDS; Bilen et al., ICASSP 2020) on the MI355X (csrc/sed_psds.hip): the number DCASE
task 4 is ranked by.

The counting -- thresholds x recordings x classes x frames decisions, intersected with the ground truth under the DTC / GTC / CTTC
criteria -- is one launch per batch of recordings (sed_psds_counts) that ADDS integers into two small device arrays; compute()
copies those to the host once and psds_from_counts turns them into the score in float64.  The definitions are those of
include/sed_hip.h.  This is the project's own statement of PSDS on the FRAME GRID, not the psds_eval package: onsets and offsets
are whole frames, a class without a ground-truth event is left out of the score (the package raises), and no agreement run against
the package exists.  The device functions take CUDA tensors and raise on CPU tensors: there is no CPU path."""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction

import numpy as np

MAX_THRESHOLDS = 64
MAX_CLASSES = 64
MAX_BATCH = 65535
MAX_DEN = 1 << 15

# the DCASE 2021-23 task-4 settings
SCENARIOS = {1: dict(dtc=(7, 10), gtc=(7, 10), cttc=(3, 10), alpha_ct=0.0, alpha_st=1.0, e_max=100),
             2: dict(dtc=(1, 10), gtc=(1, 10), cttc=(3, 10), alpha_ct=0.5, alpha_st=1.0, e_max=100)}


def criterion_fraction(x):
    """A DTC / GTC / CTTC criterion as the integer fraction (num, den) the kernel compares with: a (num, den) pair is taken as it
    is, a number x becomes Fraction(str(x)).limit_denominator(1000) (0.7 -> (7, 10)).  0 < num <= den <= 2^15."""
    if isinstance(x, (tuple, list)):
        if len(x) != 2 or any(int(v) != v for v in x):
            raise ValueError(f"a criterion is a number in (0, 1] or a (num, den) pair of integers (got {x!r})")
        num, den = int(x[0]), int(x[1])
    else:
        if isinstance(x, float) and not math.isfinite(x):
            raise ValueError(f"a criterion is a number in (0, 1] (got {x!r})")
        f = Fraction(str(x)).limit_denominator(1000)
        num, den = f.numerator, f.denominator
    if not 0 < num <= den <= MAX_DEN:
        raise ValueError(f"a criterion is in (0, 1] with a denominator of at most 2^15 (got {x!r} -> {num}/{den})")
    return num, den


def resolve_scenario(scenario):
    """1, 2 or a dict with dtc, gtc, cttc, alpha_ct, alpha_st, e_max -> a checked copy whose criteria are (num, den) pairs."""
    if isinstance(scenario, dict):
        keys = {"dtc", "gtc", "cttc", "alpha_ct", "alpha_st", "e_max"}
        if set(scenario) != keys:
            raise ValueError(f"a PSDS scenario has the keys {sorted(keys)} (got {sorted(scenario)})")
        s = dict(scenario)
    elif scenario in SCENARIOS and not isinstance(scenario, bool):
        s = dict(SCENARIOS[scenario])
    else:
        raise ValueError(f"scenario is 1, 2 or a dict (got {scenario!r})")
    for name in ("dtc", "gtc", "cttc"):
        s[name] = criterion_fraction(s[name])
    s["alpha_ct"], s["alpha_st"], s["e_max"] = float(s["alpha_ct"]), float(s["alpha_st"]), float(s["e_max"])
    if not (s["alpha_ct"] >= 0 and s["alpha_st"] >= 0 and 0 < s["e_max"] < float("inf")):
        raise ValueError(f"alpha_ct and alpha_st must be >= 0 and e_max > 0 (got {s['alpha_ct']}, {s['alpha_st']}, {s['e_max']})")
    return s


def check_thresholds(thresholds):
    """1..64 finite thresholds, any order -> fp32 array"""
    th = np.linspace(0.01, 0.99, 50) if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if not 1 <= len(th) <= MAX_THRESHOLDS or not np.all(np.isfinite(th)):
        raise ValueError(f"1..{MAX_THRESHOLDS} finite thresholds are needed (got {len(th)})")
    return th.astype(np.float32)


def psds_from_counts(counts, gt, total_frames, fps, alpha_ct, alpha_st, e_max):
    """Host, float64.  counts (nth, K, K + 3) integers (tp, fp, ndet, ct[0..K-1]) and gt (K, 2) integers (events, frames) as
    sed_psds_counts leaves them; total_frames scored frames in all, fps frames per second.
      hours = total_frames / fps / 3600; a class is scored if it has a ground-truth event.  Per scored class k and threshold i:
      tpr = tp / n_gt[k], fpr = fp / hours, efpr = fpr + alpha_ct * mean over scored c != k of ct[c] / (gt_frames[c] / fps / 3600)
      (0 without another scored class).  The class curve: the points sorted by (efpr, tpr), tpr replaced by its running maximum;
      its value at e is the largest such tpr with efpr <= e, 0 before the first point (a right-continuous step function).  The
      common axis: every class's efpr in [0, e_max], sorted, unique, then e_max.  eff(e) = max(mean_k - alpha_st * std_k, 0) over
      the scored classes (population std).  PSDS = fsum_j eff(e_j) (e_{j+1} - e_j) / e_max.
    Returns {'psds', 'classes_scored', 'reason' (why psds is NaN, else None), 'per_class': [{'scored', 'n_gt', 'area', 'efpr',
    'tpr'}] (the curve's points after the running maximum), 'axis', 'eff', 'macro_f1' (per threshold, over the scored classes,
    F1 = 2 tp / (tp + fp + n_gt)), 'best_macro_f1', 'best_macro_f1_index'}.  Without a scored class psds is NaN and
    classes_scored 0."""
    counts = np.asarray(counts)
    gt = np.asarray(gt)
    if counts.ndim != 3 or counts.shape[2] != counts.shape[1] + 3 or gt.shape != (counts.shape[1], 2):
        raise ValueError(f"counts must be (nth, K, K + 3) and gt (K, 2) (got {counts.shape}, {gt.shape})")
    total_frames, fps, alpha_ct, alpha_st, e_max = int(total_frames), float(fps), float(alpha_ct), float(alpha_st), float(e_max)
    if not (total_frames >= 0 and fps > 0 and e_max > 0):
        raise ValueError(f"total_frames >= 0, fps > 0 and e_max > 0 are needed (got {total_frames}, {fps}, {e_max})")
    nth, K = counts.shape[0], counts.shape[1]
    nan = float("nan")
    scored = [k for k in range(K) if int(gt[k, 0]) >= 1]
    per_class = [{"scored": k in scored, "n_gt": int(gt[k, 0]), "area": nan, "efpr": [], "tpr": []} for k in range(K)]
    res = {"psds": nan, "classes_scored": len(scored), "reason": None, "per_class": per_class, "axis": [], "eff": [],
           "macro_f1": [nan] * nth, "best_macro_f1": nan, "best_macro_f1_index": None}
    if not scored:
        res["reason"] = "no class has a ground-truth event"
        return res
    if total_frames == 0:
        res["reason"] = "no frame was scored"
        return res
    hours = total_frames / fps / 3600.0
    gt_hours = {c: int(gt[c, 1]) / fps / 3600.0 for c in scored}
    curves = {}
    for k in scored:
        pts = []
        for i in range(nth):
            tpr = int(counts[i, k, 0]) / int(gt[k, 0])
            efpr = int(counts[i, k, 1]) / hours
            others = [c for c in scored if c != k]
            if others:
                efpr = efpr + alpha_ct * (math.fsum(int(counts[i, k, 3 + c]) / gt_hours[c] for c in others) / len(others))
            pts.append((efpr, tpr))
        pts.sort()
        best, xs, ys = 0.0, [], []
        for e, t in pts:
            best = max(best, t)
            xs.append(e)
            ys.append(best)
        curves[k] = (xs, ys)
        per_class[k]["efpr"], per_class[k]["tpr"] = xs, ys
    axis = sorted({e for k in scored for e in curves[k][0] if 0.0 <= e <= e_max}) + [e_max]

    def value(k, e):
        xs, ys = curves[k]
        j = int(np.searchsorted(np.asarray(xs), e, side="right"))       # the points with efpr <= e
        return ys[j - 1] if j > 0 else 0.0

    vals = np.array([[value(k, e) for e in axis[:-1]] for k in scored], dtype=np.float64).reshape(len(scored), len(axis) - 1)
    widths = [axis[j + 1] - axis[j] for j in range(len(axis) - 1)]
    eff = [max(float(np.mean(vals[:, j])) - alpha_st * float(np.std(vals[:, j])), 0.0) for j in range(len(widths))]
    res["psds"] = math.fsum(f * w for f, w in zip(eff, widths)) / e_max
    for r, k in enumerate(scored):
        per_class[k]["area"] = math.fsum(float(vals[r, j]) * widths[j] for j in range(len(widths))) / e_max
    res["axis"], res["eff"] = axis, eff
    f1 = [float(np.mean([2.0 * int(counts[i, k, 0]) / (int(counts[i, k, 0]) + int(counts[i, k, 1]) + int(gt[k, 0])) for k in scored]))
          for i in range(nth)]
    res["macro_f1"] = f1
    res["best_macro_f1_index"] = int(np.argmax(f1))
    res["best_macro_f1"] = f1[res["best_macro_f1_index"]]
    return res


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class PsdsAccumulator:
    """Sums the PSDS counts of K classes on `device` over any number of update() calls (recordings of any lengths).
    counts: int64 device tensor (nth, K, K + 3); gt: int64 (K, 2); total_frames: the scored frames so far (host, from shapes)."""

    def __init__(self, K, device, thresholds=None, scenario=1, median_window=1):
        import torch
        from .event_utils import MAX_MEDIAN_WINDOW
        self.K, self.device = int(K), torch.device(device)
        if not 1 <= self.K <= MAX_CLASSES:
            raise ValueError(f"K must be in 1..{MAX_CLASSES} (got {K})")
        self.thresholds = check_thresholds(thresholds)
        self.scenario = resolve_scenario(scenario)
        self.median_window = int(median_window)
        if self.median_window < 1 or self.median_window > MAX_MEDIAN_WINDOW or self.median_window % 2 == 0:
            raise ValueError(f"median window must be odd, 1..{MAX_MEDIAN_WINDOW} frames (got {median_window})")
        if self.device.type != "cuda":
            raise RuntimeError("PsdsAccumulator needs a CUDA device (there is no CPU path)")
        self._th = (C.c_float * len(self.thresholds))(*self.thresholds.tolist())
        self.counts = torch.zeros(len(self.thresholds), self.K, self.K + 3, dtype=torch.int64, device=self.device)
        self.gt = torch.zeros(self.K, 2, dtype=torch.int64, device=self.device)
        self.total_frames = 0

    def reset(self):
        """forget what was counted"""
        self.counts.zero_()
        self.gt.zero_()
        self.total_frames = 0

    def update(self, probs, target):
        """probs (B, T, K) or (T, K) probabilities and target (B, Tt, K) or (Tt, K) labels, CUDA tensors: the first min(T, Tt)
        frames of every recording are counted (an optional sed_median_time, then one sed_psds_counts; no host synchronisation)."""
        from .. import _lib as L
        from .event_utils import _as_btk, median_filter_time
        p3, _ = _as_btk(probs, "PsdsAccumulator.update")
        t3, _ = _as_btk(target, "PsdsAccumulator.update")
        if p3.shape[0] != t3.shape[0] or p3.shape[2] != self.K or t3.shape[2] != self.K:
            raise ValueError(f"expected (B, T, {self.K}) and (B, Tt, {self.K}) (got {tuple(p3.shape)}, {tuple(t3.shape)})")
        p3 = p3.float().contiguous()
        t3 = t3.float().contiguous()
        B, T, Tt = p3.shape[0], p3.shape[1], t3.shape[1]
        n = min(T, Tt)
        lib = L.lib()
        if B > MAX_BATCH or n > lib.sed_psds_max_frames(self.K, len(self.thresholds)):
            raise ValueError(f"PSDS counts: at most {MAX_BATCH} recordings of at most "
                             f"{lib.sed_psds_max_frames(self.K, len(self.thresholds))} frames per call (got {B} x {n})")
        if B == 0 or n == 0:
            return
        if self.median_window != 1:
            p3 = median_filter_time(p3, self.median_window)
        s = self.scenario
        L.check(lib.sed_psds_counts(L.ptr(p3), L.ptr(t3), B, T, Tt, self.K, self._th, len(self.thresholds), s["dtc"][0], s["dtc"][1],
                                    s["gtc"][0], s["gtc"][1], s["cttc"][0], s["cttc"][1], L.ptr(self.counts), L.ptr(self.gt),
                                    _stream()), "psds_counts")
        self.total_frames += B * n

    def compute_raw(self):
        """(counts (nth, K, K + 3), gt (K, 2)) as int64 numpy arrays: ONE device-to-host copy"""
        import torch
        nth, K = len(self.thresholds), self.K
        host = torch.cat([self.counts.reshape(-1), self.gt.reshape(-1)]).cpu().numpy()
        a = nth * K * (K + 3)
        return host[:a].reshape(nth, K, K + 3).copy(), host[a:].reshape(K, 2).copy()

    def compute(self, fps):
        """psds_from_counts of everything counted so far, plus 'thresholds' and 'best_macro_f1_threshold'"""
        counts, gt = self.compute_raw()
        s = self.scenario
        res = psds_from_counts(counts, gt, self.total_frames, fps, s["alpha_ct"], s["alpha_st"], s["e_max"])
        res["thresholds"] = [float(t) for t in self.thresholds]
        i = res["best_macro_f1_index"]
        res["best_macro_f1_threshold"] = None if i is None else float(self.thresholds[i])
        return res


def psds_device(probs, target, fps, thresholds=None, scenario=1, median_window=1):
    """The PSDS dict of one (B, T, K) or (T, K) pair of CUDA tensors (PsdsAccumulator: one update, one compute)."""
    import torch
    if not (isinstance(probs, torch.Tensor) and probs.is_cuda):
        raise RuntimeError("psds_device needs CUDA tensors (there is no CPU path)")
    acc = PsdsAccumulator(probs.shape[-1], probs.device, thresholds=thresholds, scenario=scenario, median_window=median_window)
    acc.update(probs, target)
    return acc.compute(fps)
