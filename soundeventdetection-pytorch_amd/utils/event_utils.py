"""Event decoding on the MI355X (csrc/sed_events.hip): median filter along time, double-threshold (hysteresis) decisions with gap
merging and a minimum length, the (class, onset, offset) event list, and segment-based / event-based (collar) scores.

The reference stops at per-frame probabilities (train.py:43, infer.py); this is the post-processing every DCASE baseline adds.  The
device functions take CUDA tensors laid out (B, T, K) or (T, K) -- the models' output layout -- and raise on CPU tensors: there is no
CPU path.  Only event_based_metrics runs on the host, on event lists (a few rows per recording)."""
from __future__ import annotations

import math

import numpy as np

MAX_MEDIAN_WINDOW = 511


def seconds_to_frames(seconds, fps):
    """A duration in seconds as a whole number of frames (nearest, never negative)."""
    return max(0, int(round(float(seconds) * float(fps))))


def seconds_to_window(seconds, fps):
    """A median-filter length in seconds as the nearest odd frame count >= 1 (0 s -> 1 = no filter)."""
    x = float(seconds) * float(fps)
    return max(1, 2 * int(math.floor(x / 2.0)) + 1) if x > 0 else 1


def _as_btk(x, what):
    import torch
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"{what} needs a CUDA tensor (there is no CPU path)")
    if x.dim() not in (2, 3):
        raise ValueError(f"{what}: expected (B, T, K) or (T, K), got {tuple(x.shape)}")
    y = x.detach()
    return (y[None] if y.dim() == 2 else y), x.dim() == 2


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def median_filter_time(x, win):
    """scipy.ndimage.median_filter(x, size=(1, win, 1), mode='reflect') for a CUDA (B, T, K) or (T, K) tensor: the median over
    `win` (odd, 1..511) frames along time, half-sample-symmetric reflection at both ends.  Returns a new fp32 tensor of the same
    shape; every element is one of the input's values."""
    import torch
    from .. import _lib as L
    x3, squeeze = _as_btk(x, "median_filter_time")
    win = int(win)
    if win < 1 or win > MAX_MEDIAN_WINDOW or win % 2 == 0:
        raise ValueError(f"median window must be odd, 1..{MAX_MEDIAN_WINDOW} frames (got {win})")
    x3 = x3.float().contiguous()
    B, T, K = x3.shape
    out = torch.empty_like(x3)
    L.check(L.lib().sed_median_time(L.ptr(x3), L.ptr(out), B, T, K, win, _stream()), "median_time")
    return out[0] if squeeze else out


class DecodedEvents:
    """What decode_events returns; everything stays on the device until numpy() / seconds() is called.
    events (capacity, 4) int32 rows (b, k, onset, offset), offset exclusive, ascending (b, k, onset), the first `total` valid;
    row_counts (B*K,) int32; total (1,) int32; decisions (B, T, K) or (T, K) uint8."""

    def __init__(self, events, row_counts, total, decisions, probs):
        self.events, self.row_counts, self.total, self.decisions, self.probs = events, row_counts, total, decisions, probs

    def numpy(self):
        """The (n, 4) int32 host array of (b, k, onset, offset) (events_to_host)."""
        return events_to_host(self)[0]

    def seconds(self, fps, b=0):
        """(n, 3) float64 rows (class, onset_s, offset_s) of recording b."""
        ev = self.numpy()
        ev = ev[ev[:, 0] == b]
        return np.stack([ev[:, 1].astype(np.float64), ev[:, 2] / float(fps), ev[:, 3] / float(fps)], axis=1).reshape(-1, 3)


SINGLE_COPY_ROWS = 65536


def events_to_host(*decoded):
    """The (n, 4) int32 host arrays of one or more DecodedEvents.  Buffers of up to SINGLE_COPY_ROWS rows in all (any single
    recording) come over in ONE device-to-host copy together with their counts; larger ones after one small copy of the counts."""
    import torch
    totals = torch.cat([d.total.reshape(1) for d in decoded])
    if sum(d.events.shape[0] for d in decoded) <= SINGLE_COPY_ROWS:
        host = torch.cat([totals.reshape(-1, 1).expand(-1, 4)] + [d.events for d in decoded]).cpu().numpy()
        out, pos = [], len(decoded)
        for i, d in enumerate(decoded):
            out.append(host[pos:pos + int(host[i, 0])].copy())
            pos += d.events.shape[0]
        return out
    return [d.events[:int(n)].cpu().numpy() for d, n in zip(decoded, totals.cpu().tolist())]


def decode_events(probs, threshold=0.5, low_threshold=None, median_window=1, max_gap=0, min_len=1):
    """probs: CUDA (B, T, K) or (T, K) frame probabilities.  median_window > 1 filters them first (median_filter_time).  A run of
    frames with p > low_threshold is an event candidate if one of its frames has p > threshold (low_threshold=None: the same
    value, plain thresholding); candidates at most max_gap frames apart merge; merged events shorter than min_len frames are
    dropped.  Comparisons are strict and in fp32.  Returns a DecodedEvents; no host synchronisation happens here (the event buffer
    is sized for the worst case, B*K*ceil(T/2) rows)."""
    import torch
    from .. import _lib as L
    p3, squeeze = _as_btk(probs, "decode_events")
    th_hi = float(threshold)
    th_lo = th_hi if low_threshold is None else float(low_threshold)
    if not th_lo <= th_hi:
        raise ValueError(f"low_threshold {th_lo} must not exceed threshold {th_hi}")
    max_gap, min_len, median_window = int(max_gap), int(min_len), int(median_window)
    if max_gap < 0 or min_len < 1:
        raise ValueError(f"max_gap must be >= 0 and min_len >= 1 (got {max_gap}, {min_len})")
    p3 = p3.float().contiguous()
    if median_window != 1:
        p3 = median_filter_time(p3, median_window)
    B, T, K = p3.shape
    lib = L.lib()
    ws_bytes = lib.sed_decode_events_ws_bytes(B, T, K)
    if ws_bytes == 0:
        raise ValueError(f"decode_events: shape {(B, T, K)} is out of range (B*K*ceil(T/2) must stay below 2^31)")
    dev = p3.device
    cap = B * K * ((T + 1) // 2)
    events = torch.empty(cap, 4, dtype=torch.int32, device=dev)
    row_counts = torch.empty(B * K, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    decisions = torch.empty(B, T, K, dtype=torch.uint8, device=dev)
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    L.check(lib.sed_decode_events(L.ptr(p3), B, T, K, th_hi, th_lo, max_gap, min_len, L.ptr(decisions), L.ptr(events), cap,
                                  L.ptr(row_counts), L.ptr(total), L.ptr(ws), _stream()), "decode_events")
    return DecodedEvents(events, row_counts, total, decisions[0] if squeeze else decisions, p3[0] if squeeze else p3)


def events_from_targets(target):
    """Reference events of a 0/1 event matrix (CUDA (B, T, K) or (T, K)): the runs of target > 0.5 -- the same decoder at 0.5."""
    return decode_events(target, threshold=0.5)


def prf_counts(tp, fp, fn):
    """(precision, recall, F1) from counts, with metric_utils' conventions: recall 1 without reference, precision 1 without
    predictions."""
    tp, fp, fn = float(tp), float(fp), float(fn)
    prec = tp / (tp + fp) if tp + fp > 0 else 1.0
    rec = tp / (tp + fn) if tp + fn > 0 else 1.0
    return prec, rec, (2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0)


def segment_counts_device(decisions, target, seg_frames):
    """(K, 3) int64 device tensor of segment-based (TP, FP, FN): decisions uint8 and target fp32, CUDA (B, T, K) / (B, Tt, K) (or
    without B); the first min(T, Tt) frames are cut into segments of seg_frames frames (the last may be shorter)."""
    import torch
    from .. import _lib as L
    d3, _ = _as_btk(decisions, "segment_counts_device")
    t3, _ = _as_btk(target, "segment_counts_device")
    if d3.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"decisions must be uint8 or bool (got {d3.dtype})")
    d3 = d3.to(torch.uint8).contiguous()
    t3 = t3.float().contiguous()
    if d3.shape[0] != t3.shape[0] or d3.shape[2] != t3.shape[2]:
        raise ValueError(f"decisions {tuple(d3.shape)} and target {tuple(t3.shape)} differ in batch or classes")
    if int(seg_frames) < 1:
        raise ValueError(f"seg_frames must be >= 1 (got {seg_frames})")
    B, T, K = d3.shape
    counts = torch.empty(K, 3, dtype=torch.int64, device=d3.device)
    L.check(L.lib().sed_segment_counts(L.ptr(d3), L.ptr(t3), B, T, t3.shape[1], K, int(seg_frames), L.ptr(counts), _stream()),
            "segment_counts")
    return counts


def metrics_from_segment_counts(counts):
    """counts (K, 3) host integers (TP, FP, FN) -> {'per_class': [{precision, recall, f1, error_rate}], 'micro': {...}, 'counts'}.
    error_rate = (S + D + I) / N with S = min(FP, FN), D = FN - S, I = FP - S, N = TP + FN, i.e. max(FP, FN) / N, taken per class
    over the summed counts (0 when there is no reference and no false alarm; FP when there is no reference)."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 3)

    def one(tp, fp, fn):
        p, r, f = prf_counts(tp, fp, fn)
        n = tp + fn
        return {"precision": p, "recall": r, "f1": f, "error_rate": float(max(fp, fn)) / float(n) if n > 0 else float(fp)}

    tot = counts.sum(axis=0)
    return {"per_class": [one(*(int(v) for v in row)) for row in counts], "micro": one(*(int(v) for v in tot)),
            "counts": counts}


def segment_metrics_device(decisions, target, seg_frames):
    """Segment-based precision / recall / F1 / error rate, per class and micro-averaged: counting on the device
    (sed_segment_counts), 3K integers to the host."""
    return metrics_from_segment_counts(segment_counts_device(decisions, target, seg_frames).cpu().numpy())


def event_match_counts(pred, ref, collar_frames, offset_pct=0.5):
    """Host, numpy.  pred / ref: (n, 3) rows (class, onset, offset) in frames, or (n, 4) rows (b, class, onset, offset) -- events of
    different recordings never match.  A predicted and a reference event of one class are compatible when
    |onset_p - onset_r| <= collar_frames and |offset_p - offset_r| <= max(collar_frames, ceil(offset_pct * len_r)); TP is the size
    of a MAXIMUM matching of the compatibility graph (scipy.sparse.csgraph.maximum_bipartite_matching), not of a greedy one.
    Returns {class: (TP, FP, FN)} for every class that occurs."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching

    def rows(e):
        e = np.asarray(e, dtype=np.int64)
        if e.size == 0:
            return np.zeros((0, 4), dtype=np.int64)
        e = e.reshape(-1, e.shape[-1])
        if e.shape[1] == 3:
            e = np.concatenate([np.zeros((len(e), 1), dtype=np.int64), e], axis=1)
        if e.shape[1] != 4:
            raise ValueError("events must be (n, 3) = (class, onset, offset) or (n, 4) = (b, class, onset, offset)")
        return e

    P, R = rows(pred), rows(ref)
    out = {}
    for k in sorted(set(P[:, 1].tolist()) | set(R[:, 1].tolist())):
        p, r = P[P[:, 1] == k], R[R[:, 1] == k]
        tp = 0
        if len(p) and len(r):
            tol = np.maximum(int(collar_frames), np.ceil(float(offset_pct) * (r[:, 3] - r[:, 2])).astype(np.int64))
            ok = ((p[:, None, 0] == r[None, :, 0]) & (np.abs(p[:, None, 2] - r[None, :, 2]) <= int(collar_frames)) &
                  (np.abs(p[:, None, 3] - r[None, :, 3]) <= tol[None, :]))
            if ok.any():
                match = maximum_bipartite_matching(csr_matrix(ok.astype(np.int8)), perm_type="column")
                tp = int(np.count_nonzero(match >= 0))
        out[int(k)] = (tp, len(p) - tp, len(r) - tp)
    return out


def event_based_metrics(pred, ref, collar_frames, offset_pct=0.5):
    """Event-based (collar) precision / recall / F1 per class and micro-averaged from event_match_counts:
    {'per_class': {class: {precision, recall, f1, tp, fp, fn}}, 'micro': {...}}."""
    counts = event_match_counts(pred, ref, collar_frames, offset_pct)

    def one(tp, fp, fn):
        p, r, f = prf_counts(tp, fp, fn)
        return {"precision": p, "recall": r, "f1": f, "tp": int(tp), "fp": int(fp), "fn": int(fn)}

    tot = np.sum([list(v) for v in counts.values()], axis=0) if counts else (0, 0, 0)
    return {"per_class": {k: one(*v) for k, v in counts.items()}, "micro": one(*(int(v) for v in tot))}
