"""Times of the device rank metrics (csrc/sed_rank.hip: pack, segmented radix sort, curve scan) against the same metric from
torch.sort + torch ops on the device and from numpy on the host.

  python tools/ranking_time.py [--batches 9] [--reps 5] [--warmup 2] [--out profiles/ranking_time.json]

Workloads: (n, K) = (600100, 14) and (600100, 1) -- 100 recordings of 6001 frames; scores are sigmoids of a class-dependent normal
(all but a few distinct), 5 % positives.  The variants are INTERLEAVED: each of `batches` rounds runs every variant `reps` times
between two device events (input copies that a variant needs but is not about are made outside its events); reported per variant:
the median over the rounds of the per-call time, and the spread (max - min) / median.
  pack_recording_ms   sed_rank_pack of one (6001, K) recording into the key buffer
  pack_all_ms         sed_rank_pack of all n rows in one call
  sort_ms             sed_rank_sort of the (K, n) keys (a fresh unsorted copy per call, copied outside the events)
  curve_ms            sed_rank_curve on the sorted keys
  together_ms         pack of all rows + sort + curve, back to back
  torch_ms            the same metric in torch: torch.sort(descending) per class row, gather of the labels, cumsum, tie-group ends by
                      comparison with the neighbour, AP / auc2 / best F1 by masked sums (float64 / int64), all on the device
  torch_sort_ms       torch.sort(descending) of the (K, n) fp32 scores alone, values and int64 indices: the sort inside torch_ms
  torch_sort_keys_ms  torch.sort of the (K, n) int32 keys, the closest torch has to a key-only sort (it still writes the indices)
  host_ms             the device-to-host copy of scores and targets plus numpy (key packing, np.sort per row, the same masked sums),
                      host clock, best of 3
  compute_call_ms     RankingAccumulator.compute_raw(): scratch copy + sort + curve + the small copy to the host, host clock
P and auc2 of the three paths must agree exactly and AP to 1e-12 (checked).  sort_bytes is the traffic model 4 passes x (histogram
read + scatter read + scatter write) x 4 B x K x n, sort_gbps that over sort_ms.  Needs the MI355X; prints one JSON object and writes
it to --out."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sed = importlib.import_module("soundeventdetection-pytorch_amd")
ru = importlib.import_module("soundeventdetection-pytorch_amd.utils.ranking_utils")
L = sed._lib
RECORDING, RECORDINGS = 6001, 100


def timed_ms(run, reps, prep=None):
    """per-call device time of run() over reps calls; prep() runs before every call, outside the events"""
    total = 0.0
    pairs = []
    for _ in range(reps):
        if prep is not None:
            prep()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    for e0, e1 in pairs:
        total += e0.elapsed_time(e1)
    return total / reps


def best_wall_ms(fn, reps):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return best


def torch_metric(st, yt):
    """st (K, n) fp32 scores, yt (K, n) bool labels on the device -> (P, auc2, AP, best F1) per class, device tensors"""
    ss, idx = torch.sort(st, dim=1, descending=True)
    tp = yt.gather(1, idx).to(torch.int64).cumsum(1)
    n = st.shape[1]
    npred = torch.arange(1, n + 1, device=st.device, dtype=torch.int64)[None]
    last = torch.ones_like(ss, dtype=torch.bool)
    last[:, :-1] = ss[:, :-1] != ss[:, 1:]
    P = tp[:, -1:]
    zero = torch.zeros_like(tp)
    tp_end = torch.where(last, tp, zero)
    fp_end = torch.where(last, npred - tp, zero)
    prev_tp = torch.zeros_like(tp)
    prev_fp = torch.zeros_like(tp)
    prev_tp[:, 1:] = torch.cummax(tp_end, dim=1)[0][:, :-1]
    prev_fp[:, 1:] = torch.cummax(fp_end, dim=1)[0][:, :-1]
    tpg, fpg = tp - prev_tp, (npred - tp) - prev_fp
    Pd = P.double()
    ap = torch.where(last, (tpg.double() / Pd) * (tp.double() / npred.double()), torch.zeros_like(Pd)).sum(1)
    auc2 = torch.where(last, fpg * (2 * prev_tp + tpg), zero).sum(1)
    f1 = torch.where(last, 2.0 * tp.double() / (npred + P).double(), torch.zeros_like(Pd)).max(1)[0]
    return P[:, 0], auc2, ap, f1


def numpy_metric(score, target):
    """score, target (n, K) host arrays -> (P, auc2, AP, best F1) per class"""
    keys = ((score.T.view(np.uint32).astype(np.uint32) << np.uint32(1)) | (target.T > 0.5)).astype(np.uint32)
    K, n = keys.shape
    P, auc2, ap, f1 = [], [], [], []
    npred = np.arange(1, n + 1, dtype=np.int64)
    for k in range(K):
        ks = np.sort(keys[k])[::-1]
        tp = np.cumsum(ks & np.uint32(1), dtype=np.int64)
        last = np.ones(n, dtype=bool)
        last[:-1] = (ks[:-1] >> np.uint32(1)) != (ks[1:] >> np.uint32(1))
        tpe, ne = tp[last], npred[last]
        ptp = np.concatenate(([0], tpe[:-1]))
        pfp = np.concatenate(([0], (ne - tpe)[:-1]))
        tpg, fpg = tpe - ptp, (ne - tpe) - pfp
        Pk = int(tp[-1])
        P.append(Pk)
        auc2.append(int(np.sum(fpg * (2 * ptp + tpg))))
        ap.append(float(np.sum((tpg / Pk) * (tpe / ne))) if Pk else float("nan"))
        f1.append(float(np.max(2.0 * tpe / (ne + Pk))))
    return np.array(P), np.array(auc2), np.array(ap), np.array(f1)


def workload(n, K, batches, reps, warmup):
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(K)
    target = (rng.uniform(size=(n, K)) < 0.05).astype(np.float32)
    logit = rng.standard_normal((n, K)) * 1.5 - 2.0 + 2.5 * target
    score = (1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
    s, t = torch.from_numpy(score).cuda(), torch.from_numpy(target).cuda()
    keys = torch.empty(K, n, dtype=torch.int32, device="cuda")
    work = torch.empty_like(keys)
    invalid = torch.zeros(K, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.sed_rank_ws_bytes(K, n), dtype=torch.uint8, device="cuda")
    ap = torch.empty(K, dtype=torch.float64, device="cuda")
    counts = torch.empty(K, 6, dtype=torch.int64, device="cuda")
    best = torch.empty(K, dtype=torch.float32, device="cuda")
    s_rec, t_rec = s[:RECORDING].contiguous(), t[:RECORDING].contiguous()
    s_t, y_t = s.t().contiguous(), (t.t() > 0.5).contiguous()

    def pack_recording():
        L.check(lib.sed_rank_pack(L.ptr(s_rec), L.ptr(t_rec), RECORDING, RECORDING, K, L.ptr(work), n, 0, L.ptr(invalid), st), "pack")

    def pack_all(dst=keys):
        L.check(lib.sed_rank_pack(L.ptr(s), L.ptr(t), n, n, K, L.ptr(dst), n, 0, L.ptr(invalid), st), "pack")

    def fresh():
        work.copy_(keys)

    def sort():
        L.check(lib.sed_rank_sort(L.ptr(work), K, n, n, L.ptr(ws), st), "sort")

    def curve():
        L.check(lib.sed_rank_curve(L.ptr(work), K, n, n, L.ptr(ap), L.ptr(counts), L.ptr(best), L.ptr(ws), st), "curve")

    def together():
        pack_all(work)
        sort()
        curve()

    def torch_path():
        return torch_metric(s_t, y_t)

    def torch_sort():
        return torch.sort(s_t, dim=1, descending=True)

    def torch_sort_keys():
        return torch.sort(keys, dim=1)

    def host_path():
        return numpy_metric(s.cpu().numpy(), t.cpu().numpy())

    pack_all()
    acc = ru.RankingAccumulator(K, "cuda", capacity=n)
    acc.update(s, t)
    # the three paths agree
    fresh(); sort(); curve()
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    tP, tauc, tap, tf1 = (x.cpu().numpy() for x in torch_path())
    hP, hauc, hap, hf1 = host_path()
    f1_dev = 2.0 * c[:, 3] / (c[:, 4] + c[:, 0])
    if not (np.array_equal(c[:, 0], tP) and np.array_equal(c[:, 0], hP) and np.array_equal(c[:, 2], tauc) and np.array_equal(c[:, 2], hauc)):
        raise SystemExit(f"({n}, {K}): P / auc2 of the three paths differ")
    if not (np.allclose(ap.cpu().numpy(), tap, rtol=1e-12, atol=0) and np.allclose(ap.cpu().numpy(), hap, rtol=1e-12, atol=0)
            and np.allclose(f1_dev, tf1, rtol=1e-12) and np.allclose(f1_dev, hf1, rtol=1e-12)):
        raise SystemExit(f"({n}, {K}): AP / best F1 of the three paths differ")

    variants = {"pack_recording": (pack_recording, None), "pack_all": (pack_all, None), "sort": (sort, fresh), "curve": (curve, None),
                "together": (together, None), "torch": (torch_path, None), "torch_sort": (torch_sort, None),
                "torch_sort_keys": (torch_sort_keys, None)}
    for _ in range(warmup):
        for run, prep in variants.values():
            timed_ms(run, 1, prep)
    fresh(); sort()                                   # curve() times on sorted keys: every round leaves `work` sorted before it
    rounds = {name: [] for name in variants}
    for _ in range(batches):
        for name, (run, prep) in variants.items():
            if name == "curve":
                fresh(); sort()
            rounds[name].append(timed_ms(run, reps, prep))
    row = {"n": n, "K": K, "batches": batches, "reps": reps}
    for name, ms in rounds.items():
        med = float(np.median(ms))
        row[name + "_ms"] = med
        row[name + "_spread"] = float((max(ms) - min(ms)) / med)
    row["compute_call_ms"] = best_wall_ms(acc.compute_raw, 3)
    row["host_ms"] = best_wall_ms(host_path, 3)
    row["d2h_ms"] = best_wall_ms(lambda: (s.cpu(), t.cpu()), 3)
    row["sort_bytes"] = 4 * 3 * 4 * K * n
    row["sort_gbps"] = row["sort_bytes"] / (row["sort_ms"] * 1e-3) / 1e9
    row["torch_sort_over_sort"] = row["torch_sort_ms"] / row["sort_ms"]
    row["torch_sort_keys_over_sort"] = row["torch_sort_keys_ms"] / row["sort_ms"]
    row["torch_over_together"] = row["torch_ms"] / row["together_ms"]
    row["host_over_compute_call"] = row["host_ms"] / row["compute_call_ms"]
    row["mAP"] = float(np.mean(ap.cpu().numpy()))
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", type=int, default=9)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranking_time.json"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ranking_time.py measures on the MI355X: no GPU visible, nothing measured")
    n = RECORDING * RECORDINGS
    rows = [workload(n, 14, a.batches, a.reps, a.warmup), workload(n, 1, a.batches, a.reps, a.warmup)]
    res = {"tool": "tools/ranking_time.py", "device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(),
           "host_threads": os.environ.get("OMP_NUM_THREADS"), "workloads": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
