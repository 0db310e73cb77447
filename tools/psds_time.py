"""Times of the PSDS threshold sweep on the device (csrc/sed_psds.hip: one sed_psds_counts per batch of recordings) against the path
that existed before it -- one decode_events per operating point, the event lists copied to the host, the intersections there -- and
against the numpy formula of tests/psds_formula.py alone.

  python tools/psds_time.py [--batches 7] [--reps 3] [--warmup 2] [--host_recordings 4] [--out profiles/psds_time.json]

Workloads: 100 recordings of 6001 frames, K = 14 and K = 1, 50 thresholds (0.01 .. 0.99), criteria of scenarios 1 and 2.  The
probabilities are sigmoids of low-pass-filtered noise plus the class's target and some of the next class's; the targets are random
runs (35 % active, mean length 40 frames).  The device variants are INTERLEAVED: each of `batches` rounds runs every variant `reps`
times between two device events; reported per variant: the median over the rounds of the per-call time and the spread
(max - min) / median.
  counts_s1_ms, counts_s2_ms   sed_psds_counts over all recordings, criteria of scenario 1 / 2
  decode50_ms                  the device part of the old path: 50 x utils.event_utils.decode_events (plain thresholding) + one for
                               the targets, as the package calls them (their buffers are allocated per call, as there)
  accumulator_call_ms          PsdsAccumulator: update + compute_raw (the copy of the counts to the host), host clock, best of 3
  old_device_and_copy_ms       the 51 decode_events + events_to_host of the 51 event lists, host clock, best of 2, all recordings
  old_host_intersect_ms        the intersections of those event lists on the host (plain loops that count frames, as the formula),
                               measured on the first `host_recordings` recordings and scaled by 100 / host_recordings (recordings are
                               independent, the loop is linear in them); per scenario
  old_path_ms                  old_device_and_copy_ms + old_host_intersect_ms
  formula_ms                   tests/psds_formula.psds_counts on the host arrays, measured and scaled the same way; per scenario
The counts of the three paths must agree exactly on the recordings the host paths ran (checked), and the new call's counts over
all recordings must equal the sum of its counts per recording (checked).  hbm_bytes = the two input tensors read once; l2_bytes =
what the workgroups pull in all: every (b, k) workgroup reads its recording's whole target array and as many lines again for its
prob column; decisions = nth x B x K x T frame comparisons.  Needs the MI355X; prints one JSON object and writes it to --out."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sed = importlib.import_module("soundeventdetection-pytorch_amd")
pu = importlib.import_module("soundeventdetection-pytorch_amd.utils.psds_utils")
eu = importlib.import_module("soundeventdetection-pytorch_amd.utils.event_utils")
from psds_formula import psds_counts          # noqa: E402

L = sed._lib
RECORDING, RECORDINGS, NTH = 6001, 100, 50
HBM_BYTES_PER_S = 6.3e12              # the achievable rate (MI355X float4 copy)


def timed_ms(run, reps):
    """per-call device time of run() over reps calls"""
    pairs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    return sum(e0.elapsed_time(e1) for e0, e1 in pairs) / reps


def best_wall_ms(fn, reps):
    best, out = None, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return best, out


def make_inputs(B, T, K, seed):
    rng = np.random.default_rng(seed)
    target = np.zeros((B, T, K), dtype=np.float32)
    for b in range(B):
        for k in range(K):
            pos = int(rng.geometric(1.0 / 74.0)) - 1
            while pos < T:
                on = int(rng.geometric(1.0 / 40.0))
                target[b, pos:pos + on, k] = 1.0
                pos += on + int(rng.geometric(1.0 / 74.0))
    win = 9
    noise = rng.standard_normal((B, T + win - 1, K))
    csum = np.concatenate([np.zeros((B, 1, K)), np.cumsum(noise, axis=1)], axis=1)
    smooth = (csum[:, win:] - csum[:, :-win]) / np.sqrt(win)
    logits = 1.3 * smooth + 2.2 * (target - 0.5) + 1.6 * np.roll(target, -1, axis=2) * (K > 1) - 0.4
    return (1.0 / (1.0 + np.exp(-logits))).astype(np.float32), target


def counts_from_events(pred_lists, ref, B, K, n, crit):
    """the old path's host step: pred_lists[i] / ref = (m, 4) int rows (b, k, onset, offset) ascending -> counts, gt as the formula"""
    dtc, gtc, cttc = crit
    tgt = np.zeros((B, n, K), dtype=bool)
    gt = np.zeros((K, 2), dtype=np.int64)
    ref_of = {}
    for b, k, a, e in ref.tolist():
        tgt[b, a:e, k] = True
        gt[k, 0] += 1
        gt[k, 1] += e - a
        ref_of.setdefault((b, k), []).append((a, e))
    counts = np.zeros((len(pred_lists), K, K + 3), dtype=np.int64)
    for i, pred in enumerate(pred_lists):
        covered = np.zeros((B, n, K), dtype=bool)
        for b, k, a, e in pred.tolist():
            length = e - a
            counts[i, k, 2] += 1
            per_class = np.count_nonzero(tgt[b, a:e], axis=0)
            if int(per_class[k]) * dtc[1] >= dtc[0] * length:
                covered[b, a:e, k] = True
            else:
                counts[i, k, 1] += 1
                for c in range(K):
                    if c != k and int(per_class[c]) * cttc[1] >= cttc[0] * length:
                        counts[i, k, 3 + c] += 1
        for (b, k), events in ref_of.items():
            for a, e in events:
                if int(np.count_nonzero(covered[b, a:e, k])) * gtc[1] >= gtc[0] * (e - a):
                    counts[i, k, 0] += 1
    return counts, gt


def workload(K, batches, reps, warmup, host_recordings):
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    B, T, R = RECORDINGS, RECORDING, host_recordings
    prob, target = make_inputs(B, T, K, seed=K)
    p, t = torch.from_numpy(prob).cuda(), torch.from_numpy(target).cuda()
    th = pu.check_thresholds(None)
    crits = {s: tuple(pu.SCENARIOS[s][c] for c in ("dtc", "gtc", "cttc")) for s in (1, 2)}
    accs = {s: pu.PsdsAccumulator(K, "cuda", scenario=s) for s in (1, 2)}

    def counts_call(s, pp=p, tt=t):
        accs[s].update(pp, tt)

    def decode_all(pp=p, tt=t):
        return [eu.decode_events(pp, threshold=float(v)) for v in th], eu.events_from_targets(tt)

    def old_device_and_copy(pp=p, tt=t):
        preds, ref = decode_all(pp, tt)
        lists = eu.events_to_host(*preds, ref)
        return lists[:-1], lists[-1]

    def accumulator_call():
        a = accs[1]
        a.reset()
        a.update(p, t)
        return a.compute_raw()

    print(f"K={K}: inputs ready", flush=True)
    # the three paths agree on the first R recordings; the whole batch equals the sum over single recordings
    row = {"B": B, "T": T, "K": K, "nth": NTH, "batches": batches, "reps": reps, "host_recordings": R}
    sub_pred, sub_ref = old_device_and_copy(p[:R].contiguous(), t[:R].contiguous())
    for s in (1, 2):
        accs[s].reset()
        counts_call(s, p[:R].contiguous(), t[:R].contiguous())
        dev_counts, dev_gt = accs[s].compute_raw()
        t0 = time.perf_counter()
        f_counts, f_gt = psds_counts(prob[:R], target[:R], th, *crits[s])
        row[f"formula_s{s}_ms"] = (time.perf_counter() - t0) * 1e3 * B / R
        t0 = time.perf_counter()
        o_counts, o_gt = counts_from_events(sub_pred, sub_ref, R, K, T, crits[s])
        row[f"old_host_intersect_s{s}_ms"] = (time.perf_counter() - t0) * 1e3 * B / R
        if not (np.array_equal(dev_counts, f_counts) and np.array_equal(dev_gt, f_gt) and np.array_equal(o_counts, f_counts)
                and np.array_equal(o_gt, f_gt)):
            raise SystemExit(f"K={K}, scenario {s}: the counts of the three paths differ")
        print(f"K={K}: scenario {s} agrees on {R} recordings", flush=True)
        accs[s].reset()
        for b in range(B):
            counts_call(s, p[b:b + 1], t[b:b + 1])
        one_by_one = accs[s].compute_raw()
        accs[s].reset()
        counts_call(s)
        whole = accs[s].compute_raw()
        if not (np.array_equal(one_by_one[0], whole[0]) and np.array_equal(one_by_one[1], whole[1])):
            raise SystemExit(f"K={K}, scenario {s}: the whole batch differs from the sum over its recordings")
        row[f"detections_s{s}"] = int(whole[0][:, :, 2].sum())
        row[f"true_positives_s{s}"] = int(whole[0][:, :, 0].sum())
        row[f"cross_triggers_s{s}"] = int(whole[0][:, :, 3:].sum())
    row["ground_truth_events"] = int(whole[1][:, 0].sum())

    variants = {"counts_s1": lambda: counts_call(1), "counts_s2": lambda: counts_call(2), "decode50": decode_all}
    for _ in range(warmup):
        for run in variants.values():
            timed_ms(run, 1)
    rounds = {name: [] for name in variants}
    for _ in range(batches):
        for name, run in variants.items():
            rounds[name].append(timed_ms(run, reps))
    for name, ms in rounds.items():
        med = float(np.median(ms))
        row[name + "_ms"] = med
        row[name + "_spread"] = float((max(ms) - min(ms)) / med)
    print(f"K={K}: device variants timed", flush=True)
    row["accumulator_call_ms"] = best_wall_ms(accumulator_call, 3)[0]
    row["old_device_and_copy_ms"] = best_wall_ms(old_device_and_copy, 2)[0]
    for s in (1, 2):
        row[f"old_path_s{s}_ms"] = row["old_device_and_copy_ms"] + row[f"old_host_intersect_s{s}_ms"]
        row[f"old_path_over_accumulator_call_s{s}"] = row[f"old_path_s{s}_ms"] / row["accumulator_call_ms"]
        row[f"formula_over_accumulator_call_s{s}"] = row[f"formula_s{s}_ms"] / row["accumulator_call_ms"]
        row[f"decode50_over_counts_s{s}"] = row["decode50_ms"] / row[f"counts_s{s}_ms"]
    row["hbm_bytes"] = 2 * B * T * K * 4
    row["l2_bytes"] = B * K * 2 * T * K * 4
    row["decisions"] = NTH * B * K * T
    row["hbm_floor_ms"] = row["hbm_bytes"] / HBM_BYTES_PER_S * 1e3
    row["counts_s1_over_hbm_floor"] = row["counts_s1_ms"] / row["hbm_floor_ms"]
    row["l2_gbps_s1"] = row["l2_bytes"] / (row["counts_s1_ms"] * 1e-3) / 1e9
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", type=int, default=7)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--host_recordings", type=int, default=4)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "psds_time.json"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/psds_time.py measures on the MI355X: no GPU visible, nothing measured")
    rows = [workload(14, a.batches, a.reps, a.warmup, a.host_recordings), workload(1, a.batches, a.reps, a.warmup, a.host_recordings)]
    res = {"tool": "tools/psds_time.py", "device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(),
           "host_threads": os.environ.get("OMP_NUM_THREADS"), "workloads": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
