"""Times of the device event decoding (csrc/sed_events.hip: median filter along time + hysteresis decoder) against the same work on
the host.

  python tools/events_time.py [--reps 50] [--warmup 5] [--window 51] [--out profiles/events_time.json]

Workloads: probabilities (B, T, K) = (32, 6000, 1) and (32, 6000, 14) -- sigmoid of a scaled random walk -- filtered over `window`
frames and decoded with (threshold, low_threshold, max_gap, min_len) = (0.5, 0.3, 5, 10).  Per workload:
  median_ms           sed_median_time alone, HIP events around `reps` launches after `warmup`
  decode_ms           sed_decode_events alone (counting pass, prefix sum, writing pass) on the filtered probabilities
  device_ms           utils.event_utils.decode_events: filter + decode with its allocations, events on the current stream
  device_call_ms      the same plus the event list's copy to the host (DecodedEvents.numpy()), host clock, best of 5
  host_ms             the same work without the kernels: the probabilities' device-to-host copy, scipy.ndimage.median_filter
                      (mode='reflect') and a numpy decoder (run boundaries by np.diff per row), host clock, best of 3
  events              the number of events; the two paths must give the same list (checked)
Needs the MI355X; prints one JSON object and writes it to --out."""
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
eu = importlib.import_module("soundeventdetection-pytorch_amd.utils.event_utils")
L = sed._lib
TH_HI, TH_LO, MAX_GAP, MIN_LEN = 0.5, 0.3, 5, 10


def events_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def best_wall_ms(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return best


def host_decode(p, th_hi, th_lo, max_gap, min_len):
    """numpy decoder: (n, 4) int32 rows (b, k, onset, offset) in (b, k, onset) order"""
    B, T, K = p.shape
    lo = np.zeros((B, K, T + 2), dtype=np.int8)
    lo[:, :, 1:-1] = np.transpose(p > np.float32(th_lo), (0, 2, 1))
    hi = np.transpose(p > np.float32(th_hi), (0, 2, 1))
    out = []
    for b in range(B):
        for k in range(K):
            d = np.diff(lo[b, k])
            on, off = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
            if not len(on):
                continue
            csum = np.concatenate(([0], np.cumsum(hi[b, k])))
            keep = csum[off] > csum[on]
            on, off = on[keep], off[keep]
            if not len(on):
                continue
            split = np.flatnonzero(on[1:] - off[:-1] > max_gap)
            s, e = on[np.concatenate(([0], split + 1))], off[np.concatenate((split, [len(off) - 1]))]
            long_enough = e - s >= min_len
            for s1, e1 in zip(s[long_enough], e[long_enough]):
                out.append((b, k, s1, e1))
    return np.asarray(out, dtype=np.int32).reshape(-1, 4)


def workload(B, T, K, window, reps, warmup):
    from scipy.ndimage import median_filter
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    walk = np.cumsum(rng.standard_normal((B, T, K)), axis=1) * 0.15
    walk -= walk.mean(axis=1, keepdims=True)
    p = torch.from_numpy((1.0 / (1.0 + np.exp(-walk))).astype(np.float32)).cuda()
    filt = torch.empty_like(p)
    cap = B * K * ((T + 1) // 2)
    events = torch.empty(cap, 4, dtype=torch.int32, device="cuda")
    counts = torch.empty(B * K, dtype=torch.int32, device="cuda")
    total = torch.empty(1, dtype=torch.int32, device="cuda")
    dec = torch.empty(B, T, K, dtype=torch.uint8, device="cuda")
    ws = torch.empty(lib.sed_decode_events_ws_bytes(B, T, K) // 4, dtype=torch.int32, device="cuda")

    def median():
        L.check(lib.sed_median_time(L.ptr(p), L.ptr(filt), B, T, K, window, st), "median_time")

    def decode():
        L.check(lib.sed_decode_events(L.ptr(filt), B, T, K, TH_HI, TH_LO, MAX_GAP, MIN_LEN, L.ptr(dec), L.ptr(events), cap,
                                      L.ptr(counts), L.ptr(total), L.ptr(ws), st), "decode_events")

    def device():
        return eu.decode_events(p, threshold=TH_HI, low_threshold=TH_LO, median_window=window, max_gap=MAX_GAP, min_len=MIN_LEN)

    def device_call():
        return device().numpy()

    def host():
        x = p.cpu().numpy()
        return host_decode(median_filter(x, size=(1, window, 1), mode="reflect"), TH_HI, TH_LO, MAX_GAP, MIN_LEN)

    median_ms = events_ms(median, reps, warmup)
    decode_ms = events_ms(decode, reps, warmup)
    device_ms = events_ms(device, reps, warmup)
    got = device_call()
    call_ms = best_wall_ms(device_call, 5)
    want = host()
    host_ms = best_wall_ms(host, 3)
    if not np.array_equal(got, want):
        raise SystemExit(f"({B}, {T}, {K}): the device and the host event lists differ")
    return {"B": B, "T": T, "K": K, "window": window, "threshold": TH_HI, "low_threshold": TH_LO, "max_gap": MAX_GAP,
            "min_len": MIN_LEN, "events": int(len(got)), "median_ms": median_ms, "decode_ms": decode_ms, "device_ms": device_ms,
            "device_call_ms": call_ms, "host_ms": host_ms, "host_over_device_call": host_ms / call_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=int, default=51)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/events_time.py measures on the MI355X: no GPU visible, nothing measured")
    rows = [workload(32, 6000, 1, a.window, a.reps, a.warmup), workload(32, 6000, 14, a.window, a.reps, a.warmup)]
    res = {"tool": "tools/events_time.py", "device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(),
           "host_threads": os.environ.get("OMP_NUM_THREADS"), "workloads": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
