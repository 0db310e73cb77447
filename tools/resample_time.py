"""Times of the device audio ingest (csrc/sed_resample.hip: PCM decode + downmix + polyphase resampler) against the host path.

  python tools/resample_time.py [--seconds 60] [--reps 200] [--warmup 20] [--out profiles/resample_time.json]

Workloads: `seconds` of 48 kHz int16 with 1 and with 4 channels -> 32 kHz mono, and 44.1 kHz int16 mono -> 48 kHz.  Per workload:
  launch_ms           sed_resample_poly alone, HIP events around `reps` launches after `warmup`, each launch on its own PCM / output
                      buffers out of a ring larger than the 256 MiB Infinity Cache, so the PCM comes from HBM (launch_hot_ms: one
                      buffer pair over and over, served from the caches)
  h2d_launch_ms       the pinned PCM's host-to-device copy plus the launch (events, same stream)
  ingest_call_ms      AudioIngest()(numpy PCM): pageable copy + launch + synchronise, host clock, best of 5
  host_ms             read_multichannel_audio(path, target_fs) without a device (float64, scipy.signal.resample_poly) on the same
                      samples written as a WAV file, host clock, best of 3 (includes the file read, as the callers' path does)
  bytes               what the launch must move: PCM in + float32 out; floor_ms = bytes / the box's HBM stream peak as bench.py --full
                      measures it (bench.measure_peaks: hbm_peak_measured_gbs); launch_over_floor = launch_ms / floor_ms
Needs the MI355X; prints one JSON object and writes it to --out."""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sed = importlib.import_module("soundeventdetection-pytorch_amd")
du = importlib.import_module("soundeventdetection-pytorch_amd.dataset.dataset_utils")
L = sed._lib
RING_BYTES = 600 << 20


def events_ms(fn, reps, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
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


def workload(name, src, dst, ch, seconds, reps, warmup, peak_gbs, tmp):
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    n_in = int(seconds * src)
    up, down = du.resample_ratio(src, dst)
    n_out = du.resampled_length(n_in, up, down)
    pcm = np.random.default_rng(0).integers(-20000, 20000, (n_in, ch), dtype=np.int16)
    nbytes = pcm.nbytes + 4 * n_out
    nring = max(2, -(-RING_BYTES // nbytes))
    taps = torch.from_numpy(du.resample_phases(up, down)).cuda()
    d_pcm = [torch.from_numpy(pcm).cuda() for _ in range(nring)]
    d_out = [torch.empty(1, n_out, dtype=torch.float32, device="cuda") for _ in range(nring)]

    def launch(i):
        k = i % nring
        L.check(lib.sed_resample_poly(L.PCM_I16, L.ptr(d_pcm[k]), L.ptr(taps), L.ptr(d_out[k]), 1, n_in, n_out, ch, 1, up, down, st),
                "resample_poly")

    launch_ms = events_ms(launch, reps, warmup)
    hot_ms = events_ms(lambda i: launch(0), reps, warmup)
    pinned = torch.from_numpy(pcm).pin_memory()

    def h2d_launch(i):
        d_pcm[i % nring].copy_(pinned, non_blocking=True)
        launch(i)

    h2d_ms = events_ms(h2d_launch, max(10, reps // 10), 3)
    ing = du.AudioIngest("cuda", 1)

    def ingest_call():
        ing(pcm, src, dst)
        torch.cuda.synchronize()

    ingest_call()
    call_ms = best_wall_ms(ingest_call, 5)
    from scipy.io import wavfile
    path = os.path.join(tmp, name + ".wav")
    wavfile.write(path, src, pcm)
    host_ms = best_wall_ms(lambda: du.read_multichannel_audio(path, target_fs=dst), 3)
    host = du.read_multichannel_audio(path, target_fs=dst)[:, 0]
    diff = float(np.abs(d_out[0][0].cpu().numpy().astype(np.float64) - host).max())
    floor_ms = nbytes / (peak_gbs * 1e9) * 1e3
    return {"name": name, "src_rate": src, "dst_rate": dst, "channels_in": ch, "seconds": seconds, "up": up, "down": down,
            "n_in": n_in, "n_out": n_out, "bytes": nbytes, "ring_buffers": nring, "launch_ms": launch_ms, "launch_hot_ms": hot_ms,
            "h2d_launch_ms": h2d_ms, "ingest_call_ms": call_ms, "host_ms": host_ms, "floor_ms": floor_ms,
            "launch_over_floor": launch_ms / floor_ms, "host_over_ingest_call": host_ms / call_ms,
            "max_abs_diff_vs_host": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/resample_time.py measures on the MI355X: no GPU visible, nothing measured")
    import bench
    peaks = bench.measure_peaks(sed, torch.device("cuda"))
    peak = peaks["hbm_peak_measured_gbs"]
    with tempfile.TemporaryDirectory() as tmp:
        rows = [workload("48k_mono_to_32k", 48000, 32000, 1, a.seconds, a.reps, a.warmup, peak, tmp),
                workload("48k_4ch_to_32k", 48000, 32000, 4, a.seconds, a.reps, a.warmup, peak, tmp),
                workload("44k1_mono_to_48k", 44100, 48000, 1, a.seconds, a.reps, a.warmup, peak, tmp)]
    res = {"tool": "tools/resample_time.py", "device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(),
           "host_threads": os.environ.get("OMP_NUM_THREADS"), "hbm_peak_measured_gbs": peak, "workloads": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
