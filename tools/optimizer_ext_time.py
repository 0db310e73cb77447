"""HIP-event times of the train step with the optimizer options off and on (sed_grad_norm, sed_adam_step_ex; FusedTrainer's
weight_decay / decoupled_weight_decay / max_grad_norm).

  python tools/optimizer_ext_time.py [--steps K] [--warmup W] [--rounds R] [--out profiles/optimizer_ext_time.json]

Two workloads -- the bench shape (Cnn_AvgPooling main widths, bf16, B = 32, T = 6001, F = 64) and Crnn_AvgPooling at B = 16, same
T -- each in three configurations: options off (the reference step: sed_adam_amsgrad_step), clipping on, clipping plus decoupled
weight decay.  The three trainers of a workload live side by side and are timed in interleaved rounds (off, clip, clip+decay, off,
...), so drift of the machine hits all of them alike; the per-configuration figure is the median over the rounds, with the
spread (max - min) beside it.  The optimizer part alone (optimizer_step() on the gradients of the last backward: one launch
off, three on) is timed the same way: the whole-step deltas are a few microseconds on a step of milliseconds and sit inside
its spread, the isolated numbers are the ones to read.  Prints one JSON object and writes it to --out."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sed = importlib.import_module("soundeventdetection-pytorch_amd")
MAIN_CFG = [(32, 2), (64, 2), (128, 2), (128, 1)]
CONFIGS = {"off": {}, "clip": {"max_grad_norm": 1.0},
           "clip_decoupled_decay": {"max_grad_norm": 1.0, "weight_decay": 1e-2, "decoupled_weight_decay": True}}


def time_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def workload(make, B, T, steps, warmup, rounds):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, 1, T, 64, device="cuda", generator=g)
    y = (torch.rand(B, T, 1, device="cuda", generator=g) < 0.2).float()
    trainers = {}
    for name, kw in CONFIGS.items():
        torch.manual_seed(0)
        trainers[name] = sed.FusedTrainer(make().cuda(), lr=1e-4, recall_factor=5.0, **kw)
    for tr in trainers.values():
        for _ in range(warmup):
            tr.train_step(x, y)
    torch.cuda.synchronize()
    step = {k: [] for k in trainers}
    opt = {k: [] for k in trainers}
    for _ in range(rounds):
        for name, tr in trainers.items():
            step[name].append(time_ms(lambda: tr.train_step(x, y), steps))
        for name, tr in trainers.items():
            opt[name].append(time_ms(tr.optimizer_step, 20 * steps))

    def stat(v):
        return {"median_ms": round(statistics.median(v), 5), "spread_ms": round(max(v) - min(v), 5)}

    out = {"shape": [B, 1, T, 64], "flat_parameters": trainers["off"].flat.numel,
           "train_step": {k: stat(v) for k, v in step.items()}, "optimizer_step_alone": {k: stat(v) for k, v in opt.items()}}
    for k in ("clip", "clip_decoupled_decay"):
        out["optimizer_step_alone"][k]["delta_vs_off_ms"] = round(
            out["optimizer_step_alone"][k]["median_ms"] - out["optimizer_step_alone"]["off"]["median_ms"], 5)
        out["train_step"][k]["delta_vs_off_ms"] = round(out["train_step"][k]["median_ms"] - out["train_step"]["off"]["median_ms"], 5)
    del trainers
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=6001)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_ext_time.json"))
    a = ap.parse_args()
    res = {"steps": a.steps, "rounds": a.rounds,
           "cnn_bf16_B32": workload(lambda: sed.Cnn_AvgPooling(1, MAIN_CFG, precision="bf16"), 32, a.frames, a.steps, a.warmup, a.rounds),
           "crnn_bf16_B16": workload(lambda: sed.Crnn_AvgPooling(1, MAIN_CFG, precision="bf16"), 16, a.frames, a.steps, a.warmup,
                                     a.rounds)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
