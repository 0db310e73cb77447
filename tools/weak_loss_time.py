"""Times of the weak-label loss call (csrc/sed_weak.hip) against the strong loss call it stands beside, and of the whole bench-shape
train step with the weak loss off, added, and alone.

  python tools/weak_loss_time.py [--reps 30] [--warmup 3] [--out profiles/weak_loss_time.json]

Loss calls: pre (B, t, K) = (32, 750, 1) and (32, 750, 14) with ratio = 8 and Tt = 6001 strong-label frames, the shapes of the
bench step's loss at 1 and 14 classes.  Interleaved (every repeat runs each variant once, `inner` calls between two device events,
after `warmup` untimed repeats), median / min / max over the repeats of the time per call:
  strong           sed_bce_fwd_bwd (two launches): the yardstick
  weak_<mode>      sed_weak_bce_fwd_bwd (two launches) on the same logits and the same strong target, of which it takes the clip
                   label itself, for max / mean / linear / exp
  weak_clip_linear the same with (B, K) clip labels: no target tensor to scan
  pool_linear      sed_clip_pool_fwd (one launch): the clip probabilities only
Both loss calls read the B*t*K logits once or twice and B*Tt*K target values once; at these sizes (24 k and 336 k logits) that is
microseconds of traffic and the calls are expected to be bound by their two launches.
Train step: Cnn_AvgPooling, bf16, B = 32, T = 6001 frames of 64 mel bins, one class (bench.py's shape, features only), eager
FusedTrainer.train_step with --weak_labels off / both / only (linear pooling), interleaved the same way, `inner` = 1.
Needs the MI355X; prints one JSON object and writes it to --out."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sed = importlib.import_module("soundeventdetection-pytorch_amd")
L = sed._lib
MAIN_CFG = [(32, 2), (64, 2), (128, 2), (128, 1)]


def timed_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def interleaved(variants, reps, warmup, inner):
    times = {k: [] for k in variants}
    for r in range(warmup + reps):
        for k, fn in variants.items():
            ms = timed_ms(fn, inner)
            if r >= warmup:
                times[k].append(ms)
    rows = {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))} for k, v in times.items()}
    first = next(iter(rows))
    base = rows[first]["median_ms"]
    return rows, {k: rows[k]["median_ms"] / base for k in rows}, (rows[first]["max_ms"] - rows[first]["min_ms"]) / base


def loss_calls(B, t, K, ratio, Tt, reps, warmup, inner, seed):
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(seed)
    pre = torch.randn(B, t, K, device="cuda", generator=gen) * 3
    target = (torch.rand(B, Tt, K, device="cuda", generator=gen) < 0.05).float()
    clip_t = target[:, :min(t * ratio, Tt)].max(dim=1).values.contiguous()
    loss, dpre = torch.empty(1, device="cuda"), torch.empty(B, t, K, device="cuda")
    clip = torch.empty(B, K, device="cuda")
    part = torch.empty((B * t * K + 255) // 256, device="cuda")
    ws = torch.empty(max(1, lib.sed_weak_bce_ws_bytes(B, t, K) // 8), dtype=torch.float64, device="cuda")

    def strong():
        L.check(lib.sed_bce_fwd_bwd(L.ptr(pre), L.ptr(target), L.ptr(loss), L.ptr(dpre), L.ptr(part), B, t, K, ratio, Tt, 5.0, 1.0, st),
                "bce_fwd_bwd")

    def weak(mode, tgt, frames):
        def run():
            L.check(lib.sed_weak_bce_fwd_bwd(L.ptr(pre), L.ptr(tgt), frames, L.ptr(clip), L.ptr(loss), L.ptr(dpre), 0, B, t, K, ratio, Tt,
                                             L.POOL_MODES[mode], 5.0, 1.0, 1.0, L.ptr(ws), st), "weak_bce_fwd_bwd")
        return run

    def pool():
        L.check(lib.sed_clip_pool_fwd(L.ptr(pre), L.ptr(clip), B, t, K, ratio, Tt, L.POOL_LINEAR, st), "clip_pool_fwd")

    variants = {"strong": strong}
    variants.update({f"weak_{m}": weak(m, target, Tt) for m in L.POOL_MODES})
    variants["weak_clip_linear"] = weak("linear", clip_t, 0)
    variants["pool_linear"] = pool
    # results first: the clip-label and the strong-label form of the same call give the same bits
    variants["weak_linear"]()
    a = (loss.clone(), dpre.clone())
    variants["weak_clip_linear"]()
    torch.cuda.synchronize()
    if not (torch.equal(a[0], loss) and torch.equal(a[1], dpre)):
        raise SystemExit(f"({B}, {t}, {K}): clip labels and strong labels give different results")
    rows, ratios, spread = interleaved(variants, reps, warmup, inner)
    return {"B": B, "t": t, "K": K, "ratio": ratio, "Tt": Tt, "logits": B * t * K, "target_values": B * Tt * K, "reps": reps,
            "warmup": warmup, "inner": inner, "variants": rows, "ratio_to_strong": ratios, "strong_spread": spread}


def train_steps(B, T, reps, warmup, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, T, 64, generator=gen).cuda()
    y = torch.zeros(B, T, 1)
    for b in range(B):
        for s0 in torch.randint(0, T - 200, (3,), generator=gen).tolist():
            y[b, s0:s0 + 150] = 1.0
    y = y.cuda()
    variants = {}
    for name, kw in (("off", {}), ("both", {"weak_pooling": "linear"}), ("only", {"weak_pooling": "linear", "weak_only": True})):
        torch.manual_seed(0)
        model = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="bf16").cuda()
        tr = sed.FusedTrainer(model, lr=1e-6, recall_factor=5.0, **kw)
        variants[name] = (lambda tr=tr: tr.train_step(x, y))
    rows, ratios, spread = interleaved(variants, reps, warmup, 1)
    return {"model": "Cnn_AvgPooling bf16, main config", "B": B, "T": T, "mel_bins": 64, "classes": 1, "pooling": "linear", "reps": reps,
            "warmup": warmup, "inner": 1, "variants": rows, "ratio_to_off": ratios, "off_spread": spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weak_loss_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/weak_loss_time.py measures on the MI355X: no GPU visible, nothing measured")
    calls = [loss_calls(32, 750, 1, 8, 6001, a.reps, a.warmup, 200, 0), loss_calls(32, 750, 14, 8, 6001, a.reps, a.warmup, 200, 1)]
    res = {"tool": "tools/weak_loss_time.py", "device": torch.cuda.get_device_name(0), "loss_calls": calls,
           "train_step": train_steps(32, 6001, a.reps, a.warmup, 2)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
