"""Times of the semi-supervised calls (csrc/sed_semi.hip, sed_weak_bce_fwd_bwd_ex) against the calls they stand beside, and of the
whole bench-shape train step with the options off, with label kinds, and with a mean teacher.

  python tools/semi_time.py [--reps 30] [--warmup 3] [--out profiles/semi_time.json]

Loss calls: pre (B, t, K) = (32, 750, 1) and (32, 750, 14) with ratio = 8 and Tt = 6001 strong-label frames, the shapes of the bench
step's loss at 1 and 14 classes.  Interleaved (every repeat runs each variant once, `inner` calls between two device events, after
`warmup` untimed repeats), median / min / max over the repeats of the time per call:
  strong           sed_bce_fwd_bwd (two launches, fp32): the yardstick of bce_sel and frame_mse
  bce_sel          sed_bce_sel_fwd_bwd (two launches, double) over every second clip
  frame_mse        sed_frame_mse_fwd_bwd (two launches) against a second set of logits
  weak             sed_weak_bce_fwd_bwd, linear pooling (two launches): the yardstick of the two _ex forms
  weak_ex_bce      sed_weak_bce_fwd_bwd_ex, SED_CRIT_BCE over every second clip
  weak_ex_mse      sed_weak_bce_fwd_bwd_ex, SED_CRIT_MSE against (B, K) clip probabilities
  ema              sed_ema_update (one launch) over 575 k parameters, the main model's flat buffer
All of them are expected to be bound by their launches (tens to hundreds of thousands of logits, a 2.3 MB buffer).
Train step: Cnn_AvgPooling, bf16, B = 32, T = 6001 frames of 64 mel bins, one class (bench.py's shape, features only), eager
FusedTrainer.train_step, interleaved the same way with `inner` = 1:
  off              every option off
  kinds            the same with a (B,) kind tensor (a third of the clips each kind) and linear pooling added
  mean_teacher     mean_teacher=True with linear pooling and kinds
  forward          the student's training-mode forward alone (CnnEngine.forward)
The one expectation: mean_teacher costs about one extra training-mode forward plus a handful of launch-bound calls, so
mean_teacher / off is expected near 1 + forward / off; both ratios are reported from the same run.
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
    pre_t = pre + 0.3 * torch.randn(B, t, K, device="cuda", generator=gen)
    target = (torch.rand(B, Tt, K, device="cuda", generator=gen) < 0.05).float()
    sel = (torch.arange(B, device="cuda") % 2 == 0).to(torch.uint8)
    loss, dpre = torch.empty(1, device="cuda"), torch.empty(B, t, K, device="cuda")
    clip, clip_t = torch.empty(B, K, device="cuda"), torch.empty(B, K, device="cuda")
    part = torch.empty((B * t * K + 255) // 256, device="cuda")
    ws = torch.empty(max(1, lib.sed_weak_bce_ws_bytes(B, t, K) // 8), dtype=torch.float64, device="cuda")
    sws = torch.empty(max(1, lib.sed_bce_sel_ws_bytes(B, t, K) // 8, lib.sed_frame_mse_ws_bytes(B, t, K) // 8), dtype=torch.float64,
                      device="cuda")
    L.check(lib.sed_clip_pool_fwd(L.ptr(pre_t), L.ptr(clip_t), B, t, K, ratio, Tt, L.POOL_LINEAR, st), "clip_pool_fwd")
    dims = (B, t, K, ratio, Tt)

    def strong():
        L.check(lib.sed_bce_fwd_bwd(L.ptr(pre), L.ptr(target), L.ptr(loss), L.ptr(dpre), L.ptr(part), *dims, 5.0, 1.0, st), "bce_fwd_bwd")

    def bce_sel():
        L.check(lib.sed_bce_sel_fwd_bwd(L.ptr(pre), L.ptr(target), L.ptr(sel), L.ptr(loss), L.ptr(dpre), 0, *dims, 5.0, 1.0, 1.0, L.ptr(sws),
                                        st), "bce_sel_fwd_bwd")

    def frame_mse():
        L.check(lib.sed_frame_mse_fwd_bwd(L.ptr(pre), L.ptr(pre_t), None, L.ptr(loss), L.ptr(dpre), 0, *dims, 1.0, 1.0, L.ptr(sws), st),
                "frame_mse_fwd_bwd")

    def weak():
        L.check(lib.sed_weak_bce_fwd_bwd(L.ptr(pre), L.ptr(target), Tt, L.ptr(clip), L.ptr(loss), L.ptr(dpre), 0, *dims, L.POOL_LINEAR, 5.0,
                                         1.0, 1.0, L.ptr(ws), st), "weak_bce_fwd_bwd")

    def weak_ex_bce():
        L.check(lib.sed_weak_bce_fwd_bwd_ex(L.ptr(pre), L.ptr(target), Tt, L.ptr(sel), L.CRIT_BCE, L.ptr(clip), L.ptr(loss), L.ptr(dpre), 0,
                                            *dims, L.POOL_LINEAR, 5.0, 1.0, 1.0, L.ptr(ws), st), "weak_bce_fwd_bwd_ex")

    def weak_ex_mse():
        L.check(lib.sed_weak_bce_fwd_bwd_ex(L.ptr(pre), L.ptr(clip_t), 0, None, L.CRIT_MSE, L.ptr(clip), L.ptr(loss), L.ptr(dpre), 0, *dims,
                                            L.POOL_LINEAR, 5.0, 1.0, 1.0, L.ptr(ws), st), "weak_bce_fwd_bwd_ex")

    variants = {"strong": strong, "bce_sel": bce_sel, "frame_mse": frame_mse, "weak": weak, "weak_ex_bce": weak_ex_bce,
                "weak_ex_mse": weak_ex_mse}
    rows, ratios, spread = interleaved(variants, reps, warmup, inner)
    wk = rows["weak"]["median_ms"]
    return {"B": B, "t": t, "K": K, "ratio": ratio, "Tt": Tt, "logits": B * t * K, "target_values": B * Tt * K, "reps": reps,
            "warmup": warmup, "inner": inner, "variants": rows, "ratio_to_strong": {k: ratios[k] for k in ("bce_sel", "frame_mse")},
            "ratio_to_weak": {k: rows[k]["median_ms"] / wk for k in ("weak_ex_bce", "weak_ex_mse")}, "strong_spread": spread}


def ema_call(n, reps, warmup, inner):
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    teacher, student = torch.randn(n, device="cuda"), torch.randn(n, device="cuda")
    rows, _, spread = interleaved({"ema": lambda: L.check(lib.sed_ema_update(L.ptr(teacher), L.ptr(student), n, 0.999, st), "ema_update")},
                                  reps, warmup, inner)
    return {"n": n, "bytes_moved": 12 * n, "reps": reps, "warmup": warmup, "inner": inner, "variants": rows, "spread": spread}


def train_steps(B, T, reps, warmup, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, T, 64, generator=gen).cuda()
    y = torch.zeros(B, T, 1)
    for b in range(B):
        for s0 in torch.randint(0, T - 200, (3,), generator=gen).tolist():
            y[b, s0:s0 + 150] = 1.0
    y = y.cuda()
    kind = (torch.arange(B) % 3).cuda()
    variants = {}
    for name, kw, kd in (("off", {}, None), ("kinds", {"weak_pooling": "linear"}, kind),
                         ("mean_teacher", {"weak_pooling": "linear", "mean_teacher": True}, kind)):
        torch.manual_seed(0)
        model = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="bf16").cuda()
        tr = sed.FusedTrainer(model, lr=1e-6, recall_factor=5.0, **kw)
        variants[name] = (lambda tr=tr: tr.train_step(x, y)) if kd is None else (lambda tr=tr, kd=kd: tr.train_step(x, y, kd))
    torch.manual_seed(0)
    fwd_model = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="bf16").cuda()
    P = fwd_model._tensor_dict()
    variants["forward"] = lambda: fwd_model.engine.forward(x, P, training=True)
    rows, ratios, spread = interleaved(variants, reps, warmup, 1)
    return {"model": "Cnn_AvgPooling bf16, main config", "B": B, "T": T, "mel_bins": 64, "classes": 1, "pooling": "linear", "reps": reps,
            "warmup": warmup, "inner": 1, "variants": rows, "ratio_to_off": ratios, "off_spread": spread,
            "expected_mean_teacher_ratio": 1.0 + ratios["forward"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semi_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/semi_time.py measures on the MI355X: no GPU visible, nothing measured")
    calls = [loss_calls(32, 750, 1, 8, 6001, a.reps, a.warmup, 200, 0), loss_calls(32, 750, 14, 8, 6001, a.reps, a.warmup, 200, 1)]
    res = {"tool": "tools/semi_time.py", "device": torch.cuda.get_device_name(0), "loss_calls": calls,
           "ema": ema_call(575000, a.reps, a.warmup, 200), "train_step": train_steps(32, 6001, a.reps, a.warmup, 2)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
