"""Times of the attention pooling head's calls (csrc/sed_attn.hip) against the calls they stand beside, of the attention logits
launch against its byte floor, and of the whole bench-shape train step with linear pooling and with attention pooling.

  python tools/att_time.py [--reps 30] [--warmup 3] [--out profiles/att_time.json]

Calls: (B, t, K) = (32, 750, 1) and (32, 750, 14), ratio = 8, Tt = 6001 strong-label frames, C = Cp = 512 feature channels.
Interleaved (every repeat runs each variant once, `inner` calls between two device events, after `warmup` untimed repeats),
median / min / max over the repeats of the time per call:
  weak_linear      sed_weak_bce_fwd_bwd, linear pooling (two launches): the yardstick of the loss
  att_loss         sed_att_loss_fwd_bwd on the same logits and target (two launches)
  att_pool         sed_att_pool_fwd (one launch)
  head_bwd         sed_head_bwd, K classes (two launches): the yardstick of the backward
  att_bwd          sed_att_bwd_pack + sed_head_bwd with 2K + sed_att_bwd_split (four launches): both linear layers
  att_logits       sed_att_logits_fwd (one launch).  It reads rows * Cp * 4 bytes of m; the call walks eight copies of m in turn
                   (8 x 49 MB, more than the 256 MB Infinity Cache holds), so every launch streams its rows from HBM.  Its floor is
                   those bytes over the read-only HBM stream rate bench.py --full measures (bench.measure_peaks, taken here on the
                   same device in the same process).
Train step: Cnn_AvgPooling, bf16, B = 32, T = 6001 frames of 64 mel bins, one class (bench.py's shape, features only), eager
FusedTrainer.train_step, weak_only, with linear pooling on a model without the head and with att pooling on a model with it,
interleaved the same way, `inner` = 1.  `predicted_ratio` = 1 + (att_logits + att_loss - weak_linear + att_bwd - head_bwd) / step,
from the K = 1 calls at this tool's head width (the model's own head is 128 channels wide: the prediction is an upper bound).
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
M_COPIES = 8


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
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
                "spread": float((np.max(v) - np.min(v)) / np.median(v))} for k, v in times.items()}


def calls(B, t, K, C, ratio, Tt, reps, warmup, inner, seed, read_gbs):
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rows = B * t
    pre = torch.randn(B, t, K, device="cuda", generator=gen) * 3
    att = torch.randn(B, t, K, device="cuda", generator=gen) * 2
    target = (torch.rand(B, Tt, K, device="cuda", generator=gen) < 0.05).float()
    ms = [torch.randn(rows, C, device="cuda", generator=gen) for _ in range(M_COPIES)]
    fc_w, att_w = (torch.randn(K, C, device="cuda", generator=gen) * 0.05 for _ in range(2))
    att_b = torch.zeros(K, device="cuda")
    loss, clip = torch.empty(1, device="cuda"), torch.empty(B, K, device="cuda")
    dpre, datt, out = (torch.empty(B, t, K, device="cuda") for _ in range(3))
    ws_weak = torch.empty(max(1, lib.sed_weak_bce_ws_bytes(B, t, K) // 8), dtype=torch.float64, device="cuda")
    ws_att = torch.empty(max(1, lib.sed_att_loss_ws_bytes(B, t, K) // 8), dtype=torch.float64, device="cuda")
    ws_head = torch.empty(lib.sed_head_bwd_ws_floats(B, t, C, 2 * K), device="cuda")
    dcat, wcat = torch.empty(rows, 2 * K, device="cuda"), torch.empty(2 * K, C, device="cuda")
    dwcat, dbcat = torch.empty(2 * K, C, device="cuda"), torch.empty(2 * K, device="cuda")
    g = [torch.empty(K, C, device="cuda"), torch.empty(K, device="cuda"), torch.empty(K, C, device="cuda"), torch.empty(K, device="cuda")]
    dfeat = torch.empty(rows, C, dtype=torch.bfloat16, device="cuda")
    turn = [0]
    P = L.ptr

    def weak_linear():
        L.check(lib.sed_weak_bce_fwd_bwd(P(pre), P(target), Tt, P(clip), P(loss), P(dpre), 0, B, t, K, ratio, Tt, L.POOL_LINEAR, 5.0, 1.0,
                                         1.0, P(ws_weak), st), "weak_bce_fwd_bwd")

    def att_loss():
        L.check(lib.sed_att_loss_fwd_bwd(P(pre), P(att), P(target), Tt, None, L.CRIT_BCE, P(clip), P(loss), P(dpre), P(datt), 0, B, t, K,
                                         ratio, Tt, 5.0, 1.0, 1.0, P(ws_att), st), "att_loss_fwd_bwd")

    def att_pool():
        L.check(lib.sed_att_pool_fwd(P(pre), P(att), P(clip), B, t, K, ratio, Tt, st), "att_pool_fwd")

    def head_bwd():
        L.check(lib.sed_head_bwd(L.SED_BF16, P(dpre), P(ms[0]), P(fc_w), P(g[0]), P(g[1]), P(dfeat), P(ws_head), B, t, 1, C, C, K, 1, st),
                "head_bwd")

    def att_bwd():
        L.check(lib.sed_att_bwd_pack(P(dpre), P(datt), P(fc_w), P(att_w), P(dcat), P(wcat), rows, C, K, st), "att_bwd_pack")
        L.check(lib.sed_head_bwd(L.SED_BF16, P(dcat), P(ms[0]), P(wcat), P(dwcat), P(dbcat), P(dfeat), P(ws_head), B, t, 1, C, C, 2 * K, 1,
                                 st), "head_bwd")
        L.check(lib.sed_att_bwd_split(P(dwcat), P(dbcat), P(g[0]), P(g[1]), P(g[2]), P(g[3]), C, K, st), "att_bwd_split")

    def att_logits():
        turn[0] = (turn[0] + 1) % M_COPIES
        L.check(lib.sed_att_logits_fwd(P(ms[turn[0]]), P(att_w), P(att_b), P(out), rows, C, C, K, st), "att_logits_fwd")

    variants = {"weak_linear": weak_linear, "att_loss": att_loss, "att_pool": att_pool, "head_bwd": head_bwd, "att_bwd": att_bwd,
                "att_logits": att_logits}
    res = interleaved(variants, reps, warmup, inner)
    nbytes = rows * C * 4
    floor_ms = nbytes / (read_gbs * 1e9) * 1e3
    return {"B": B, "t": t, "K": K, "C": C, "ratio": ratio, "Tt": Tt, "reps": reps, "warmup": warmup, "inner": inner, "variants": res,
            "att_logits_bytes": nbytes, "att_logits_floor_ms": floor_ms,
            "att_logits_over_floor": res["att_logits"]["median_ms"] / floor_ms,
            "att_loss_over_weak_linear": res["att_loss"]["median_ms"] / res["weak_linear"]["median_ms"],
            "att_bwd_over_head_bwd": res["att_bwd"]["median_ms"] / res["head_bwd"]["median_ms"],
            "new_launch_time_ms": res["att_logits"]["median_ms"] + res["att_loss"]["median_ms"] - res["weak_linear"]["median_ms"]
            + res["att_bwd"]["median_ms"] - res["head_bwd"]["median_ms"]}


def train_steps(B, T, reps, warmup, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, T, 64, generator=gen).cuda()
    y = torch.zeros(B, T, 1)
    for b in range(B):
        for s0 in torch.randint(0, T - 200, (3,), generator=gen).tolist():
            y[b, s0:s0 + 150] = 1.0
    y = y.cuda()
    variants = {}
    for name, att in (("linear", False), ("att", True)):
        torch.manual_seed(0)
        model = sed.Cnn_AvgPooling(1, MAIN_CFG, precision="bf16", attention=att).cuda()
        tr = sed.FusedTrainer(model, lr=1e-6, recall_factor=5.0, weak_pooling=name, weak_only=True)
        variants[name] = (lambda tr=tr: tr.train_step(x, y))
    res = interleaved(variants, reps, warmup, 1)
    return {"model": "Cnn_AvgPooling bf16, main config", "B": B, "T": T, "mel_bins": 64, "classes": 1, "weak_only": True, "reps": reps,
            "warmup": warmup, "inner": 1, "variants": res, "att_over_linear": res["att"]["median_ms"] / res["linear"]["median_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "att_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/att_time.py measures on the MI355X: no GPU visible, nothing measured")
    import bench
    peaks = bench.measure_peaks(sed, torch.device("cuda"))
    read_gbs = peaks["hbm_read_gbs"]
    cl = [calls(32, 750, 1, 512, 8, 6001, a.reps, a.warmup, 50, 0, read_gbs), calls(32, 750, 14, 512, 8, 6001, a.reps, a.warmup, 50, 1, read_gbs)]
    step = train_steps(32, 6001, a.reps, a.warmup, 2)
    step["predicted_ratio"] = 1.0 + cl[0]["new_launch_time_ms"] / step["variants"]["linear"]["median_ms"]
    res = {"tool": "tools/att_time.py", "device": torch.cuda.get_device_name(0), "hbm_read_gbs": read_gbs,
           "hbm_read_how": "bench.measure_peaks (the read-only stream of bench.py --full), this process", "calls": cl, "train_step": step}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
