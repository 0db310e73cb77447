"""Times of the pre-LN residual LayerNorm pair (sed_resid_layernorm_fwd / _bwd, csrc/sed_layernorm.hip) against the composed route, and the
train step of the self-attention head post-LN against pre-LN and macaron.

  python tools/sa_preln_time.py [--reps 20] [--warmup 3] [--out profiles/sa_preln_time.json]

Method of tools/ffn_time.py: interleaved (every repeat runs each variant once, `inner` calls between two device events, after `warmup`
untimed repeats), median / min / max over the repeats of the time per call, spread = (max - min) / median.
Kernel, at (R, C) = (24000, 128) and (12000, 512), fp32 tensors in memory, no dropout:
  fused_fwd      sed_resid_layernorm_fwd(x, a, s = 1): xsum, y, stats
  composed_fwd   torch.add(x, a, out=xsum), then sed_add_layernorm_fwd(xsum, zeros): the stream kept by a torch launch, the LayerNorm
                 reading it again
  fused_bwd      sed_resid_layernorm_bwd(dy, dres_in, xsum, ...) with dxsum aliased to dres_in, da NULL
  composed_bwd   sed_add_layernorm_bwd(dy, xsum, zeros) into dres, then dres_in.add_(dres)
  prediction     written down before anything is timed: the fused form saves one read and one write of an [R][C] tensor per pair
                 (forward: xsum written by the add and read again by the LayerNorm -- here the composed LayerNorm also reads the zeros;
                 backward: dres written and read again by the add), 8 R C bytes over the HBM stream rate bench.py --full measures
                 (bench.measure_peaks, this process).  Both tensors of a pair fit the 256 MiB Infinity Cache (12 MB and 24 MB), so the
                 saving may be hidden by it, as it was for the FFN: the JSON records predicted against measured.
Train step: eager bf16 FusedTrainer.train_step, B = 32, T = 6001 frames of 64 mel bins, one class, Csa_AvgPooling with two layers and
  sa_ffn = 512 (GELU): post-LN, pre-LN with the same sub-layers, pre-LN with macaron.  No target: ratios and spreads are recorded.
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
EPS = 1e-5


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


def kernel(R, C, reps, warmup, inner, peaks):
    lib, st, P = L.lib(), torch.cuda.current_stream().cuda_stream, L.ptr
    gen = torch.Generator(device="cuda").manual_seed(R + C)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)
    x, a, dy, dres_in = rnd(R, C), rnd(R, C), rnd(R, C), rnd(R, C)
    gamma, beta = 1.0 + 0.1 * rnd(C), 0.1 * rnd(C)
    zeros = torch.zeros(R, C, device="cuda")
    xsum, y, stats = torch.empty(R, C, device="cuda"), torch.empty(R, C, device="cuda"), torch.empty(R, 2, device="cuda")
    dres, dg, db = torch.empty(R, C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    ws = torch.empty(max(1, lib.sed_resid_layernorm_bwd_ws_floats(R, C)), device="cuda")
    hbm = peaks["hbm_peak_measured_gbs"] * 1e9
    predicted_saving_ms = 8.0 * R * C / hbm * 1e3               # before anything is timed: one read and one write of [R][C] floats

    def fused_fwd():
        L.check(lib.sed_resid_layernorm_fwd(P(x), P(a), 1.0, P(gamma), P(beta), P(xsum), P(y), P(stats), R, C, EPS, 0.0, None, 0, st), "resid_ln_fwd")

    def composed_fwd():
        torch.add(x, a, out=xsum)
        L.check(lib.sed_add_layernorm_fwd(P(xsum), P(zeros), P(gamma), P(beta), P(y), P(stats), R, C, EPS, st), "add_ln_fwd")

    def fused_bwd():
        L.check(lib.sed_resid_layernorm_bwd(P(dy), P(dres_in), P(xsum), P(gamma), P(stats), 1.0, P(dres_in), None, P(dg), P(db), P(ws), R, C,
                                            0.0, None, 0, st), "resid_ln_bwd")

    def composed_bwd():
        L.check(lib.sed_add_layernorm_bwd(P(dy), P(xsum), P(zeros), P(gamma), P(stats), P(dres), P(dg), P(db), P(ws), R, C, st), "add_ln_bwd")
        dres_in.add_(dres)

    fused_fwd()                                                 # xsum and stats of the timed backwards
    res = interleaved({"fused_fwd": fused_fwd, "composed_fwd": composed_fwd, "fused_bwd": fused_bwd, "composed_bwd": composed_bwd},
                      reps, warmup, inner)
    med = {k: v["median_ms"] for k, v in res.items()}
    return {"R": R, "C": C, "reps": reps, "warmup": warmup, "inner": inner, "tensor_mb": 4.0 * R * C / 1e6, "variants": res,
            "fused_fwd_over_composed": med["fused_fwd"] / med["composed_fwd"], "fused_bwd_over_composed": med["fused_bwd"] / med["composed_bwd"],
            "predicted_saving_ms": predicted_saving_ms, "measured_saving_fwd_ms": med["composed_fwd"] - med["fused_fwd"],
            "measured_saving_bwd_ms": med["composed_bwd"] - med["fused_bwd"],
            "fused_fwd_gbs_algorithmic": 4.0 * 4 * R * C / med["fused_fwd"] / 1e6,     # x, a read; xsum, y written
            "fused_bwd_gbs_algorithmic": 4.0 * 6 * R * C / med["fused_bwd"] / 1e6}     # dy, xsum twice, dres_in read; dxsum written


def batch(B, T, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, T, 64, generator=gen).cuda()
    y = torch.zeros(B, T, 1)
    for b in range(B):
        for s0 in torch.randint(0, T - 200, (3,), generator=gen).tolist():
            y[b, s0:s0 + 150] = 1.0
    return x, y.cuda()


def steps(B, T, reps, warmup, seed):
    x, y = batch(B, T, seed)
    base = dict(sa_ffn=512, sa_layers=2, sa_activation="gelu")
    trainers = {}
    for name, kw in (("post_ln", dict()), ("pre_ln", dict(sa_norm_first=True)), ("pre_ln_macaron", dict(sa_norm_first=True, sa_macaron=True))):
        torch.manual_seed(0)
        trainers[name] = sed.FusedTrainer(sed.Csa_AvgPooling(1, MAIN_CFG, precision="bf16", sa_heads=4, **base, **kw).cuda(), lr=1e-6,
                                          recall_factor=5.0)
        trainers[name].train_step(x, y)
    torch.cuda.synchronize()
    res = interleaved({n: (lambda tr=tr: tr.train_step(x, y)) for n, tr in trainers.items()}, reps, warmup, 1)
    post = res["post_ln"]["median_ms"]
    return {"B": B, "T": T, "mel_bins": 64, "classes": 1, "precision": "bf16", "layers": 2, "ffn": 512, "reps": reps, "warmup": warmup, "inner": 1,
            "variants": res, "pre_ln_over_post_ln": res["pre_ln"]["median_ms"] / post,
            "pre_ln_macaron_over_post_ln": res["pre_ln_macaron"]["median_ms"] / post}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sa_preln_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/sa_preln_time.py measures on the MI355X: no GPU visible, nothing measured")
    import bench
    peaks = bench.measure_peaks(sed, torch.device("cuda"))
    kernels = [kernel(R, C, a.reps, a.warmup, 10, peaks) for (R, C) in ((24000, 128), (12000, 512))]
    step = steps(32, 6001, a.reps, a.warmup, 2)
    res = {"tool": "tools/sa_preln_time.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "hbm_peak_measured_gbs": peaks["hbm_peak_measured_gbs"],
           "peaks_how": "bench.measure_peaks (the stream copy / read of bench.py --full), this process",
           "kernel": kernels, "train_step": step}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
