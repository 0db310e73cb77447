"""Times of the self-attention head's dropout twins (csrc/philox.h; the DROP instantiations of csrc/sed_mhsa.hip / sed_layernorm.hip / sed_ffn.hip):
every _drop launch beside its plain twin of the same build, and the train step with and without dropout.

  python tools/dropout_time.py [--reps 20] [--warmup 3] [--out profiles/dropout_time.json]

Method of tools/sa_time.py: interleaved (every repeat runs each variant once, `inner` calls between two device events, after `warmup`
untimed repeats), median / min / max over the repeats of the time per call, spread = (max - min) / median.
Launches at the head's shape (B, t, C, H, D) = (32, 750, 128, 4, 512), R = 24000 rows, p = 0.1, SED_BF16 and SED_F32 where the entry
takes a dtype (the LayerNorm and activation-backward launches are fp32 only).
Train step: eager bf16 FusedTrainer.train_step, B = 32, T = 6001 frames of 64 mel bins, one class, a 2-layer Csa_AvgPooling with
sa_ffn 512 and sa_conv_kernel 7 (14 dropped sites), p = 0 against p = 0.1.

Prediction, written before anything was timed.  Read from the code, a Philox call is 20 low and 20 high 32-bit multiplies plus about 60
adds and xors.  The attention kernels make four calls per lane and 32 x 32 tile beside about 17 expf and 4 (bf16) to 32 (fp32) MFMAs;
the dK / dV pass adds 64 quad permutes.  Integer multiplies are not full rate, so the calls are the larger part of a bf16 tile's work:
  sed_mhsa_fwd_drop / sed_mhsa_bwd_drop   lose visibly: 2 to 4 times the plain twin in bf16, 1.3 to 2 times in fp32 (the fp32 MFMAs
                                          hide more of it)
  sed_add_layernorm_fwd_drop / _bwd_drop  one call per lane and row (quad exchange, kept over the passes) beside 3 to 5 passes over
                                          L2-resident rows: at most 1.5 times
  sed_ffn_fwd_drop                        one call per four hidden values beside 2 x 128 MACs each on the matrix pipe: at most 1.15 times
  sed_ffn_act_bwd_drop                    one call per four elements in a bandwidth-bound launch: at most 1.5 times
  train step                              the head is a small part of the step at this size: p = 0.1 at most 1.10 times p = 0
The result records each measured ratio and whether it lies in the predicted range; the plain twin of the same build is the yardstick,
not a target.
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
PREDICTED = {"mhsa_fwd:bf16": (2.0, 4.0), "mhsa_bwd:bf16": (2.0, 4.0), "mhsa_fwd:f32": (1.3, 2.0), "mhsa_bwd:f32": (1.3, 2.0),
             "add_layernorm_fwd": (1.0, 1.5), "add_layernorm_bwd": (1.0, 1.5), "ffn_fwd:bf16": (1.0, 1.15), "ffn_fwd:f32": (1.0, 1.15),
             "ffn_act_bwd": (1.0, 1.5), "train_step": (1.0, 1.10)}


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


def launches(B, t, C, H, D, p, reps, warmup, inner):
    lib, st, P, ck = L.lib(), torch.cuda.current_stream().cuda_stream, L.ptr, L.check
    R, dh = B * t, C // H
    gen = torch.Generator(device="cuda").manual_seed(1)
    rn = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)
    em = lambda *shape: torch.empty(*shape, device="cuda")
    rng = torch.tensor([12345, 678, 9, 0], dtype=torch.int32, device="cuda")
    qkv, dctx, ctx, lse, dqkv = rn(R, 3 * C), rn(R, C) / R, em(R, C), em(B, H, t), em(R, 3 * C)
    core_ws = em(max(1, lib.sed_mhsa_bwd_ws_floats(B, t, H, dh)))
    x, a, dy, gamma, beta = rn(R, C), rn(R, C), rn(R, C) / R, 1 + 0.1 * rn(C), 0.1 * rn(C)
    y, stats, dres, da, dg, db = em(R, C), em(R, 2), em(R, C), em(R, C), em(C), em(C)
    ln_ws = em(max(1, lib.sed_add_layernorm_bwd_ws_floats(R, C)))
    w1, b1, w2, b2 = rn(D, C) / C ** 0.5, 0.1 * rn(D), rn(C, D) / D ** 0.5, 0.1 * rn(C)
    f, u, fa, fda, fdu = em(R, C), em(R, D), em(R, D), rn(R, D), em(R, D)
    variants = {}
    for name, dt in (("bf16", L.SED_BF16), ("f32", L.SED_F32)):
        variants[f"mhsa_fwd:{name}"] = (
            lambda dt=dt: ck(lib.sed_mhsa_fwd(dt, P(qkv), P(ctx), P(lse), B, t, H, dh, st), "mhsa_fwd"),
            lambda dt=dt: ck(lib.sed_mhsa_fwd_drop(dt, P(qkv), P(ctx), P(lse), B, t, H, dh, p, P(rng), 0, st), "mhsa_fwd_drop"))
        variants[f"mhsa_bwd:{name}"] = (
            lambda dt=dt: ck(lib.sed_mhsa_bwd(dt, P(qkv), P(ctx), P(dctx), P(lse), P(dqkv), P(core_ws), B, t, H, dh, st), "mhsa_bwd"),
            lambda dt=dt: ck(lib.sed_mhsa_bwd_drop(dt, P(qkv), P(ctx), P(dctx), P(lse), P(dqkv), P(core_ws), B, t, H, dh, p, P(rng), 0, st),
                             "mhsa_bwd_drop"))
        variants[f"ffn_fwd:{name}"] = (
            lambda dt=dt: ck(lib.sed_ffn_fwd(dt, L.SED_ACT_GELU, P(x), P(w1), P(b1), P(w2), P(b2), P(f), P(u), R, C, D, st), "ffn_fwd"),
            lambda dt=dt: ck(lib.sed_ffn_fwd_drop(dt, L.SED_ACT_GELU, P(x), P(w1), P(b1), P(w2), P(b2), P(f), P(u), R, C, D, p, P(rng), 3, st),
                             "ffn_fwd_drop"))
    variants["add_layernorm_fwd"] = (
        lambda: ck(lib.sed_add_layernorm_fwd(P(x), P(a), P(gamma), P(beta), P(y), P(stats), R, C, 1e-5, st), "ln_fwd"),
        lambda: ck(lib.sed_add_layernorm_fwd_drop(P(x), P(a), P(gamma), P(beta), P(y), P(stats), R, C, 1e-5, p, P(rng), 1, st), "ln_fwd_drop"))
    variants["add_layernorm_bwd"] = (
        lambda: ck(lib.sed_add_layernorm_bwd(P(dy), P(x), P(a), P(gamma), P(stats), P(dres), P(dg), P(db), P(ln_ws), R, C, st), "ln_bwd"),
        lambda: ck(lib.sed_add_layernorm_bwd_drop(P(dy), P(x), P(a), P(gamma), P(stats), P(dres), P(da), P(dg), P(db), P(ln_ws), R, C, p,
                                                  P(rng), 1, st), "ln_bwd_drop"))
    variants["ffn_act_bwd"] = (
        lambda: ck(lib.sed_ffn_act_bwd(L.SED_ACT_GELU, P(u), P(fda), P(fa), P(fdu), R * D, st), "act_bwd"),
        lambda: ck(lib.sed_ffn_act_bwd_drop(L.SED_ACT_GELU, P(u), P(fda), P(fa), P(fdu), R, D, p, P(rng), 3, st), "act_bwd_drop"))
    flat = {}
    for n, (plain, drop) in variants.items():
        flat[n + "|plain"], flat[n + "|drop"] = plain, drop
    # every launch once in dependency order (ctx, lse, stats, u exist before the backwards are timed)
    for n in ("mhsa_fwd:bf16", "add_layernorm_fwd", "ffn_fwd:bf16"):
        variants[n][0]()
    res = interleaved(flat, reps, warmup, inner)
    out = {}
    for n in variants:
        pl, dr = res[n + "|plain"], res[n + "|drop"]
        ratio = dr["median_ms"] / pl["median_ms"]
        lo, hi = PREDICTED[n]
        out[n] = {"plain": pl, "drop": dr, "drop_over_plain": ratio, "predicted_range": [lo, hi], "prediction_held": bool(lo <= ratio <= hi)}
    return {"B": B, "t": t, "C": C, "H": H, "D": D, "p": p, "reps": reps, "warmup": warmup, "inner": inner, "launches": out}


def batch(B, T, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, T, 64, generator=gen).cuda()
    y = torch.zeros(B, T, 1)
    for b in range(B):
        for s0 in torch.randint(0, T - 200, (3,), generator=gen).tolist():
            y[b, s0:s0 + 150] = 1.0
    return x, y.cuda()


def steps(B, T, reps, warmup):
    x, y = batch(B, T, 2)
    trs = {}
    for name, p in (("p0", 0.0), ("p0.1", 0.1)):
        torch.manual_seed(0)
        model = sed.Csa_AvgPooling(1, MAIN_CFG, precision="bf16", sa_heads=4, sa_layers=2, sa_ffn=512, sa_activation="gelu", sa_conv_kernel=7,
                                   sa_dropout=p, sa_dropout_seed=1).cuda()
        trs[name] = sed.FusedTrainer(model, lr=1e-6, recall_factor=5.0)
        trs[name].train_step(x, y)
    torch.cuda.synchronize()
    res = interleaved({n: (lambda tr=tr: tr.train_step(x, y)) for n, tr in trs.items()}, reps, warmup, 1)
    ratio = res["p0.1"]["median_ms"] / res["p0"]["median_ms"]
    lo, hi = PREDICTED["train_step"]
    return {"B": B, "T": T, "mel_bins": 64, "classes": 1, "precision": "bf16", "model": "sa_layers 2, sa_ffn 512 gelu, sa_conv_kernel 7, 4 heads",
            "reps": reps, "warmup": warmup, "inner": 1, "variants": res, "p0.1_over_p0": ratio, "predicted_range": [lo, hi],
            "prediction_held": bool(lo <= ratio <= hi)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/dropout_time.py measures on the MI355X: no GPU visible, nothing measured")
    res = {"tool": "tools/dropout_time.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "launches": launches(32, 750, 128, 4, 512, 0.1, a.reps, a.warmup, 5), "train_step": steps(32, 6001, a.reps, a.warmup)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
