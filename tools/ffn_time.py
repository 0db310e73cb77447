"""Times of the fused feed-forward sub-layer (csrc/sed_ffn.hip): the kernel against the composed route and against torch, beside a
stated floor, and the train step of the self-attention head with and without FFNs and a second layer.

  python tools/ffn_time.py [--reps 20] [--warmup 3] [--out profiles/ffn_time.json]
  python tools/ffn_time.py --cact        the device GELU / GELU' error over u in [-10, 10] (the C_ACT / C_DACT of tests/ffn_formula.py)

Method of tools/sa_time.py: interleaved (every repeat runs each variant once, `inner` calls between two device events, after `warmup`
untimed repeats), median / min / max over the repeats of the time per call, spread = (max - min) / median.
Kernel, at (R, C, D) = (24000, 128, 512) and (12000, 512, 2048), GELU, SED_BF16 and SED_F32, fp32 tensors in memory:
  ffn_infer / ffn_train   sed_ffn_fwd without / with the stored pre-activation u
  composed                sed_gemm_nt (u = x w1^T + b1), torch.nn.functional.gelu into a second [R][D] tensor, sed_gemm_nt (y)
  torch                   torch.nn.functional linear / gelu / linear on tensors of the mode's type (bf16 / fp32 in memory)
  floor                   4 R C D FLOPs over the matrix peak bench.py --full measures (bench.measure_peaks, this process; the fp32-input
                          MFMA runs at 1/16 of the bf16 rate) plus the bytes every form must move -- x, y, both weights and biases
                          once, and u for the training form -- over the measured HBM stream rate
  prediction              written down before anything is timed: the inference form saves the write and the read of u, and of a, against
                          the composed route: 4 R D floats over the measured HBM stream rate = composed - ffn_infer if both ran at
                          the memory system's speed
Train step: eager bf16 FusedTrainer.train_step, B = 32, T = 6001 frames of 64 mel bins, one class, Csa_AvgPooling with sa_ffn = 0 /
  one layer, sa_ffn = 4C = 512 / one layer, sa_ffn = 512 / two layers (GELU).
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
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
                "spread": float((np.max(v) - np.min(v)) / np.median(v))} for k, v in times.items()}


def kernel(R, C, D, dtype, reps, warmup, inner, peaks):
    lib, st, P = L.lib(), torch.cuda.current_stream().cuda_stream, L.ptr
    gen = torch.Generator(device="cuda").manual_seed(R + C)
    x = torch.randn(R, C, device="cuda", generator=gen)
    w1, b1 = torch.randn(D, C, device="cuda", generator=gen) / C ** 0.5, torch.randn(D, device="cuda", generator=gen) * 0.1
    w2, b2 = torch.randn(C, D, device="cuda", generator=gen) / D ** 0.5, torch.randn(C, device="cuda", generator=gen) * 0.1
    y, u = torch.empty(R, C, device="cuda"), torch.empty(R, D, device="cuda")
    dt = L.SED_BF16 if dtype == "bf16" else L.SED_F32
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    hbm = peaks["hbm_peak_measured_gbs"] * 1e9
    peak = peaks["mfma_bf16_tflops"] * 1e12 / (1 if dtype == "bf16" else 16)
    predicted_saving_ms = 4.0 * R * D * 4 / hbm * 1e3           # before anything is timed
    xt, w1t, b1t, w2t, b2t = (v.to(tdt) for v in (x, w1, b1, w2, b2))
    F = torch.nn.functional

    def ffn_infer():
        L.check(lib.sed_ffn_fwd(dt, L.SED_ACT_GELU, P(x), P(w1), P(b1), P(w2), P(b2), P(y), None, R, C, D, st), "ffn_fwd")

    def ffn_train():
        L.check(lib.sed_ffn_fwd(dt, L.SED_ACT_GELU, P(x), P(w1), P(b1), P(w2), P(b2), P(y), P(u), R, C, D, st), "ffn_fwd")

    def composed():
        L.check(lib.sed_gemm_nt(dt, P(x), C, P(w1), C, P(b1), P(u), D, R, D, C, 1, None, st), "gemm_nt")
        act = F.gelu(u)                                     # a second [R][D] tensor (torch's caching allocator: no allocation call)
        L.check(lib.sed_gemm_nt(dt, P(act), D, P(w2), D, P(b2), P(y), C, R, C, D, 1, None, st), "gemm_nt")

    def torch_route():
        with torch.no_grad():
            F.linear(F.gelu(F.linear(xt, w1t, b1t)), w2t, b2t)

    res = interleaved({"ffn_infer": ffn_infer, "ffn_train": ffn_train, "composed": composed, "torch": torch_route}, reps, warmup, inner)
    flops = 4.0 * R * C * D
    base_bytes = 4.0 * (2 * R * C + 2 * C * D + C + D)
    floor_infer = max(flops / peak, base_bytes / hbm) * 1e3
    floor_train = max(flops / peak, (base_bytes + 4.0 * R * D) / hbm) * 1e3
    med = {k: v["median_ms"] for k, v in res.items()}
    return {"R": R, "C": C, "D": D, "dtype": dtype, "act": "gelu", "reps": reps, "warmup": warmup, "inner": inner, "variants": res,
            "floor_infer_ms": floor_infer, "floor_train_ms": floor_train, "flops": flops,
            "ffn_infer_tflops": flops / med["ffn_infer"] / 1e9, "ffn_infer_over_floor": med["ffn_infer"] / floor_infer,
            "ffn_train_over_floor": med["ffn_train"] / floor_train, "ffn_infer_over_composed": med["ffn_infer"] / med["composed"],
            "ffn_train_over_composed": med["ffn_train"] / med["composed"], "ffn_infer_over_torch": med["ffn_infer"] / med["torch"],
            "predicted_saving_ms": predicted_saving_ms, "measured_saving_ms": med["composed"] - med["ffn_infer"]}


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
    trainers = {}
    for name, kw in (("ffn0_layers1", dict()), ("ffn512_layers1", dict(sa_ffn=512, sa_activation="gelu")),
                     ("ffn512_layers2", dict(sa_ffn=512, sa_layers=2, sa_activation="gelu"))):
        torch.manual_seed(0)
        trainers[name] = sed.FusedTrainer(sed.Csa_AvgPooling(1, MAIN_CFG, precision="bf16", sa_heads=4, **kw).cuda(), lr=1e-6, recall_factor=5.0)
        trainers[name].train_step(x, y)
    torch.cuda.synchronize()
    res = interleaved({n: (lambda tr=tr: tr.train_step(x, y)) for n, tr in trainers.items()}, reps, warmup, 1)
    base = res["ffn0_layers1"]["median_ms"]
    return {"B": B, "T": T, "mel_bins": 64, "classes": 1, "precision": "bf16", "reps": reps, "warmup": warmup, "inner": 1, "variants": res,
            "ffn512_layers1_over_ffn0": res["ffn512_layers1"]["median_ms"] / base,
            "ffn512_layers2_over_ffn0": res["ffn512_layers2"]["median_ms"] / base}


def cact():
    """worst relative error of the device GELU (relative to |a|) and GELU' (relative to Phi + |u| phi) in units of 2^-24"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ffn_formula as F
    lib, P = L.lib(), L.ptr
    u = np.arange(-10.0, 10.0 + 2.0 ** -13, 2.0 ** -12).astype(np.float32)
    n = u.size
    du_, da = torch.from_numpy(u).cuda(), torch.ones(n, device="cuda")
    a, du = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    L.check(lib.sed_ffn_act_bwd(L.SED_ACT_GELU, P(du_), P(da), P(a), P(du), n, torch.cuda.current_stream().cuda_stream), "ffn_act_bwd")
    torch.cuda.synchronize()
    u64 = u.astype(np.float64)
    ra, rg = F.act_fwd(u64, "gelu"), F.act_grad(u64, "gelu")
    ea = np.abs(a.cpu().numpy() - ra) / np.where(ra != 0, np.abs(ra), 1.0) / F.U
    eg = np.abs(du.cpu().numpy() - rg) / (F.Phi(u64) + np.abs(u64) * F.phi(u64)) / F.U
    return {"grid": "u = -10 ... 10 step 2^-12", "n": int(n), "gelu_worst_rel_err_in_u": float(ea.max()), "gelu_worst_at": float(u[int(ea.argmax())]),
            "gelu_grad_worst_rel_err_in_u": float(eg.max()), "gelu_grad_worst_at": float(u[int(eg.argmax())])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cact", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffn_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ffn_time.py measures on the MI355X: no GPU visible, nothing measured")
    if a.cact:
        print(json.dumps(cact()))
        return
    import bench
    peaks = bench.measure_peaks(sed, torch.device("cuda"))
    kernels = [kernel(R, C, D, dtype, a.reps, a.warmup, 5, peaks) for (R, C, D) in ((24000, 128, 512), (12000, 512, 2048))
               for dtype in ("bf16", "fp32")]
    step = steps(32, 6001, a.reps, a.warmup, 2)
    res = {"tool": "tools/ffn_time.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "mfma_bf16_tflops": peaks["mfma_bf16_tflops"], "hbm_peak_measured_gbs": peaks["hbm_peak_measured_gbs"],
           "peaks_how": "bench.measure_peaks (the register-fed MFMA loop and the stream copy / read of bench.py --full), this process",
           "gelu_accuracy": cact(), "kernel": kernels, "train_step": step}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
