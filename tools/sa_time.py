"""Times of the self-attention temporal head (csrc/sed_mhsa.hip): the attention core against torch's scaled_dot_product_attention
and against a stated floor, the whole head against the recurrent head's launches at the same rows, and the bench-shape train step
with and without the head.

  python tools/sa_time.py [--reps 20] [--warmup 3] [--out profiles/sa_time.json]

Method of tools/att_time.py: interleaved (every repeat runs each variant once, `inner` calls between two device events, after
`warmup` untimed repeats), median / min / max over the repeats of the time per call, spread = (max - min) / median.
Core, at (B, t, C, H) = (32, 750, 128, 4) and (16, 750, 512, 8), SED_F32 and SED_BF16:
  mhsa_fwd / mhsa_bwd     sed_mhsa_fwd (with lse) / sed_mhsa_bwd (three launches), fp32 tensors in memory in both modes
  sdpa_fwd / sdpa_fwd_bwd torch.nn.functional.scaled_dot_product_attention on (B, H, t, dh) tensors of the mode's type (fp32 / bf16 in
                          memory), forward under no_grad / forward + backward; per backend that runs when it alone is allowed
                          (flash, efficient, math) and with torch's own choice ("default")
  floor                   the MFMA FLOPs the kernels execute -- forward 4 B H t^2 dh (S and P.V), backward 14 B H t^2 dh (S and dP in
                          both passes, dV, dK, dQ; 10 without the recomputation) -- over the matrix peak bench.py --full measures
                          (bench.measure_peaks, this process; the fp32-input MFMA runs at 1/16 of the bf16 rate), plus B H t^2
                          exponentials (backward: 2 B H t^2) at the vector rate of v_exp_f32, 8 results per clock per SIMD x 4 SIMDs x
                          256 CUs x 2.4 GHz = 1.97e13 / s
Head, at the bench shape's rows (B = 32, t = 750, C = 128): heads.SaHead's forward + backward (4 heads) against
  heads.GruHead's (hidden 256), each on its own model's plan (engine.head_impl) after one train step, bf16 engines.
Train step: eager bf16 FusedTrainer.train_step, B = 32, T = 6001 frames of 64 mel bins, one class: Cnn_AvgPooling, Csa_AvgPooling and
  Crnn_AvgPooling.  predicted_ratio = 1 + (sa head forward + backward) / plain step, an upper bound (the plain head's two launches,
  which the new head replaces, are not subtracted), computed before the steps are timed.
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
EXP_PER_S = 8 * 4 * 256 * 2.4e9


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


def sdpa_variants(q, k, v, do):
    """name -> callable for every backend that runs alone, and torch's own choice; (variants, errors)"""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    sdpa = torch.nn.functional.scaled_dot_product_attention
    out, errors = {}, {}

    def fwd(backend):
        def run():
            with torch.no_grad():
                if backend is None:
                    sdpa(q, k, v)
                else:
                    with sdpa_kernel(backend):
                        sdpa(q, k, v)
        return run

    def fwd_bwd(backend):
        def run():
            for u in (q, k, v):
                u.grad = None
            if backend is None:
                sdpa(q, k, v).backward(do)
            else:
                with sdpa_kernel(backend):
                    sdpa(q, k, v).backward(do)
        return run

    for name, backend in (("default", None), ("flash", SDPBackend.FLASH_ATTENTION), ("efficient", SDPBackend.EFFICIENT_ATTENTION),
                          ("math", SDPBackend.MATH)):
        try:
            f, fb = fwd(backend), fwd_bwd(backend)
            f()
            fb()
            torch.cuda.synchronize()
            out["sdpa_fwd_" + name], out["sdpa_fwd_bwd_" + name] = f, fb
        except Exception as e:          # a backend that does not take this dtype / device
            errors[name] = str(e).splitlines()[0][:200]
    return out, errors


def core(B, t, C, H, dtype, reps, warmup, inner, peak_tflops):
    lib, st, P = L.lib(), torch.cuda.current_stream().cuda_stream, L.ptr
    dh = C // H
    gen = torch.Generator(device="cuda").manual_seed(B + C)
    qkv = torch.randn(B * t, 3 * C, device="cuda", generator=gen)
    dctx = torch.randn(B * t, C, device="cuda", generator=gen) * 0.1
    ctx, lse, dqkv = torch.empty(B * t, C, device="cuda"), torch.empty(B, H, t, device="cuda"), torch.empty(B * t, 3 * C, device="cuda")
    ws = torch.empty(lib.sed_mhsa_bwd_ws_floats(B, t, H, dh), device="cuda")
    dt = L.SED_BF16 if dtype == "bf16" else L.SED_F32
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32

    def mhsa_fwd():
        L.check(lib.sed_mhsa_fwd(dt, P(qkv), P(ctx), P(lse), B, t, H, dh, st), "mhsa_fwd")

    def mhsa_bwd():
        L.check(lib.sed_mhsa_bwd(dt, P(qkv), P(ctx), P(dctx), P(lse), P(dqkv), P(ws), B, t, H, dh, st), "mhsa_bwd")

    mhsa_fwd()
    q, k, v = (qkv.view(B, t, 3, H, dh)[:, :, i].permute(0, 2, 1, 3).contiguous().to(tdt).requires_grad_(True) for i in range(3))
    do = dctx.view(B, t, H, dh).permute(0, 2, 1, 3).contiguous().to(tdt)
    variants = {"mhsa_fwd": mhsa_fwd, "mhsa_bwd": mhsa_bwd}
    sv, errors = sdpa_variants(q, k, v, do)
    variants.update(sv)
    res = interleaved(variants, reps, warmup, inner)
    peak = peak_tflops * 1e12 / (1 if dtype == "bf16" else 16)
    n2 = float(B) * H * t * t
    floor_fwd = (4 * n2 * dh / peak + n2 / EXP_PER_S) * 1e3
    floor_bwd = (14 * n2 * dh / peak + 2 * n2 / EXP_PER_S) * 1e3
    out = {"B": B, "t": t, "C": C, "H": H, "dh": dh, "dtype": dtype, "reps": reps, "warmup": warmup, "inner": inner, "variants": res,
           "sdpa_backends_refused": errors, "floor_fwd_ms": floor_fwd, "floor_bwd_ms": floor_bwd,
           "mhsa_fwd_over_floor": res["mhsa_fwd"]["median_ms"] / floor_fwd, "mhsa_bwd_over_floor": res["mhsa_bwd"]["median_ms"] / floor_bwd,
           "mhsa_fwd_tflops": 4 * n2 * dh / res["mhsa_fwd"]["median_ms"] / 1e9, "mhsa_bwd_tflops": 14 * n2 * dh / res["mhsa_bwd"]["median_ms"] / 1e9}
    if "sdpa_fwd_default" in res:
        out["mhsa_fwd_over_sdpa_fwd"] = res["mhsa_fwd"]["median_ms"] / res["sdpa_fwd_default"]["median_ms"]
        out["mhsa_fwd_bwd_over_sdpa_fwd_bwd"] = (res["mhsa_fwd"]["median_ms"] + res["mhsa_bwd"]["median_ms"]) / res["sdpa_fwd_bwd_default"]["median_ms"]
        # torch's choice: the single backend whose time is nearest to the default's
        near = {n[len("sdpa_fwd_"):]: abs(r["median_ms"] - res["sdpa_fwd_default"]["median_ms"]) for n, r in res.items()
                if n.startswith("sdpa_fwd_") and not n.startswith("sdpa_fwd_bwd_") and n != "sdpa_fwd_default"}
        out["sdpa_default_backend_by_time"] = min(near, key=near.get) if near else None
    return out


def batch(B, T, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, T, 64, generator=gen).cuda()
    y = torch.zeros(B, T, 1)
    for b in range(B):
        for s0 in torch.randint(0, T - 200, (3,), generator=gen).tolist():
            y[b, s0:s0 + 150] = 1.0
    return x, y.cuda()


def heads_and_steps(B, T, reps, warmup, seed):
    x, y = batch(B, T, seed)
    trainers = {}
    for name, build in (("cnn", lambda: sed.Cnn_AvgPooling(1, MAIN_CFG, precision="bf16")),
                        ("csa", lambda: sed.Csa_AvgPooling(1, MAIN_CFG, precision="bf16", sa_heads=4)),
                        ("crnn", lambda: sed.Crnn_AvgPooling(1, MAIN_CFG, precision="bf16"))):
        torch.manual_seed(0)
        trainers[name] = sed.FusedTrainer(build().cuda(), lr=1e-6, recall_factor=5.0)
        trainers[name].train_step(x, y)
    torch.cuda.synchronize()
    hv = {}
    for name in ("csa", "crnn"):
        tr = trainers[name]
        head, flat = tr.engine.head_impl, tr.flat
        p = list(tr.engine._plans.values())[0]
        Pd = flat.tensor_dict()
        hv[name + "_head_fwd"] = (lambda head=head, p=p, Pd=Pd: head.forward(p, Pd, p.y[-1], True, False, True))
        hv[name + "_head_bwd"] = (lambda head=head, p=p, Pd=Pd, flat=flat: head.backward(p, Pd, flat.G, p.dpre, 1, p.dy[-1], lambda name: None))
    head = interleaved(hv, reps, warmup, 5)
    sa_ms = head["csa_head_fwd"]["median_ms"] + head["csa_head_bwd"]["median_ms"]
    gru_ms = head["crnn_head_fwd"]["median_ms"] + head["crnn_head_bwd"]["median_ms"]
    first = interleaved({"cnn": lambda: trainers["cnn"].train_step(x, y)}, 5, 2, 1)["cnn"]["median_ms"]
    predicted = 1.0 + sa_ms / first                 # before the steps below are timed
    steps = interleaved({n: (lambda tr=tr: tr.train_step(x, y)) for n, tr in trainers.items()}, reps, warmup, 1)
    return ({"B": B, "t": T // 8, "C": 128, "sa_heads": 4, "gru_hidden": 256, "precision": "bf16", "inner": 5, "variants": head,
             "sa_head_ms": sa_ms, "gru_head_ms": gru_ms, "sa_over_gru": sa_ms / gru_ms},
            {"B": B, "T": T, "mel_bins": 64, "classes": 1, "precision": "bf16", "reps": reps, "warmup": warmup, "inner": 1, "variants": steps,
             "plain_step_ms_for_prediction": first, "predicted_ratio": predicted,
             "csa_over_cnn": steps["csa"]["median_ms"] / steps["cnn"]["median_ms"],
             "crnn_over_cnn": steps["crnn"]["median_ms"] / steps["cnn"]["median_ms"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sa_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/sa_time.py measures on the MI355X: no GPU visible, nothing measured")
    import bench
    peaks = bench.measure_peaks(sed, torch.device("cuda"))
    tf = peaks["mfma_bf16_tflops"]
    cores = [core(B, t, C, H, dtype, a.reps, a.warmup, 5, tf) for (B, t, C, H) in ((32, 750, 128, 4), (16, 750, 512, 8))
             for dtype in ("bf16", "fp32")]
    head, step = heads_and_steps(32, 6001, a.reps, a.warmup, 2)
    res = {"tool": "tools/sa_time.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "mfma_bf16_tflops": tf,
           "mfma_how": "bench.measure_peaks (the register-fed MFMA loop of bench.py --full), this process", "exp_per_s": EXP_PER_S,
           "core": cores, "head": head, "train_step": step}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
