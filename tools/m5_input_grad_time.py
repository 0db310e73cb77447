"""HIP-event times of M5's input-gradient path (csrc/sed_m5_dgrad.hip, M5Engine.backward(need_dx=True)).

  python tools/m5_input_grad_time.py [--steps K] [--warmup W] [--batch B] [--out FILE]

At the M5 bench shape of tools/bench_models.py (B = 2880 frames of 31680 samples), bf16 and fp32, through M5Engine:
1. the training-mode backward (and forward + WeightedBCE + backward) without and with need_dx;
2. the eval forward without and with keep_for_grad, and the eval-mode backward without and with need_dx;
3. the new launch alone next to its yardstick on the same tensors of the plan (after a backward): bf16
   sed_m5_conv1_dgrad_fused_pool against sed_m5_conv1_wgrad_fused_pool (both read the pooled dy and z1 and rebuild dz on load), fp32
   sed_m5_conv1_dgrad against sed_m5_conv1_wgrad (both read the materialised dz).  The weight-gradient kernels are not touched by the
   change that added the data gradient, so the library's own build of them is the yardstick.
Prints one JSON object (and writes it to --out)."""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sed = importlib.import_module("soundeventdetection-pytorch_amd")
mw = importlib.import_module("soundeventdetection-pytorch_amd.models.waveform_models")
L = sed._lib
FRAME = 31680


def time_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def times(prec, B, steps, warmup):
    torch.manual_seed(0)
    model = mw.M5(1, precision=prec).cuda()
    eng, lib = model.engine, L.lib()
    P = model._tensor_dict()
    G = {n: torch.empty_like(p) for n, p in model.named_parameters()}
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, 1, FRAME, device="cuda", generator=g) * 0.1
    y = (torch.rand(B, device="cuda", generator=g) < 0.1).float()
    st = torch.cuda.current_stream().cuda_stream

    def step(dx):
        p = eng.forward(x, P, True, update_running_stats=False)
        eng.loss_and_grad(p, y, 5.0)
        eng.backward(p, P, G, need_dx=dx)

    out = {"train_fwd_bwd_ms": time_ms(lambda: step(False), steps, warmup),
           "train_fwd_bwd_dx_ms": time_ms(lambda: step(True), steps, warmup)}
    p = eng.forward(x, P, True, update_running_stats=False)
    eng.loss_and_grad(p, y, 5.0)
    out["train_bwd_ms"] = time_ms(lambda: eng.backward(p, P, G), steps, warmup)
    out["train_bwd_dx_ms"] = time_ms(lambda: eng.backward(p, P, G, need_dx=True), steps, warmup)
    # the new launch and its yardstick on the plan's own tensors (conv_block1 is processed last: its operands are still in place)
    l1 = p.layers[0]
    ca, cb, cc = l1.coef[0], l1.coef[1], l1.coef[2]
    w = P["conv_block1.0.weight"]
    dx = torch.empty(B, 1, FRAME, device="cuda")
    if prec == "bf16":
        pair = {"sed_m5_conv1_wgrad_fused_pool_ms": time_ms(lambda: L.check(lib.sed_m5_conv1_wgrad_fused_pool(
                    eng.dt, x.data_ptr(), l1.dy.data_ptr(), l1.z.data_ptr(), l1.scale.data_ptr(), l1.shift.data_ptr(), ca.data_ptr(),
                    cb.data_ptr(), cc.data_ptr(), p.c1_ws.data_ptr(), B, FRAME, st), "wgrad"), steps, warmup),
                "sed_m5_conv1_dgrad_fused_pool_ms": time_ms(lambda: L.check(lib.sed_m5_conv1_dgrad_fused_pool(
                    eng.dt, l1.dy.data_ptr(), l1.z.data_ptr(), l1.scale.data_ptr(), l1.shift.data_ptr(), ca.data_ptr(), cb.data_ptr(),
                    cc.data_ptr(), w.data_ptr(), dx.data_ptr(), B, FRAME, st), "dgrad"), steps, warmup)}
        nbytes = (l1.dy.numel() + l1.z.numel()) * 2 + dx.numel() * 4
    else:
        dz = p.scratch[0]
        pair = {"sed_m5_conv1_wgrad_ms": time_ms(lambda: L.check(lib.sed_m5_conv1_wgrad(
                    eng.dt, x.data_ptr(), dz.data_ptr(), p.c1_ws.data_ptr(), B, FRAME, st), "wgrad"), steps, warmup),
                "sed_m5_conv1_dgrad_ms": time_ms(lambda: L.check(lib.sed_m5_conv1_dgrad(
                    eng.dt, dz.data_ptr(), w.data_ptr(), dx.data_ptr(), B, FRAME, st), "dgrad"), steps, warmup)}
        nbytes = l1.z.numel() * 4 + dx.numel() * 4
    a, b = list(pair.values())
    pair["dgrad_over_wgrad"] = b / a
    pair["dgrad_GB"] = nbytes / 1e9
    pair["dgrad_GB_per_s"] = nbytes / b / 1e6
    out["conv_block1_launches"] = pair
    out["eval_fwd_ms"] = time_ms(lambda: eng.forward(x, P, False), steps, warmup)
    out["eval_fwd_keep_ms"] = time_ms(lambda: eng.forward(x, P, False, keep_for_grad=True), steps, warmup)
    p = eng.forward(x, P, False, keep_for_grad=True)
    eng.loss_and_grad(p, y, 5.0)
    out["eval_bwd_ms"] = time_ms(lambda: eng.backward(p, P, G), steps, warmup)
    out["eval_bwd_dx_ms"] = time_ms(lambda: eng.backward(p, P, G, need_dx=True), steps, warmup)
    out["bwd_dx_over_plain"] = out["train_bwd_dx_ms"] / out["train_bwd_ms"]
    del eng, model, p, x, dx
    torch.cuda.empty_cache()

    def rnd(v):
        return {k: rnd(u) for k, u in v.items()} if isinstance(v, dict) else (round(v, 4) if isinstance(v, float) else v)
    return rnd(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=2880)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    res = {"shape": [a.batch, 1, FRAME], "steps": a.steps, "warmup": a.warmup}
    for prec in ("bf16", "fp32"):
        res[prec] = times(prec, a.batch, a.steps, a.warmup)
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
