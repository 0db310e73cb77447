"""HIP-event times of the input-gradient and eval-mode backward paths (csrc/sed_c1_dx.hip, CnnEngine.backward(need_dx=True)).

  python tools/input_grad_time.py [--steps K] [--warmup W] [--batch B] [--frames T]

At the bench shape (Cnn_AvgPooling main widths, B = 32, T = 6001, F = 64), through CnnEngine:
1. forward + WeightedBCE + backward of a training step, bf16 and f16x3, without and with the input gradient (keep_for_grad /
   need_dx; bf16 at F = 64 is C1 mode, where the input gradient takes the unfused block-0 route);
2. the eval forward without and with keep_for_grad (what a grad-enabled eval forward adds), and the eval-mode backward;
3. sed_conv3x3_c1_dgrad alone, bf16 [B][T][64][32] with z1 read and recomputed, and fp32 with z1 read, with its effective
   bandwidth on its own bytes (g1 [+ z1] + x + dx).
Prints one JSON object."""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sed = importlib.import_module("soundeventdetection-pytorch_amd")
L = sed._lib
MAIN_CFG = [(32, 2), (64, 2), (128, 2), (128, 1)]


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


def engine_times(prec, B, T, F, steps, warmup):
    torch.manual_seed(0)
    model = sed.Cnn_AvgPooling(1, MAIN_CFG, precision=prec).cuda()
    eng = model.engine
    P = model._tensor_dict()
    G = {n: torch.empty_like(p) for n, p in model.named_parameters()}
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, 1, T, F, device="cuda", generator=g)
    y = (torch.rand(B, T, 1, device="cuda", generator=g) < 0.2).float()

    def step(dx):
        p = eng.forward(x, P, True, update_running_stats=False, keep_for_grad=dx)
        eng.loss_and_grad(p, y, 5.0)
        eng.backward(p, P, G, need_dx=dx)

    def eval_fwd(keep):
        return eng.forward(x, P, False, keep_for_grad=keep)

    out = {"train_fwd_bwd_ms": time_ms(lambda: step(False), steps, warmup),
           "train_fwd_bwd_dx_ms": time_ms(lambda: step(True), steps, warmup),
           "eval_fwd_ms": time_ms(lambda: eval_fwd(False), steps, warmup),
           "eval_fwd_keep_ms": time_ms(lambda: eval_fwd(True), steps, warmup)}
    p = eval_fwd(True)
    eng.loss_and_grad(p, y, 5.0)
    out["eval_bwd_ms"] = time_ms(lambda: eng.backward(p, P, G), steps, warmup)
    out["eval_bwd_dx_ms"] = time_ms(lambda: eng.backward(p, P, G, need_dx=True), steps, warmup)
    out["c1_mode"] = bool(p.c1_mode)
    del eng, model, p
    torch.cuda.empty_cache()
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}


def kernel_times(B, T, F, steps, warmup):
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    C = 32
    x = torch.randn(B, T, F, device="cuda")
    w1 = torch.randn(C, 1, 3, 3, device="cuda")
    ca, cb, cc = (torch.randn(C, device="cuda") for _ in range(3))
    dx = torch.empty(B, T, F, device="cuda")
    out = {}
    for name, tdt, dtc, given in (("bf16_z_read", torch.bfloat16, L.SED_BF16, True), ("bf16_z_recomputed", torch.bfloat16, L.SED_BF16, False),
                                  ("fp32_z_read", torch.float32, L.SED_F32, True)):
        g1 = torch.randn(B, T, F, C, device="cuda").to(tdt)
        z1 = torch.randn(B, T, F, C, device="cuda").to(tdt) if given else None
        zp = z1.data_ptr() if given else None
        ms = time_ms(lambda: L.check(lib.sed_conv3x3_c1_dgrad(dtc, g1.data_ptr(), zp, x.data_ptr(), None, None, w1.data_ptr(), ca.data_ptr(),
                                                               cb.data_ptr(), cc.data_ptr(), dx.data_ptr(), B, T, F, C, C, st), name), steps, warmup)
        nbytes = g1.numel() * g1.element_size() * (2 if given else 1) + x.numel() * 4 * (1 if not given else 0) + dx.numel() * 4
        out[name] = {"ms": round(ms, 4), "GB": round(nbytes / 1e9, 3), "GB_per_s": round(nbytes / ms / 1e6, 1)}
        del g1, z1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=6001)
    a = ap.parse_args()
    res = {"shape": [a.batch, 1, a.frames, 64]}
    for prec in ("bf16", "f16x3"):
        res[prec] = engine_times(prec, a.batch, a.frames, 64, a.steps, a.warmup)
        r = res[prec]
        r["dx_over_plain"] = round(r["train_fwd_bwd_dx_ms"] / r["train_fwd_bwd_ms"], 3)
        r["eval_keep_over_plain"] = round(r["eval_fwd_keep_ms"] / r["eval_fwd_ms"], 3)
    res["sed_conv3x3_c1_dgrad"] = kernel_times(a.batch, a.frames, 64, a.steps, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
