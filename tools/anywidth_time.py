"""HIP-event times of the width-general convolution kernels (csrc/sed_conv_anyw.hip).

  python tools/anywidth_time.py [--steps K] [--warmup W] [--batch B] [--frames T]

1. Train step (FusedTrainer: forward, loss, backward, Adam-amsgrad) of Cnn_AvgPooling's main widths at B = 32, T = 6001, bf16 and fp32,
   for F = 40 / 64 / 128 declared (mel_bins=F) and F = 64 undeclared.  F = 64 runs the specialised kernels either way; F = 40 runs
   the width-general kernels in every block; F = 128 only in block 0.
2. One W = 64 layer (32 -> 64 channels, B = 32, H = 6001): the forward (SED_EPI_STATS) and the weight gradient through the generic
   entries (specialised kernels) and through the _anyw entries.
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


def train_step_ms(prec, F, declared, B, T, steps, warmup):
    torch.manual_seed(0)
    model = sed.Cnn_AvgPooling(1, MAIN_CFG, precision=prec, mel_bins=F if declared else None).cuda()
    tr = sed.FusedTrainer(model, lr=1e-4, recall_factor=5.0)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, 1, T, F, device="cuda", generator=g)
    y = (torch.rand(B, T, 1, device="cuda", generator=g) < 0.2).float()
    ms = time_ms(lambda: tr.train_step(x, y), steps, warmup)
    del tr, model
    torch.cuda.empty_cache()
    return ms


def layer_ms(dt, B, H, W, Cin, Cout, steps, warmup):
    lib = L.lib()
    tdt = torch.bfloat16 if dt == L.SED_BF16 else torch.float32
    st = torch.cuda.current_stream().cuda_stream
    x = torch.randn(B, H, W, Cin, device="cuda").to(tdt)
    dz = torch.randn(B, H, W, Cout, device="cuda").to(tdt)
    z = torch.empty(B, H, W, Cout, device="cuda", dtype=tdt)
    w = torch.randn(Cout, Cin, 3, 3, device="cuda") * 0.05
    wp = torch.empty(9 * Cin * Cout, device="cuda", dtype=tdt)
    L.check(lib.sed_pack_conv_weight(dt, w.data_ptr(), wp.data_ptr(), Cout, Cin, Cout, Cin, 0, st), "pack")
    part = torch.empty(lib.sed_conv_nparts(B, H, W), 2, Cout, device="cuda")
    ws = torch.empty(lib.sed_conv_wgrad_ws_floats(B, H, W, Cin, Cout), device="cuda")
    dwp = torch.empty(9 * Cin * Cout, device="cuda")
    out = {}
    for name in ("sed_conv3x3_fwd", "sed_conv3x3_fwd_anyw"):
        fn = getattr(lib, name)
        out[name] = time_ms(lambda: L.check(fn(dt, L.PRO_NONE, L.EPI_STATS, x.data_ptr(), None, None, wp.data_ptr(), z.data_ptr(), None, None,
                                               None, None, None, part.data_ptr(), B, H, W, Cin, Cout, st), name), steps, warmup)
    for name in ("sed_conv3x3_wgrad", "sed_conv3x3_wgrad_anyw"):
        fn = getattr(lib, name)
        out[name] = time_ms(lambda: L.check(fn(dt, L.PRO_NONE, x.data_ptr(), None, None, dz.data_ptr(), dwp.data_ptr(), ws.data_ptr(), B, H, W,
                                               Cin, Cout, st), name), steps, warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=6001)
    a = ap.parse_args()
    res = {"train_step_ms": {}, "layer_w64_32to64_ms": {}}
    for prec in ("bf16", "fp32"):
        for F, declared in ((64, False), (64, True), (40, True), (128, True)):
            key = f"{prec} F{F}" + (" declared" if declared else " undeclared")
            res["train_step_ms"][key] = round(train_step_ms(prec, F, declared, a.batch, a.frames, a.steps, a.warmup), 3)
    for dt, nm in ((L.SED_BF16, "bf16"), (L.SED_F32, "fp32")):
        r = layer_ms(dt, a.batch, a.frames, 64, 32, 64, a.steps, a.warmup)
        res["layer_w64_32to64_ms"][nm] = {k: round(v, 4) for k, v in r.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
