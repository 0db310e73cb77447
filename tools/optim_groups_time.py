"""HIP-event times of the grouped optimizer step against the flat device-scalar step it stands beside, and of the grouped norm
against sed_grad_norm.

  python tools/optim_groups_time.py [--calls 200] [--repeats 30] [--out profiles/optim_groups_time.json]

Two flat buffers: the bench model's (Cnn_AvgPooling, main widths) and that of a 4-layer Conformer head on the same CNN
(Csa_AvgPooling, pre-LN, macaron, FFN 512, convolution module).  On each, per call (every entry point makes its own two or three
launches):
  ex_dev      sed_adam_step_ex_dev            AdamW, amsgrad, decay_every 0                  -- the yardstick
  groups_1    sed_adam_groups_step            one group, the same decay, constant rate
  groups_4    sed_adam_groups_step            the tests' four groups dealt round-robin over the parameters: (1, wd), (0.1, 0),
                                              (2.5, 3 wd) and a frozen one (its share of the elements is reported: those tiles return)
  norm        sed_grad_norm                                                                  -- the yardstick
  norm_groups sed_grad_norm_groups            one group
Prediction, stated before timing: the bytes are the same (p, g, m, v, vmax read; p, m, v, vmax written), so the ratio by bytes is 1.0,
and at these sizes (a few MB) every call is bound by its launches, not by the memory system.
Method: device events around `calls` back-to-back calls, the configurations interleaved within every repeat, the median over
`repeats`; the spread (max - min over the repeats) of the yardstick measured in the same run is the margin the ratios are read
against.  Prints one JSON object and writes it to --out."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sed = importlib.import_module("soundeventdetection-pytorch_amd")
L, T = sed._lib, sed.train
MAIN_CFG = [(32, 2), (64, 2), (128, 2), (128, 1)]
B1, B2, EPS, WD, LR = 0.9, 0.999, 1e-8, 1e-2, 1e-4


def time_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / calls


def tables(flat, assignment, specs):
    tiles, groups = T.build_tiles(flat, assignment, specs)
    return torch.from_numpy(tiles).cuda(), torch.from_numpy(groups).cuda()


def workload(model, calls, repeats):
    lib, P = L.lib(), L.ptr
    flat = T.FlatParams(model.cuda())
    n, dev = flat.numel, flat.p.device
    st = torch.cuda.current_stream().cuda_stream
    g = torch.randn(n, device=dev, generator=torch.Generator(device="cuda").manual_seed(1)) * 1e-2

    def state():
        return flat.p.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)

    runs = {}
    p, m, v, x = state()
    hyper, step = torch.tensor([LR, 0.0, 0.0, LR], device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    runs["ex_dev"] = lambda: lib.sed_adam_step_ex_dev(P(p), P(g), P(m), P(v), P(x), n, P(hyper), P(step), B1, B2, EPS, 1.0, 1.0, 0, WD,
                                                      1, None, st)
    four = [(1.0, WD, False), (0.1, 0.0, False), (2.5, 3 * WD, False), (1.0, WD, True)]
    frozen_share = 0.0
    for name, specs in (("groups_1", [(1.0, WD, False)]), ("groups_4", four)):
        asg = [i % len(specs) for i in range(len(flat.names))]
        tiles, groups = tables(flat, asg, specs)
        if name == "groups_4":
            frozen_share = float(sum(int(c) for s, c, k, _ in tiles.tolist() if specs[k][2])) * 4 / n
        pp, mm, vv, xx = state()
        gh, hy, sp = torch.zeros(len(specs), 4, device=dev), torch.zeros(4, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        runs[name] = (lambda pp=pp, mm=mm, vv=vv, xx=xx, tiles=tiles, groups=groups, gh=gh, hy=hy, sp=sp:
                      lib.sed_adam_groups_step(P(pp), P(g), P(mm), P(vv), P(xx), n, P(tiles), tiles.shape[0], P(groups), groups.shape[0],
                                               P(gh), P(hy), P(sp), LR, 0, 0, 0, 200, 0.997, 0.0, B1, B2, EPS, 1.0, 1, None, st))
    nparts = lib.sed_grad_norm_nparts(n)
    part, out = torch.zeros(nparts, dtype=torch.float64, device=dev), torch.zeros(2, device=dev)
    runs["norm"] = lambda: lib.sed_grad_norm(P(g), n, 1.0, 1.0, P(part), nparts, P(out), st)
    tiles1, groups1 = tables(flat, [0] * len(flat.names), [(1.0, WD, False)])
    part1, out1 = torch.zeros(tiles1.shape[0], dtype=torch.float64, device=dev), torch.zeros(2, device=dev)
    runs["norm_groups"] = lambda: lib.sed_grad_norm_groups(P(g), n, P(tiles1), tiles1.shape[0], P(groups1), 1.0, 1.0, P(part1), P(out1), st)
    for fn in runs.values():                    # warm-up: code objects loaded, every return code checked once
        for _ in range(20):
            L.check(fn(), "warm-up")
    torch.cuda.synchronize()
    assert abs(float(out[0]) - float(out1[0])) <= 1e-6 * float(out[0]), "the two norms disagree"
    times = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            times[k].append(time_us(fn, calls))

    def stat(t):
        return {"median_us": round(statistics.median(t), 3), "spread_us": round(max(t) - min(t), 3)}

    res = {"flat_parameters": n, "parameters": len(flat.names), "tiles": int(tiles1.shape[0]), "frozen_share_groups_4": round(frozen_share, 4)}
    res.update({k: stat(t) for k, t in times.items()})
    for k, ref in (("groups_1", "ex_dev"), ("groups_4", "ex_dev"), ("norm_groups", "norm")):
        res[k]["ratio_vs_" + ref] = round(res[k]["median_us"] / res[ref]["median_us"], 4)
        res[k]["yardstick_spread_over_median"] = round(res[ref]["spread_us"] / res[ref]["median_us"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_groups_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    torch.manual_seed(0)
    res = {"calls": a.calls, "repeats": a.repeats,
           "prediction": "equal bytes, ratio 1.0 by bytes; launch-bound at these sizes",
           "bench_cnn": workload(sed.Cnn_AvgPooling(1, MAIN_CFG, precision="bf16"), a.calls, a.repeats),
           "conformer_4_layers": workload(sed.Csa_AvgPooling(1, MAIN_CFG, precision="bf16", sa_heads=4, sa_layers=4, sa_ffn=512,
                                                              sa_conv_kernel=15, sa_norm_first=True, sa_macaron=True), a.calls, a.repeats)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
