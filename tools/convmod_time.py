"""Times of the Conformer convolution module of the self-attention head (csrc/sed_convmod.hip): every new launch beside its byte
floor, the module's forward and backward against the same chain in torch device ops, and the train step with and without the module.

  python tools/convmod_time.py [--reps 20] [--warmup 3] [--out profiles/convmod_time.json]
  python tools/convmod_time.py --csig    the device sigmoid error as the kernels use it (the C_SIG / C_DSILU of tests/convmod_formula.py)

Method of tools/sa_time.py: interleaved (every repeat runs each variant once, `inner` calls between two device events, after `warmup`
untimed repeats), median / min / max over the repeats of the time per call, spread = (max - min) / median.
At (B, t, C) = (32, 750, 128), k in {7, 31}, fp32 tensors in memory:
  dwconv_glu_fwd_train / _eval   sed_dwconv_glu_fwd with / without the stored v and the statistics partials
  bn_silu_fwd, bn_silu_bwd_reduce, dwconv_glu_bwd (both of its launches)
  module_fwd / module_bwd        the engine's launches of one module: pointwise GEMMs (SED_BF16), the new launches, the BatchNorm
                                 finalisation, the residual LayerNorm; the backward with its transposes and weight-gradient products
  torch_fwd / torch_bwd          F.glu, F.conv1d(groups=C), F.batch_norm, F.silu between two F.conv1d pointwise products and F.layer_norm
                                 on (B, C, t) fp32 tensors, autograd for the backward
  floor                          the bytes a launch must read and write over the HBM stream rate bench.py --full measures
                                 (bench.measure_peaks, this process).  At this shape every tensor is R C 4 = 12.3 MB ([R][2C]: 24.6 MB): a
                                 launch's whole working set fits the 256 MB Infinity Cache, so the HBM floor is pessimistic.
Train step: eager bf16 FusedTrainer.train_step, B = 32, T = 6001 frames of 64 mel bins, one class, Csa_AvgPooling with sa_conv_kernel
  0 and 7.  The prediction is written down before the k = 7 step is timed: (step_k0 + module_fwd + module_bwd) / step_k0 from the
  module's own launch times.
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
F = torch.nn.functional


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


def module(B, t, C, k, reps, warmup, inner, peaks):
    lib, st, P = L.lib(), torch.cuda.current_stream().cuda_stream, L.ptr
    R = B * t
    gen = torch.Generator(device="cuda").manual_seed(k)
    rn = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)
    em = lambda *shape: torch.empty(*shape, device="cuda")
    h, dy = rn(R, C), rn(R, C) / R
    w1, b1, w2, b2 = rn(2 * C, C) / C ** 0.5, rn(2 * C) * 0.1, rn(C, C) / C ** 0.5, rn(C) * 0.1
    wd, bd = rn(C, k) / k ** 0.5, rn(C) * 0.1
    gamma, beta, lg, lb = 1 + 0.1 * rn(C), 0.1 * rn(C), 1 + 0.1 * rn(C), 0.1 * rn(C)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    g, v, z, s, o, hc, stats = em(R, 2 * C), em(R, C), em(R, C), em(R, C), em(R, C), em(R, C), em(R, 2)
    scale, shift, mean, invstd, coef = em(C), em(C), em(C), em(C), em(3, C)
    nparts, bparts = lib.sed_dwconv_nparts(B, t), lib.sed_bn_silu_bwd_nparts(R)
    part, bpart = em(nparts, 2, C), em(bparts, 2, C)
    dres, ds, dg, dh = em(R, C), em(R, C), em(R, 2 * C), em(R, C)
    G = {n: torch.empty_like(a) for n, a in dict(w1=w1, b1=b1, w2=w2, b2=b2, wd=wd, bd=bd, gamma=gamma, beta=beta, lg=lg, lb=lb).items()}
    w2T, w1T = em(C, C), em(2 * C, C)
    ws = em(max(1, lib.sed_dwconv_glu_bwd_ws_floats(B, t, C, k)))
    ln_ws = em(max(1, lib.sed_add_layernorm_bwd_ws_floats(R, C)))
    ks = max(1, min(64, R // 256))
    tn_ws = em(max(1, lib.sed_gemm_tn_ws_floats(2 * C, C, ks)))
    dt = L.SED_BF16
    ck = L.check

    def dw_fwd_train():
        ck(lib.sed_dwconv_glu_fwd(P(g), P(wd), P(bd), P(z), P(v), P(part), B, t, C, k, st), "dwconv_glu_fwd")

    def dw_fwd_eval():
        ck(lib.sed_dwconv_glu_fwd(P(g), P(wd), P(bd), P(z), None, None, B, t, C, k, st), "dwconv_glu_fwd")

    def silu_fwd():
        ck(lib.sed_bn_silu_fwd(P(z), P(scale), P(shift), P(s), R, C, st), "bn_silu_fwd")

    def silu_bwd():
        ck(lib.sed_bn_silu_bwd_reduce(P(ds), P(z), P(scale), P(shift), P(mean), P(invstd), P(dres), P(bpart), R, C, st), "bn_silu_bwd_reduce")

    def dw_bwd():
        ck(lib.sed_dwconv_glu_bwd(P(dres), P(z), P(coef[0]), P(coef[1]), P(coef[2]), P(v), P(g), P(wd), P(dg), P(G["wd"]), P(G["bd"]), P(ws),
                                  B, t, C, k, st), "dwconv_glu_bwd")

    def module_fwd():
        ck(lib.sed_gemm_nt(dt, P(h), C, P(w1), C, P(b1), P(g), 2 * C, R, 2 * C, C, 1, None, st), "gemm_nt")
        dw_fwd_train()
        ck(lib.sed_bn_train_finalize(P(part), nparts, float(R), P(gamma), P(beta), P(rm), P(rv), 0.1, 1e-5, P(scale), P(shift), P(mean),
                                     P(invstd), C, C, st), "bn_train_finalize")
        silu_fwd()
        ck(lib.sed_gemm_nt(dt, P(s), C, P(w2), C, P(b2), P(o), C, R, C, C, 1, None, st), "gemm_nt")
        ck(lib.sed_add_layernorm_fwd(P(h), P(o), P(lg), P(lb), P(hc), P(stats), R, C, 1e-5, st), "add_layernorm_fwd")

    def module_bwd():
        tws = P(tn_ws) if ks > 1 else None
        ck(lib.sed_add_layernorm_bwd(P(dy), P(h), P(o), P(lg), P(stats), P(dres), P(G["lg"]), P(G["lb"]), P(ln_ws), R, C, st), "ln_bwd")
        ck(lib.sed_transpose_shift(P(w2), C, P(w2T), C, C, C, C, 0, st), "transpose")
        ck(lib.sed_gemm_nt(dt, P(dres), C, P(w2T), C, None, P(ds), C, R, C, C, 1, None, st), "gemm_nt")
        ck(lib.sed_gemm_tn(dt, P(dres), C, P(s), C, P(G["w2"]), C, P(G["b2"]), C, C, R, t, 0, ks, tws, st), "gemm_tn")
        ck(lib.sed_bn_silu_bwd_reduce(P(ds), P(z), P(scale), P(shift), P(mean), P(invstd), P(ds), P(bpart), R, C, st), "bn_silu_bwd_reduce")
        ck(lib.sed_bn_bwd_finalize(P(bpart), bparts, float(R), P(gamma), P(mean), P(invstd), P(G["gamma"]), P(G["beta"]), P(coef[0]),
                                   P(coef[1]), P(coef[2]), C, C, st), "bn_bwd_finalize")
        ck(lib.sed_dwconv_glu_bwd(P(ds), P(z), P(coef[0]), P(coef[1]), P(coef[2]), P(v), P(g), P(wd), P(dg), P(G["wd"]), P(G["bd"]), P(ws),
                                  B, t, C, k, st), "dwconv_glu_bwd")
        ck(lib.sed_gemm_tn(dt, P(dg), 2 * C, P(h), C, P(G["w1"]), C, P(G["b1"]), 2 * C, C, R, t, 0, ks, tws, st), "gemm_tn")
        ck(lib.sed_transpose_shift(P(w1), C, P(w1T), 2 * C, 2 * C, C, 2 * C, 0, st), "transpose")
        ck(lib.sed_gemm_nt(dt, P(dg), 2 * C, P(w1T), 2 * C, None, P(dh), C, R, C, 2 * C, 1, None, st), "gemm_nt")
        dh.add_(dres)

    # the same chain in torch device ops, (B, C, t) fp32
    ht = h.view(B, t, C).transpose(1, 2).contiguous().requires_grad_(True)
    tp = [a.clone().requires_grad_(True) for a in (w1.view(2 * C, C, 1), b1, wd.view(C, 1, k), bd, gamma, beta, w2.view(C, C, 1), b2, lg, lb)]
    trm, trv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    dyt = dy.view(B, t, C)

    def torch_chain():
        x = F.glu(F.conv1d(ht, tp[0], tp[1]), dim=1)
        x = F.batch_norm(F.conv1d(x, tp[2], tp[3], padding=(k - 1) // 2, groups=C), trm, trv, tp[4], tp[5], True, 0.1, 1e-5)
        x = F.conv1d(F.silu(x), tp[6], tp[7])
        return F.layer_norm((ht + x).transpose(1, 2), (C,), tp[8], tp[9], 1e-5)

    def torch_fwd():
        with torch.no_grad():
            torch_chain()

    def torch_fwd_bwd():
        torch.autograd.grad(torch_chain(), [ht] + tp, dyt)

    module_fwd()
    module_bwd()
    res = interleaved({"dwconv_glu_fwd_train": dw_fwd_train, "dwconv_glu_fwd_eval": dw_fwd_eval, "bn_silu_fwd": silu_fwd,
                       "bn_silu_bwd_reduce": silu_bwd, "dwconv_glu_bwd": dw_bwd, "module_fwd": module_fwd, "module_bwd": module_bwd,
                       "torch_fwd": torch_fwd, "torch_fwd_bwd": torch_fwd_bwd}, reps, warmup, inner)
    hbm = peaks["hbm_peak_measured_gbs"] * 1e9
    rc = 4.0 * R * C
    # bytes a launch must move: g is [R][2C]; v, z, s, ds, gz are [R][C]; dg is [R][2C]
    floors = {"dwconv_glu_fwd_train": 4 * rc, "dwconv_glu_fwd_eval": 3 * rc, "bn_silu_fwd": 2 * rc, "bn_silu_bwd_reduce": 3 * rc,
              "dwconv_glu_bwd": 7 * rc}
    med = {n: r["median_ms"] for n, r in res.items()}
    return {"B": B, "t": t, "C": C, "k": k, "gemm_dtype": "bf16", "reps": reps, "warmup": warmup, "inner": inner, "variants": res,
            "floor_ms": {n: b / hbm * 1e3 for n, b in floors.items()}, "over_floor": {n: med[n] / (b / hbm * 1e3) for n, b in floors.items()},
            "tensor_mb": rc / 1e6, "fits_infinity_cache": bool(7 * rc < 256e6),
            "module_fwd_over_torch": med["module_fwd"] / med["torch_fwd"],
            "module_fwd_bwd_over_torch": (med["module_fwd"] + med["module_bwd"]) / med["torch_fwd_bwd"]}


def batch(B, T, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, T, 64, generator=gen).cuda()
    y = torch.zeros(B, T, 1)
    for b in range(B):
        for s0 in torch.randint(0, T - 200, (3,), generator=gen).tolist():
            y[b, s0:s0 + 150] = 1.0
    return x, y.cuda()


def steps(B, T, reps, warmup, seed, module_ms):
    x, y = batch(B, T, seed)
    torch.manual_seed(0)
    tr0 = sed.FusedTrainer(sed.Csa_AvgPooling(1, MAIN_CFG, precision="bf16", sa_heads=4).cuda(), lr=1e-6, recall_factor=5.0)
    tr0.train_step(x, y)
    torch.cuda.synchronize()
    k0_alone = interleaved({"k0": lambda: tr0.train_step(x, y)}, max(5, reps // 2), warmup, 1)["k0"]["median_ms"]
    predicted = (k0_alone + module_ms) / k0_alone           # written down before the k = 7 step exists
    torch.manual_seed(0)
    tr7 = sed.FusedTrainer(sed.Csa_AvgPooling(1, MAIN_CFG, precision="bf16", sa_heads=4, sa_conv_kernel=7).cuda(), lr=1e-6, recall_factor=5.0)
    tr7.train_step(x, y)
    torch.cuda.synchronize()
    res = interleaved({"k0": lambda: tr0.train_step(x, y), "k7": lambda: tr7.train_step(x, y)}, reps, warmup, 1)
    measured = res["k7"]["median_ms"] / res["k0"]["median_ms"]
    return {"B": B, "T": T, "mel_bins": 64, "classes": 1, "precision": "bf16", "reps": reps, "warmup": warmup, "inner": 1, "variants": res,
            "k0_alone_ms": k0_alone, "module_fwd_plus_bwd_ms": module_ms, "predicted_k7_over_k0": predicted, "measured_k7_over_k0": measured}


def csig():
    """worst error of v = a sigmoid(x) in units of u |v| and of silu'(x) in units of u A(x), A = sigma (1 + |x| (1 - sigma)), u = 2^-24,
    as sed_dwconv_glu_fwd (k = 3, filter (0, 1, 0), bias 0: z = v exactly) and sed_bn_silu_bwd_reduce (ds = 1, scale 1, shift 0) compute them"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import convmod_formula as V
    lib, P, st = L.lib(), L.ptr, torch.cuda.current_stream().cuda_stream
    x = np.concatenate([np.arange(-30.0, 30.0 + 2.0 ** -11, 2.0 ** -10), [40.0] * 3]).astype(np.float32)
    n = x.size // 4 * 4
    x = x[-n:]
    rng = np.random.default_rng(0)
    a = np.concatenate([np.ones(n // 2), rng.uniform(0.5, 2.0, n - n // 2)]).astype(np.float32)
    C, R = 4, n // 4
    g = torch.from_numpy(np.concatenate([a.reshape(R, C), x.reshape(R, C)], axis=1)).cuda()
    w = torch.tensor([[0.0, 1.0, 0.0]] * C, device="cuda")
    z, v = torch.empty(R, C, device="cuda"), torch.empty(R, C, device="cuda")
    L.check(lib.sed_dwconv_glu_fwd(P(g), P(w), P(torch.zeros(C, device="cuda")), P(z), P(v), None, 1, R, C, 3, st), "dwconv_glu_fwd")
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    xs = torch.from_numpy(x.reshape(R, C)).cuda()
    gz = torch.empty(R, C, device="cuda")
    part = torch.empty(lib.sed_bn_silu_bwd_nparts(R), 2, C, device="cuda")
    L.check(lib.sed_bn_silu_bwd_reduce(P(torch.ones(R, C, device="cuda")), P(xs), P(one), P(zero), P(zero), P(one), P(gz), P(part), R, C, st),
            "bn_silu_bwd_reduce")
    s = torch.empty(R, C, device="cuda")
    L.check(lib.sed_bn_silu_fwd(P(xs), P(one), P(zero), P(s), R, C, st), "bn_silu_fwd")
    torch.cuda.synchronize()
    assert torch.equal(z, v), "z differs from v under the identity filter"
    x64, a64 = x.astype(np.float64), a.astype(np.float64)
    rv = a64 * V.sigmoid(x64)
    ev = np.abs(v.cpu().numpy().reshape(-1) - rv) / rv / V.U
    rs = x64 * V.sigmoid(x64)
    es = np.abs(s.cpu().numpy().reshape(-1) - rs) / np.where(rs != 0, np.abs(rs), 1.0) / V.U
    rg = V.silu_grad(x64)
    eg = np.abs(gz.cpu().numpy().reshape(-1) - rg) / V.silu_grad_abs(x64) / V.U
    near = np.abs(x64) <= 8.0
    return {"grid": "x = -30 ... 30 step 2^-10, and 40", "n": int(n), "glu_worst_err_in_u": float(ev.max()), "glu_worst_at": float(x[int(ev.argmax())]),
            "silu_worst_err_in_u": float(es.max()), "silu_worst_at": float(x[int(es.argmax())]),
            "silu_grad_worst_err_in_u": float(eg.max()), "silu_grad_worst_at": float(x[int(eg.argmax())]),
            "within_abs_x_8": {"glu_worst_err_in_u": float(ev[near].max()), "silu_worst_err_in_u": float(es[near].max()),
                               "silu_grad_worst_err_in_u": float(eg[near].max())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--csig", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convmod_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/convmod_time.py measures on the MI355X: no GPU visible, nothing measured")
    if a.csig:
        print(json.dumps(csig()))
        return
    import bench
    peaks = bench.measure_peaks(sed, torch.device("cuda"))
    mods = [module(32, 750, 128, k, a.reps, a.warmup, 5, peaks) for k in (7, 31)]
    m7 = mods[0]["variants"]
    step = steps(32, 6001, a.reps, a.warmup, 2, m7["module_fwd"]["median_ms"] + m7["module_bwd"]["median_ms"])
    res = {"tool": "tools/convmod_time.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "hbm_peak_measured_gbs": peaks["hbm_peak_measured_gbs"],
           "peaks_how": "bench.measure_peaks (the stream copy / read of bench.py --full), this process",
           "sigmoid_accuracy": csig(), "module": mods, "train_step": step}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
