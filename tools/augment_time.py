"""Times of the log-mel batch augmentation launch (csrc/sed_augment.hip) against the plain crop launch it replaces and against the
same transformation written with torch ops.

  python tools/augment_time.py [--reps 30] [--warmup 3] [--out profiles/augment_time.json]

Workloads: (B, T, F) = (32, 6001, 64) and (128, 30, 64) crops from a resident z-scored feature bank of --bank_frames frames (random
starts).  Per workload, interleaved (every repeat runs each variant once, `inner` launches between two device events, after
`warmup` untimed repeats), median / min / max over the repeats of the time per launch:
  a_crops        sed_logmel_crops: gather + z-score (what the dataset launches without augmentation)
  b_off          sed_logmel_augment with everything off (the identity table, no gain): must give a_crops' bits (checked)
  c_on           everything on without mixup: two time masks, two frequency masks, shift, band gain on every sample
  d_on_mixup     the same with mixup on every sample
  e_torch        d_on_mixup's transformation with torch ops: index gather for crop + shift, z-score, gain add, `lerp` for the mix,
                 `where` for the masks; the boolean time / frequency masks are built outside the timed region (in its favour);
                 its result must agree with d_on_mixup's (checked, fp32 rounding apart)
gbps is the ALGORITHMIC traffic over the median time: one read and one write of the (B, T, F) fp32 batch, two reads under full
mixup -- not what the memory system moved (masked frames are not read at all; tables, mean / std and gains are not counted).
What the byte counts predict, against a_crops: b_off and c_on move the same bytes (ratio 1), d_on_mixup 1.5 times as many.
Labels are left out (events = NULL): a_crops does not produce them either.  Needs the MI355X; prints one JSON object and writes it
to --out."""
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
A = importlib.import_module("soundeventdetection-pytorch_amd.dataset.spectogram.augment")
L = sed._lib


def timed_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def workload(B, T, F, bank_frames, reps, warmup, inner, seed):
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(seed)
    np.random.seed(seed)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    bank = torch.randn(bank_frames, F, device="cuda", generator=gen) * 10 - 30
    mean_h = (rng.standard_normal(F) - 30).astype(np.float32)
    std_h = (5 + 5 * rng.random(F)).astype(np.float32)
    mean, std = torch.from_numpy(mean_h).cuda(), torch.from_numpy(std_h).cuda()
    starts_h = rng.integers(0, bank_frames - T + 1, B).astype(np.int32)
    starts = torch.from_numpy(starts_h).cuda()
    out_a, out = torch.empty(B, T, F, device="cuda"), torch.empty(B, T, F, device="cuda")

    off = A.SpecAugmentConfig()
    on = A.SpecAugmentConfig(time_masks=2, time_mask_frames=max(1, T // 20), freq_masks=2, freq_mask_bins=8, time_shift=True,
                             filter_prob=1.0)
    tab_off, _ = A.draw(off, starts_h, T, F)
    tab_on, gain_h = A.draw(on, starts_h, T, F, std_mel=std_h)
    tab_mix = tab_on.copy()
    tab_mix[:, 2] = np.roll(np.arange(B), 1) if B > 1 else 0
    tab_mix[:, 3] = rng.uniform(0.5, 1.0, B).astype(np.float32).view(np.int32)
    gain = torch.from_numpy(gain_h).cuda()
    d_off, d_on, d_mix = (torch.from_numpy(t).cuda() for t in (tab_off, tab_on, tab_mix))

    def crops():
        L.check(lib.sed_logmel_crops(L.ptr(bank), bank_frames, starts_h.ctypes.data, L.ptr(starts), L.ptr(mean), L.ptr(std),
                                     L.ptr(out_a), B, T, F, st), "logmel_crops")

    def augment(tab_h, tab_d, g, cfg):
        def run():
            L.check(lib.sed_logmel_augment(L.ptr(bank), bank_frames, None, 0, L.ptr(mean), L.ptr(std), tab_h.ctypes.data,
                                           L.ptr(tab_d), L.ptr(g), 0.0, 0, L.ptr(out), None, B, T, F, cfg.time_masks,
                                           cfg.freq_masks, st), "logmel_augment")
        return run

    # the torch-op version of d_on_mixup: index tensors and boolean masks prepared once, outside the timed region
    ar = torch.arange(T, device="cuda")
    shift = torch.from_numpy(tab_mix[:, 1].astype(np.int64)).cuda()
    rows = starts.long()[:, None] + (ar[None, :] - shift[:, None]) % T
    partner = torch.from_numpy(tab_mix[:, 2].astype(np.int64)).cuda()
    lam = torch.from_numpy(np.ascontiguousarray(tab_mix[:, 3]).view(np.float32).copy()).cuda()[:, None, None]
    tmask = torch.zeros(B, T, dtype=torch.bool, device="cuda")
    fmask = torch.zeros(B, F, dtype=torch.bool, device="cuda")
    for b in range(B):
        for j in range(on.time_masks):
            tmask[b, tab_mix[b, 4 + 2 * j]:tab_mix[b, 4 + 2 * j] + tab_mix[b, 5 + 2 * j]] = True
        for j in range(on.freq_masks):
            c = 4 + 2 * on.time_masks + 2 * j
            fmask[b, tab_mix[b, c]:tab_mix[b, c] + tab_mix[b, c + 1]] = True
    fill = torch.zeros((), device="cuda")
    res = {}

    def torch_ops():
        u = (bank[rows] - mean) / std + gain[:, None, :]
        v = torch.lerp(u[partner], u, lam)
        res["e"] = torch.where(tmask[:, :, None] | fmask[:, None, :], fill, v)

    variants = {"a_crops": crops, "b_off": augment(tab_off, d_off, None, off), "c_on": augment(tab_on, d_on, gain, on),
                "d_on_mixup": augment(tab_mix, d_mix, gain, on), "e_torch": torch_ops}
    # results first (section "when results must not change"): b_off == a_crops bit for bit, e_torch ~ d_on_mixup
    crops()
    variants["b_off"]()
    torch.cuda.synchronize()
    if not torch.equal(out, out_a):
        raise SystemExit(f"({B}, {T}, {F}): the launch with everything off differs from sed_logmel_crops")
    variants["d_on_mixup"]()
    torch_ops()
    torch.cuda.synchronize()
    diff = float((out - res["e"]).abs().max())
    if not diff <= 1e-4:
        raise SystemExit(f"({B}, {T}, {F}): the torch-op version differs from the launch by {diff}")
    times = {k: [] for k in variants}
    for r in range(warmup + reps):
        for k, fn in variants.items():
            ms = timed_ms(fn, inner)
            if r >= warmup:
                times[k].append(ms)
    nbytes = B * T * F * 4
    traffic = {"a_crops": 2, "b_off": 2, "c_on": 2, "d_on_mixup": 3, "e_torch": 3}
    rows_out = {}
    for k, v in times.items():
        med = float(np.median(v))
        rows_out[k] = {"median_ms": med, "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
                       "algorithmic_bytes": traffic[k] * nbytes, "gbps": traffic[k] * nbytes / (med * 1e-3) / 1e9}
    a = rows_out["a_crops"]["median_ms"]
    return {"B": B, "T": T, "F": F, "bank_frames": bank_frames, "reps": reps, "warmup": warmup, "inner": inner,
            "masked_fraction": float((tmask[:, :, None] | fmask[:, None, :]).float().mean()), "torch_vs_launch_max_abs": diff,
            "variants": rows_out,
            "ratio_to_a_crops": {k: rows_out[k]["median_ms"] / a for k in rows_out},
            "a_crops_spread": (rows_out["a_crops"]["max_ms"] - rows_out["a_crops"]["min_ms"]) / a,
            "predicted_ratio_to_a_crops": {"b_off": 1.0, "c_on": 1.0, "d_on_mixup": 1.5}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bank_frames", type=int, default=384064, help="frames of the resident bank (default: 98 MB at 64 bins)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/augment_time.py measures on the MI355X: no GPU visible, nothing measured")
    rows = [workload(32, 6001, 64, a.bank_frames, a.reps, a.warmup, 50, 0),
            workload(128, 30, 64, a.bank_frames, a.reps, a.warmup, 200, 1)]
    res = {"tool": "tools/augment_time.py", "device": torch.cuda.get_device_name(0), "workloads": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
