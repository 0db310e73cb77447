"""Times of the local attention window of the self-attention head (sed_mhsa_fwd_win / sed_mhsa_bwd_win, csrc/sed_mhsa.hip) against
the unchanged sed_mhsa_fwd / sed_mhsa_bwd, and the bench-shape train step with and without a window.

  python tools/sa_window_time.py [--reps 20] [--warmup 3] [--out profiles/sa_window_time.json]

Method of tools/sa_time.py: interleaved (every repeat runs each variant once, `inner` calls between two device events, after `warmup`
untimed repeats), median / min / max over the repeats of the time per call, spread = (max - min) / median.
Core, at (B, t, C, H) = (32, 750, 128, 4) and (16, 750, 512, 8), SED_F32 and SED_BF16, p = 0:
  plain_fwd / plain_bwd          sed_mhsa_fwd (with lse) / sed_mhsa_bwd
  win_fwd_L_R / win_bwd_L_R      the windowed entries at (32, 32), (64, 0) and (unbounded, unbounded) -- the last launches the plain
                                 instantiation and must time like the plain entry within that entry's own spread
  predicted                      visited / all tiles from sed_mhsa_win_tiles (forward: pass 0; backward: passes 1 and 2, which cost
                                 8 and 6 of its 14 MFMA units per tile), times the plain launch's time -- computed and stored before
                                 anything is timed.  The row-dot launch of the backward and the per-launch fixed costs are not in it.
Train step: eager bf16 FusedTrainer.train_step, B = 32, T = 6001 frames of 64 mel bins, one class, Csa_AvgPooling with 4 heads:
  no window against sa_window = (32, 32), interleaved.
Needs the MI355X; prints one JSON object and writes it to --out."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sa_time as S  # noqa: E402  (timed_ms / interleaved / batch: the method is that file's)

sed, L = S.sed, S.L
UNB = L.WIN_UNBOUNDED
WINDOWS = [(32, 32), (64, 0), (UNB, UNB)]


def wname(w):
    return "_".join("inf" if v == UNB else str(v) for v in w)


def predicted_ratios(lib, t):
    """window -> (forward, backward) visited / all, the backward weighted 8 : 6 between the dK / dV and the dQ pass"""
    full = lib.sed_mhsa_win_tiles(t, UNB, UNB, 0)
    out = {}
    for w in WINDOWS:
        f, kv, q = (lib.sed_mhsa_win_tiles(t, w[0], w[1], which) for which in (0, 1, 2))
        out[wname(w)] = {"tiles_fwd": f, "tiles_kv": kv, "tiles_q": q, "tiles_all": full, "fwd": f / full, "bwd": (8 * kv + 6 * q) / (14 * full)}
    return out


def core(B, t, C, H, dtype, reps, warmup, inner):
    lib, st, P = L.lib(), torch.cuda.current_stream().cuda_stream, L.ptr
    dh = C // H
    pred = predicted_ratios(lib, t)                 # before anything is timed
    gen = torch.Generator(device="cuda").manual_seed(B + C)
    qkv = torch.randn(B * t, 3 * C, device="cuda", generator=gen)
    dctx = torch.randn(B * t, C, device="cuda", generator=gen) * 0.1
    ctx, lse, dqkv = torch.empty(B * t, C, device="cuda"), torch.empty(B, H, t, device="cuda"), torch.empty(B * t, 3 * C, device="cuda")
    ws = torch.empty(lib.sed_mhsa_bwd_ws_floats(B, t, H, dh), device="cuda")
    dt = L.SED_BF16 if dtype == "bf16" else L.SED_F32
    variants = {
        "plain_fwd": lambda: L.check(lib.sed_mhsa_fwd(dt, P(qkv), P(ctx), P(lse), B, t, H, dh, st), "mhsa_fwd"),
        "plain_bwd": lambda: L.check(lib.sed_mhsa_bwd(dt, P(qkv), P(ctx), P(dctx), P(lse), P(dqkv), P(ws), B, t, H, dh, st), "mhsa_bwd"),
    }
    for w in WINDOWS:
        variants["win_fwd_" + wname(w)] = lambda w=w: L.check(
            lib.sed_mhsa_fwd_win(dt, P(qkv), P(ctx), P(lse), B, t, H, dh, w[0], w[1], 0.0, None, 0, st), "mhsa_fwd_win")
        # (each backward runs on the ctx / lse the last forward left: the time does not depend on the values)
        variants["win_bwd_" + wname(w)] = lambda w=w: L.check(
            lib.sed_mhsa_bwd_win(dt, P(qkv), P(ctx), P(dctx), P(lse), P(dqkv), P(ws), B, t, H, dh, w[0], w[1], 0.0, None, 0, st), "mhsa_bwd_win")
    variants["plain_fwd"]()
    res = S.interleaved(variants, reps, warmup, inner)
    out = {"B": B, "t": t, "C": C, "H": H, "dh": dh, "dtype": dtype, "reps": reps, "warmup": warmup, "inner": inner, "variants": res,
           "windows": {}}
    for w in WINDOWS:
        n = wname(w)
        pf, pb = res["plain_fwd"]["median_ms"], res["plain_bwd"]["median_ms"]
        out["windows"][n] = dict(pred[n], predicted_fwd_ms=pred[n]["fwd"] * pf, predicted_bwd_ms=pred[n]["bwd"] * pb,
                                 measured_fwd_ratio=res["win_fwd_" + n]["median_ms"] / pf, measured_bwd_ratio=res["win_bwd_" + n]["median_ms"] / pb)
    return out


def train_step(B, T, reps, warmup, seed):
    x, y = S.batch(B, T, seed)
    trainers = {}
    for name, window in (("csa", None), ("csa_win_32_32", (32, 32))):
        torch.manual_seed(0)
        model = sed.Csa_AvgPooling(1, S.MAIN_CFG, precision="bf16", sa_heads=4, sa_window=window).cuda()
        trainers[name] = sed.FusedTrainer(model, lr=1e-6, recall_factor=5.0)
        trainers[name].train_step(x, y)
    torch.cuda.synchronize()
    steps = S.interleaved({n: (lambda tr=tr: tr.train_step(x, y)) for n, tr in trainers.items()}, reps, warmup, 1)
    return {"B": B, "T": T, "t": T // 8, "mel_bins": 64, "classes": 1, "precision": "bf16", "sa_heads": 4, "reps": reps, "warmup": warmup,
            "inner": 1, "variants": steps, "win_over_plain": steps["csa_win_32_32"]["median_ms"] / steps["csa"]["median_ms"],
            "saved_ms": steps["csa"]["median_ms"] - steps["csa_win_32_32"]["median_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sa_window_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/sa_window_time.py measures on the MI355X: no GPU visible, nothing measured")
    cores = [core(B, t, C, H, dtype, a.reps, a.warmup, 5) for (B, t, C, H) in ((32, 750, 128, 4), (16, 750, 512, 8)) for dtype in ("bf16", "fp32")]
    res = {"tool": "tools/sa_window_time.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "core": cores,
           "train_step": train_step(32, 6001, a.reps, a.warmup, 2)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
