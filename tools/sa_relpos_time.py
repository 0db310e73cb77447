"""Times of the learned relative-position bias of the self-attention head (sed_mhsa_fwd_rel / sed_mhsa_bwd_rel with sed_relpos_expand /
sed_relpos_fold, csrc/sed_mhsa.hip) against the windowed entries on the same tensors, the same attention in torch with a materialised
float mask, and the bench-shape train step with and without the option.

  python tools/sa_relpos_time.py [--reps 20] [--warmup 3] [--out profiles/sa_relpos_time.json]

Method of tools/sa_window_time.py: interleaved (every repeat runs each variant once, `inner` calls between two device events, after
`warmup` untimed repeats), median / min / max over the repeats of the time per call, spread = (max - min) / median.
Core, at (B, t, C, H) = (32, 750, 128, 4) and (16, 750, 512, 8), SED_F32 and SED_BF16, p = 0, unwindowed and with window (32, 32):
  win_fwd_W / win_bwd_W     sed_mhsa_fwd_win / sed_mhsa_bwd_win (unwindowed: the plain instantiation)
  rel_fwd_W / rel_bwd_W     sed_mhsa_fwd_rel / sed_mhsa_bwd_rel on the same tensors and a N(0, 1) table (the backward includes its last
                            launch, the fp64 reduction of the per-wave partials)
  expand / fold             the two small launches, (32, 128) log buckets
  PREDICTED                 written down before anything was timed, from the code: the forward adds one LDS read and one add per
                            score beside 17 expf and the MFMAs -- 1.05 x; the backward adds that in both passes (about + 3 % of the
                            dK / dV pass), in the dQ pass 32 cross-lane reads and 64 selects and adds per tile beside its 16 expf and 6
                            MFMAs (about + 40 % of that pass, which is 6 / 14 of the backward) and one 128-byte store per tile, and the
                            reduction launch over (visited keys + 32) floats per wave (about 15 us at the first shape, unwindowed)
                            -- 1.25 x in bf16, 1.15 x in fp32 (the fp32 MFMAs take a larger share of a tile)
  torch (first shape)       scaled_dot_product_attention in fp32 with attn_mask = w[:, bucket(j - i)] expanded to (B, H, t, t), forward
                            and forward + backward down to w.grad: the t x t mask and its gradient are materialised
Train step: eager bf16 FusedTrainer.train_step, B = 32, T = 6001 frames of 64 mel bins, one class, Csa_AvgPooling with 4 heads:
  no option against sa_rel_pos = (32, 128), interleaved; predicted = the step without + (rel - win) forward and backward + expand + fold
  from the core measurements above.
Needs the MI355X; prints one JSON object and writes it to --out."""
import argparse
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
WINDOWS = [(UNB, UNB), (32, 32)]
BUCKETS = ("log", 32, 128)
PREDICTED = {"fwd_ratio": {"bf16": 1.05, "fp32": 1.05}, "bwd_ratio": {"bf16": 1.25, "fp32": 1.15}}


def wname(w):
    return "_".join("inf" if v == UNB else str(v) for v in w)


def core(B, t, C, H, dtype, reps, warmup, inner, with_torch):
    lib, st, P = L.lib(), torch.cuda.current_stream().cuda_stream, L.ptr
    dh, nb = C // H, sed.CnnEngine.rel_pos_buckets(BUCKETS)
    gen = torch.Generator(device="cuda").manual_seed(B + C)
    qkv = torch.randn(B * t, 3 * C, device="cuda", generator=gen)
    dctx = torch.randn(B * t, C, device="cuda", generator=gen) * 0.1
    w = torch.randn(H, nb, device="cuda", generator=gen)
    mp = torch.from_numpy(sed.CnnEngine.rel_pos_map(BUCKETS, t)).cuda()
    rel, drel, dw = torch.empty(H, 2 * t - 1, device="cuda"), torch.empty(H, 2 * t - 1, device="cuda"), torch.empty(H, nb, device="cuda")
    ctx, lse, dqkv = torch.empty(B * t, C, device="cuda"), torch.empty(B, H, t, device="cuda"), torch.empty(B * t, 3 * C, device="cuda")
    ws = torch.empty(max(lib.sed_mhsa_bwd_rel_ws_floats(B, t, H, dh, *wd) for wd in WINDOWS), device="cuda")
    dt = L.SED_BF16 if dtype == "bf16" else L.SED_F32
    L.check(lib.sed_relpos_expand(P(w), P(mp), P(rel), H, nb, t, st), "relpos_expand")
    variants = {
        "expand": lambda: L.check(lib.sed_relpos_expand(P(w), P(mp), P(rel), H, nb, t, st), "relpos_expand"),
        "fold": lambda: L.check(lib.sed_relpos_fold(P(drel), P(mp), P(dw), H, nb, t, st), "relpos_fold"),
    }
    for wd in WINDOWS:
        n = wname(wd)
        variants["win_fwd_" + n] = lambda wd=wd: L.check(
            lib.sed_mhsa_fwd_win(dt, P(qkv), P(ctx), P(lse), B, t, H, dh, wd[0], wd[1], 0.0, None, 0, st), "mhsa_fwd_win")
        variants["rel_fwd_" + n] = lambda wd=wd: L.check(
            lib.sed_mhsa_fwd_rel(dt, P(qkv), P(ctx), P(lse), B, t, H, dh, wd[0], wd[1], 0.0, None, 0, P(rel), st), "mhsa_fwd_rel")
        # (each backward runs on the ctx / lse the last forward left: the time does not depend on the values)
        variants["win_bwd_" + n] = lambda wd=wd: L.check(
            lib.sed_mhsa_bwd_win(dt, P(qkv), P(ctx), P(dctx), P(lse), P(dqkv), P(ws), B, t, H, dh, wd[0], wd[1], 0.0, None, 0, st), "mhsa_bwd_win")
        variants["rel_bwd_" + n] = lambda wd=wd: L.check(
            lib.sed_mhsa_bwd_rel(dt, P(qkv), P(ctx), P(dctx), P(lse), P(dqkv), P(ws), B, t, H, dh, wd[0], wd[1], 0.0, None, 0, P(rel), P(drel),
                                 st), "mhsa_bwd_rel")
    if with_torch:
        q4, k4, v4 = (qkv.view(B, t, 3, H, dh)[:, :, i].permute(0, 2, 1, 3).contiguous().requires_grad_(True) for i in range(3))
        d4 = dctx.view(B, t, H, dh).permute(0, 2, 1, 3).contiguous()
        wt = w.clone().requires_grad_(True)
        i = torch.arange(t, device="cuda")
        idx = mp.long()[(i[None, :] - i[:, None]) + t - 1]

        def torch_fwd():
            with torch.no_grad():
                torch.nn.functional.scaled_dot_product_attention(q4, k4, v4, attn_mask=wt[:, idx][None].expand(B, H, t, t))

        def torch_fwd_bwd():
            for a in (q4, k4, v4, wt):
                a.grad = None
            torch.nn.functional.scaled_dot_product_attention(q4, k4, v4, attn_mask=wt[:, idx][None].expand(B, H, t, t)).backward(d4)

        variants["torch_fwd"], variants["torch_fwd_bwd"] = torch_fwd, torch_fwd_bwd
    for fn in variants.values():
        fn()
    res = S.interleaved(variants, reps, warmup, inner)
    out = {"B": B, "t": t, "C": C, "H": H, "dh": dh, "dtype": dtype, "buckets": list(BUCKETS[1:]), "reps": reps, "warmup": warmup, "inner": inner,
           "variants": res, "windows": {}}
    for wd in WINDOWS:
        n = wname(wd)
        out["windows"][n] = {
            "ws_floats": int(lib.sed_mhsa_bwd_rel_ws_floats(B, t, H, dh, *wd)),
            "predicted_fwd_ratio": PREDICTED["fwd_ratio"][dtype], "predicted_bwd_ratio": PREDICTED["bwd_ratio"][dtype],
            "measured_fwd_ratio": res["rel_fwd_" + n]["median_ms"] / res["win_fwd_" + n]["median_ms"],
            "measured_bwd_ratio": res["rel_bwd_" + n]["median_ms"] / res["win_bwd_" + n]["median_ms"],
            "extra_ms": (res["rel_fwd_" + n]["median_ms"] - res["win_fwd_" + n]["median_ms"]) +
                        (res["rel_bwd_" + n]["median_ms"] - res["win_bwd_" + n]["median_ms"]) + res["expand"]["median_ms"] + res["fold"]["median_ms"]}
    return out


def train_step(B, T, reps, warmup, seed, extra_ms):
    x, y = S.batch(B, T, seed)
    trainers = {}
    for name, rel_pos in (("csa", None), ("csa_rel_32_128", BUCKETS[1:])):
        torch.manual_seed(0)
        model = sed.Csa_AvgPooling(1, S.MAIN_CFG, precision="bf16", sa_heads=4, sa_rel_pos=rel_pos).cuda()
        trainers[name] = sed.FusedTrainer(model, lr=1e-6, recall_factor=5.0)
        trainers[name].train_step(x, y)
    torch.cuda.synchronize()
    steps = S.interleaved({n: (lambda tr=tr: tr.train_step(x, y)) for n, tr in trainers.items()}, reps, warmup, 1)
    return {"B": B, "T": T, "t": T // 8, "mel_bins": 64, "classes": 1, "precision": "bf16", "sa_heads": 4, "reps": reps, "warmup": warmup,
            "inner": 1, "variants": steps, "predicted_ms": steps["csa"]["median_ms"] + extra_ms, "predicted_extra_ms": extra_ms,
            "measured_extra_ms": steps["csa_rel_32_128"]["median_ms"] - steps["csa"]["median_ms"],
            "rel_over_plain": steps["csa_rel_32_128"]["median_ms"] / steps["csa"]["median_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sa_relpos_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/sa_relpos_time.py measures on the MI355X: no GPU visible, nothing measured")
    shapes = ((32, 750, 128, 4), (16, 750, 512, 8))
    cores = [core(B, t, C, H, dtype, a.reps, a.warmup, 5, with_torch=(si == 0 and dtype == "fp32"))
             for si, (B, t, C, H) in enumerate(shapes) for dtype in ("bf16", "fp32")]
    res = {"tool": "tools/sa_relpos_time.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "predicted": PREDICTED,
           "core": cores, "train_step": train_step(32, 6001, a.reps, a.warmup, 2, cores[0]["windows"][wname(WINDOWS[0])]["extra_ms"])}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
