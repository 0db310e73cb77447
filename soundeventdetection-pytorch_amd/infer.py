"""Inference CLI (a working counterpart of /root/reference/infer.py:9-38, whose checkpoint load is
commented out and whose imports no longer resolve): WAV file -> log-mel on the MI355X -> Cnn_AvgPooling
in eval mode -> per-frame probabilities, threshold decisions and onset times.

    python -m sed_amd.infer recording.wav --ckpt training_dir/.../iteration_5000.pth

Writes <outputs_dir>/<name>.npz (probabilities, decisions, onset_frames, onset_seconds; with --median_window / --low_threshold / --max_gap /
--min_event also events = (class, onset_s, offset_s) rows decoded on the MI355X (utils/event_utils.py) and event_frames, the same in frames;
with --clip_pooling also clip_probs (classes,), the frame probabilities pooled into one clip probability per class; with --saliency also
saliency (T, mel_bins, classes) = d(sum_t p_k(t)) / d(model input), the eval-mode input gradient; for a checkpoint of a --pcen
training the layer is rebuilt from its 'frontend.*' keys and the map is with respect to the log-mel input, through the layer) and prints the onsets.  The features are z-scored with --mean_std (the pickle the preprocessing wrote) when given:
the reference's infer.py skips the normalisation the model was trained with."""
from __future__ import annotations

import argparse
import os
import pickle

import numpy as np
import torch


def build_parser():
    p = argparse.ArgumentParser(description="SED inference on MI355X")
    p.add_argument("audio_file", type=str)
    p.add_argument("--ckpt", type=str, required=True)
    p.add_argument("--outputs_dir", type=str, default="inference_outputs", help="Directory of your workspace.")
    p.add_argument("--device", default="cuda:0", type=str)
    p.add_argument("--mean_std", type=str, default="", help="features_mean_std pickle of the training set")
    p.add_argument("--threshold", type=float, default=0.5)
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp32", "f16x3", "bf16x3"])
    p.add_argument("--mel_bins", type=int, default=None,
                   help="log-mel bins of the front-end and the model's declared input width, 1..256 (default: the config's 64)")
    p.add_argument("--saliency", action="store_true",
                   help="also write 'saliency' (T, mel_bins, classes): d(sum_t p_k(t)) / d(input) of the first channel per class k, "
                        "taken with respect to the model input (the z-scored log-mel)")
    p.add_argument("--config", default="ref_native", choices=["ref_native", "bench"],
                   help="front-end parameter set: the reference's 48 kHz constants or the 32 kHz bench set")
    p.add_argument("--host_resample", action="store_true",
                   help="downmix and resample on the host in float64 (scipy) instead of on the MI355X")
    p.add_argument("--median_window", type=float, default=0.0,
                   help="median-filter the probabilities along time over this many seconds before deciding (nearest odd frame count; "
                        "default 0 = off)")
    p.add_argument("--low_threshold", type=float, default=None,
                   help="hysteresis: an event starts where p > --threshold and extends over the frames with p > this lower value "
                        "(default: --threshold, plain thresholding)")
    p.add_argument("--max_gap", type=float, default=0.0, help="merge events at most this many seconds apart (default 0 = off)")
    p.add_argument("--min_event", type=float, default=0.0, help="drop events shorter than this many seconds (default 0 = off)")
    p.add_argument("--clip_pooling", default=None, choices=["max", "mean", "linear", "exp", "att"],
                   help="also print and write 'clip_probs' (classes,): the frame probabilities pooled over the recording into one "
                        "clip probability per class, the way the weak-label loss pools them")
    p.add_argument("--teacher", action="store_true",
                   help="load the mean teacher's weights (the checkpoint's 'teacher' entry, written by training with --mean_teacher)")
    return p


def event_options(args, fps):
    """The decode_events keyword arguments (in frames) of --median_window / --low_threshold / --max_gap / --min_event (seconds)."""
    from .utils.event_utils import seconds_to_frames, seconds_to_window
    return {"median_window": seconds_to_window(getattr(args, "median_window", 0.0), fps),
            "low_threshold": getattr(args, "low_threshold", None),
            "max_gap": seconds_to_frames(getattr(args, "max_gap", 0.0), fps),
            "min_len": max(1, seconds_to_frames(getattr(args, "min_event", 0.0), fps))}


def onset_frames(decisions):
    """Rising edges of a 0/1 frame sequence (frame 0 counts when already active)."""
    d = np.asarray(decisions).astype(np.int8).reshape(-1)
    return np.flatnonzero(np.diff(np.concatenate(([0], d))) == 1)


def load_mean_std(mean_std, mel_bins):
    """(mean, std) of a features_mean_std pickle; each must hold one entry per mel bin"""
    with open(mean_std, "rb") as f:
        d = pickle.load(f)
    mean, std = d["mean"], d["std"]
    for name, v in (("mean", mean), ("std", std)):
        if np.asarray(v).size != mel_bins:
            raise ValueError(f"--mean_std {mean_std}: {name} has {np.asarray(v).size} entries, the model takes {mel_bins} mel bins")
    return mean, std


def saliency_maps(model, x):
    """x: (1, 1, T, F) model input.  (T, F, K): the gradient of each class's summed probability, d(sum_t p_k(t)) / dx, through
    the eval-mode backward (BatchNorm with running statistics) -- one backward per class."""
    K = model.classes_num
    out = np.zeros((x.shape[2], x.shape[3], K), dtype=np.float32)
    for k in range(K):
        xg = x.detach().clone().requires_grad_(True)
        probs = torch.sigmoid(model(xg))
        probs[0, :, k].sum().backward()
        out[:, :, k] = xg.grad[0, 0].cpu().numpy()
    return out


def infer_file(audio_file, ckpt, device="cuda:0", mean_std="", threshold=0.5, precision="bf16", mel_bins=None, saliency=False,
               host_resample=False, cfg=None, median_window=1, low_threshold=None, max_gap=0, min_len=1, clip_pooling=None,
               teacher=False):
    """cfg: a SpectogramConfig (default REF_NATIVE).  The file's PCM is downmixed and resampled to cfg.working_sample_rate on the
    device (dataset_utils.AudioIngest); host_resample=True takes the float64 scipy path instead.
    median_window / max_gap / min_len (frames) and low_threshold are utils.event_utils.decode_events's: the result's 'events'
    (n, 3) = (class, onset_s, offset_s) and 'event_frames' (n, 3) int are decoded on the device.  With all four at their defaults
    they are the runs of probabilities > threshold, and 'decisions' / 'onset_frames' are what they always were; otherwise those two
    follow the decoded events.
    clip_pooling: None, or max / mean / linear / exp, or att for a checkpoint with the attention head (att_fc.*): the result gains 'clip_probs' (channels, classes), the frame probabilities
    pooled over the recording on the device (CnnEngine.clip_probs).
    teacher: load the checkpoint's 'teacher' entry (the mean teacher of a --mean_teacher training) in place of 'model'."""
    import dataclasses
    if clip_pooling is not None:
        from .engine import check_clip_pooling
        check_clip_pooling(clip_pooling)        # ('att' against the checkpoint's keys below)
    from .dataset.dataset_utils import read_multichannel_audio
    from .dataset.spectogram.preprocess import LogMelFrontEnd
    from .dataset.spectogram.spectogram_configs import REF_NATIVE
    from .models.spectogram_models import Cnn_AvgPooling
    cfg = REF_NATIVE if cfg is None else cfg
    n_mel = cfg.mel_bins if mel_bins is None else int(mel_bins)
    cfg = dataclasses.replace(cfg, mel_bins=n_mel)
    mean = std = None
    if mean_std:
        mean, std = load_mean_std(mean_std, n_mel)
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X visible: this build has no CPU inference path")
    dev = torch.device(device)
    checkpoint = torch.load(ckpt, map_location=dev)
    if teacher:
        if "teacher" not in checkpoint:
            raise ValueError(f"{ckpt} holds no 'teacher' entry: it was not written by a mean-teacher training")
        weights = checkpoint["teacher"]
    else:
        weights = checkpoint["model"] if "model" in checkpoint else checkpoint
    frontend = None
    if "frontend.log_alpha" in weights:       # a --pcen training: the layer is rebuilt from the checkpoint's own keys
        from .models.frontend_layers import PCEN
        frontend = PCEN.from_state_dict(weights, prefix="frontend.")
    attention = "att_fc.weight" in weights    # an --attention_head training: the head is rebuilt from the checkpoint's own keys
    if clip_pooling == "att" and not attention:
        raise ValueError(f"--clip_pooling att needs a checkpoint with the attention head: {ckpt} holds no 'att_fc.weight'")
    model_config = [(32, 2), (64, 2), (128, 2), (128, 1)]
    if "attn.in_proj_weight" in weights:      # a --self_attention training: heads and positional flag from the checkpoint's attn_config
        from .models.spectogram_models import Csa_AvgPooling
        heads, pos = Csa_AvgPooling.config_from_state_dict(weights)
        layers, ffn, act = Csa_AvgPooling.encoder_config_from_state_dict(weights)      # (1, 0, relu) for a one-layer checkpoint
        norm_first, macaron = Csa_AvgPooling.block_config_from_state_dict(weights)     # (False, False: no block_config)
        model = Csa_AvgPooling(cfg.classes_num, model_config=model_config, sa_heads=heads, pos_encoding=pos, mel_bins=n_mel,
                               frontend=frontend, attention=attention, sa_layers=layers, sa_ffn=ffn, sa_activation=act,
                               sa_conv_kernel=Csa_AvgPooling.conv_config_from_state_dict(weights),      # (0: no conv_config)
                               sa_window=Csa_AvgPooling.window_config_from_state_dict(weights),          # (None: no window_config)
                               sa_rel_pos=Csa_AvgPooling.rel_pos_config_from_state_dict(weights),
                               sa_norm_first=norm_first, sa_macaron=macaron).to(dev)  # (None: no rel_pos_config)
    else:
        model = Cnn_AvgPooling(cfg.classes_num, model_config=model_config, mel_bins=n_mel, frontend=frontend,
                               attention=attention).to(dev)
    model.set_precision(precision)
    model.load_state_dict(weights)
    model.eval()
    print("Preprocessing audio file..")
    if host_resample:
        audio = np.ascontiguousarray(read_multichannel_audio(audio_file, cfg.working_sample_rate, cfg).T)
    else:
        audio = read_multichannel_audio(audio_file, cfg.working_sample_rate, cfg, device=dev)        # (channels, samples), device
    fe = LogMelFrontEnd(cfg, device=dev, mean=mean, std=std)
    feats = fe(audio)                                             # (channels, 1, T, mel) = (batch, 1, T, mel)
    print("Inference..")
    with torch.no_grad():
        logits = model(feats)                                       # (1, T', classes)
    clip = None
    if clip_pooling is not None:        # the plan of the forward just run still holds its logits
        plan = model.engine.plan(feats.shape[0], feats.shape[2], feats.shape[3], feats.device)
        clip = model.engine.clip_probs(plan, clip_pooling).cpu().numpy()
    probs_dev = torch.sigmoid(logits)[0]
    probs = probs_dev.cpu().numpy()
    dec = probs > threshold
    from .utils.event_utils import decode_events
    decoded = decode_events(probs_dev, threshold=threshold, low_threshold=low_threshold, median_window=median_window,
                            max_gap=max_gap, min_len=min_len)
    ev = decoded.numpy()[:, 1:].astype(np.int64)                    # (n, 3): class, onset, offset (exclusive), in frames
    if (int(median_window), low_threshold, int(max_gap), int(min_len)) != (1, None, 0, 1):
        dec = decoded.decisions.cpu().numpy().astype(bool)
    onsets = [onset_frames(dec[:, k]) for k in range(dec.shape[1])]
    res = {"probabilities": probs, "decisions": dec, "onset_frames": onsets,
           "frames_per_second": cfg.frames_per_second, "log_mel": feats[0, 0].cpu().numpy(), "event_frames": ev,
           "events": np.stack([ev[:, 0].astype(np.float64), ev[:, 1] / cfg.frames_per_second, ev[:, 2] / cfg.frames_per_second],
                              axis=1).reshape(-1, 3)}
    if clip is not None:
        res["clip_probs"] = clip
    if saliency:
        print("Saliency..")
        res["saliency"] = saliency_maps(model, feats[:1])
    return res


def main(argv=None):
    args = build_parser().parse_args(argv)
    from .dataset.spectogram import spectogram_configs
    cfg = {"ref_native": spectogram_configs.REF_NATIVE, "bench": spectogram_configs.BENCH}[args.config]
    res = infer_file(args.audio_file, args.ckpt, args.device, args.mean_std, args.threshold, args.precision, args.mel_bins,
                     args.saliency, args.host_resample, cfg, **event_options(args, cfg.frames_per_second),
                     clip_pooling=getattr(args, "clip_pooling", None), teacher=getattr(args, "teacher", False))
    os.makedirs(args.outputs_dir, exist_ok=True)
    name = os.path.splitext(os.path.basename(args.audio_file))[0]
    fps = res["frames_per_second"]
    extra = {"saliency": res["saliency"]} if "saliency" in res else {}
    if "clip_probs" in res:
        extra["clip_probs"] = res["clip_probs"][0]
    if event_options(args, fps) != event_options(None, fps):        # an event flag was given: the file gains the event list
        extra.update(events=res["events"], event_frames=res["event_frames"])
    np.savez(os.path.join(args.outputs_dir, name + ".npz"), probabilities=res["probabilities"],
             decisions=res["decisions"], onset_frames=np.concatenate(res["onset_frames"]) if res["onset_frames"] else [],
             onset_seconds=np.concatenate(res["onset_frames"]) / fps if res["onset_frames"] else [], **extra)
    for k, on in enumerate(res["onset_frames"]):
        print(f"class {k}: {len(on)} onsets at " + ", ".join(f"{f / fps:.2f}s" for f in on[:50]))
    for k in range(res["decisions"].shape[1]):
        rows = res["events"][res["events"][:, 0] == k]
        print(f"class {k}: " + (", ".join(f"{a:.2f}-{b:.2f} s" for _, a, b in rows[:50]) if len(rows) else "no events"))
    if "clip_probs" in res:
        print(f"clip probabilities ({args.clip_pooling} pooling): " + ", ".join(f"class {k}: {v:.4f}" for k, v in enumerate(res["clip_probs"][0])))


if __name__ == "__main__":
    main()
