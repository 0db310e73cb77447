"""Training CLI: every flag of /root/reference/main.py:89-117 with the same defaults, driving the
MI355X spectrogram path.  Run as `python -m sed_amd.main ...` from the repository root (or under
torch.distributed.run for data parallel: one process per GPU, RCCL gradient all-reduce).

Beyond the reference: `--dataset_name synthetic` (a seeded in-memory dataset; TAU / FilmClap audio
cannot be fetched on a box without network) and `--precision`.  `--train_features Waveform` (the
M5 model) trains through the same loop; `--dataset_name synthetic` gives a seeded
stand-in task for either feature type."""
from __future__ import annotations

import argparse
import dataclasses
import os

import torch

from .train import train
from .utils.common import WeightedBCE


def build_parser():
    p = argparse.ArgumentParser(description="SED training on MI355X")
    # Training
    p.add_argument("--dataset_dir", type=str, default="../data", help="Directory of dataset.")
    p.add_argument("--dataset_name", type=str, default="FilmClap", help="FilmClap, TAU or synthetic")
    p.add_argument("--train_features", type=str, default="Waveform", help="Spectogram or Waveform")
    # Spectogram only arguments
    p.add_argument("--preprocess_mode", type=str, default="logMel",
                   help="logMel or Complex; relevant only for Spectogram features")
    p.add_argument("--force_preprocess", action="store_true", default=False,
                   help="relevant only for Spectogram features")
    # Train
    p.add_argument("--outputs_root", type=str, default="training_dir")
    p.add_argument("--ckpt", type=str, default="")
    p.add_argument("--val_descriptor", default=0.2,
                   help="float for percentage string for specifying fold substring")
    p.add_argument("--train_tag", type=str, default="")
    # Training tricks
    p.add_argument("--augment_data", action="store_true", default=False)
    p.add_argument("--balance_classes", action="store_true", default=False,
                   help="Whether to make sure there is same number of samples with and without events")
    p.add_argument("--recall_priority", type=float, default=5, help="priority factor for the bce loss")
    # Hyper parameters
    p.add_argument("--batch_size", type=int, default=128)
    p.add_argument("--lr", type=float, default=0.000001)
    p.add_argument("--num_train_steps", type=int, default=100000)
    p.add_argument("--log_freq", type=int, default=5000)
    # Infrastructure
    p.add_argument("--device", default="cuda:0", type=str)
    p.add_argument("--num_workers", default=12, type=int,
                   help="accepted for compatibility: batches are assembled on the GPU, there are no workers")
    # this build only
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp32", "f16x3", "bf16x3"])
    p.add_argument("--mel_bins", type=int, default=None,
                   help="log-mel bins of the features and the model's declared input width, 1..256 (default: the config's 64)")
    p.add_argument("--weight_decay", type=float, default=0.0,
                   help="this build only: Adam weight decay (L2, added to the gradient); with --adamw decoupled (default 0)")
    p.add_argument("--adamw", action="store_true", default=False,
                   help="this build only: decoupled weight decay (torch.optim.AdamW) instead of L2")
    p.add_argument("--no_amsgrad", action="store_true", default=False,
                   help="this build only: plain Adam / AdamW without the amsgrad maximum (the reference trains with amsgrad)")
    p.add_argument("--clip_grad_norm", type=float, default=0.0,
                   help="this build only: clip the global gradient L2 norm to this value before the step (default 0 = off)")
    return p


def build_event_parser():
    """The event-level evaluation options (this build only).  They live in a parser of their own -- build_parser() keeps exactly
    the reference's flags plus the optimizer options -- and build_full_parser() joins the two for the command line."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--eval_events", action="store_true", default=False,
                   help="this build only: the periodic evaluation also decodes events on the GPU and logs segment- and "
                        "event-based scores")
    p.add_argument("--median_window", type=float, default=0.0,
                   help="--eval_events: median filter over this many seconds (nearest odd frame count; 0 = off)")
    p.add_argument("--max_gap", type=float, default=0.0, help="--eval_events: merge events at most this many seconds apart")
    p.add_argument("--min_event", type=float, default=0.0, help="--eval_events: drop events shorter than this many seconds")
    p.add_argument("--segment", type=float, default=1.0, help="--eval_events: segment length in seconds of the segment-based scores")
    p.add_argument("--collar", type=float, default=0.2, help="--eval_events: onset / offset collar in seconds of the event-based scores")
    return p


def build_augment_parser():
    """The log-mel batch augmentation options (this build only), in a parser of their own like the event options."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--spec_augment", action="store_true", default=False,
                   help="this build only: augment every log-mel training batch on the GPU (masks, shift, mixup, band gains); "
                        "the flags below take effect only with it")
    p.add_argument("--time_masks", type=int, default=2, help="--spec_augment: time masks per sample (0..8)")
    p.add_argument("--time_mask_frames", type=int, default=4, help="--spec_augment: a time mask is 0..this many frames wide")
    p.add_argument("--freq_masks", type=int, default=2, help="--spec_augment: frequency masks per sample (0..8)")
    p.add_argument("--freq_mask_bins", type=int, default=8, help="--spec_augment: a frequency mask is 0..this many mel bins wide")
    p.add_argument("--time_shift", action="store_true", default=False, help="--spec_augment: circular time shift inside the crop")
    p.add_argument("--mixup_prob", type=float, default=0.0, help="--spec_augment: probability that a sample is mixed with a partner")
    p.add_argument("--mixup_alpha", type=float, default=0.2, help="--spec_augment: lam = max(l, 1 - l), l ~ beta(alpha, alpha)")
    p.add_argument("--soft_labels", action="store_true", default=False,
                   help="--spec_augment: mixed labels are lam * y + (1 - lam) * y_partner instead of the maximum")
    p.add_argument("--filter_augment", type=float, default=0.0,
                   help="--spec_augment: probability of a piecewise-linear band gain (3..6 bands, -6..6 dB) per sample")
    return p


def build_weak_parser():
    """The weak-label (clip-level loss) options (this build only), in a parser of their own like the event options."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--weak_labels", default="off", choices=["off", "both", "only"],
                   help="this build only: train from clip-level labels -- the frame probabilities are pooled over time and the "
                        "loss is taken against the clip label (the maximum of the frame labels); 'both' adds it to the frame-level "
                        "loss, 'only' replaces that loss")
    p.add_argument("--weak_pooling", default="linear", choices=["max", "mean", "linear", "exp", "att"],
                   help="--weak_labels: the pooling function (linear = linear softmax, exp = exponential softmax, att = the learned "
                        "attention pooling of --attention_head)")
    p.add_argument("--weak_weight", type=float, default=1.0, help="--weak_labels: factor on the clip-level loss (> 0)")
    p.add_argument("--attention_head", action="store_true", default=False,
                   help="this build only: build the model with the attention pooling head, a second linear layer att_fc beside "
                        "event_fc whose softmax over time weighs the frame probabilities of a clip (pooling att)")
    p.add_argument("--self_attention", action="store_true", default=False,
                   help="this build only: build the model with the self-attention temporal head (Csa_AvgPooling: one multi-head "
                        "attention encoder layer over the frames of a clip between the mel-mean and event_fc); Spectogram features only")
    p.add_argument("--sa_heads", type=int, default=4, help="--self_attention: attention heads (the head width 128 / N must be 32 or 64)")
    p.add_argument("--no_pos_encoding", action="store_true", default=False,
                   help="--self_attention: leave out the sinusoidal positional table")
    p.add_argument("--sa_layers", type=int, default=1, help="--self_attention: encoder layers stacked behind the mel-mean (post-LN)")
    p.add_argument("--sa_ffn", type=int, default=0,
                   help="--self_attention: width D of the feed-forward sub-layer of every encoder layer (a multiple of 32 up to 4096, "
                        "usually 4 x 128 = 512); 0 builds the attention half of a layer only")
    p.add_argument("--sa_activation", choices=["relu", "gelu"], default="relu", help="--sa_ffn: the activation of the feed-forward sub-layer")
    p.add_argument("--sa_conv_kernel", type=int, default=0,
                   help="--self_attention: taps k of the depthwise filter of a Conformer convolution module between the attention and the "
                        "feed-forward sub-layer of every encoder layer (odd, 3 to 31); 0 builds no convolution module")
    p.add_argument("--sa_dropout", type=float, default=0.0,
                   help="--self_attention: dropout probability P in [0, 1) of the encoder layers in training (the attention probabilities, "
                        "every sub-layer's output before its residual add, the FFN hidden activation); 0 drops nothing")
    p.add_argument("--sa_dropout_seed", type=int, default=None,
                   help="--sa_dropout: the 64-bit seed of the counter-based masks (default: torch's initial seed)")
    p.add_argument("--sa_window", type=str, default=None, metavar="L[:R]",
                   help="--self_attention: local attention window of every encoder layer -- a frame attends to the L frames before it and "
                        "the R frames after it (one number: L = R; inf: that side unbounded; 64:0 is causal attention with a look-back "
                        "of 64 frames); default: every frame attends to every frame")
    p.add_argument("--sa_rel_pos", type=str, default=None, metavar="L|NB:MAXD",
                   help="--self_attention: learned relative-position bias per layer, head and bucket of the distance between two frames -- "
                        "L: distances clipped to [-L, L] (2L + 1 buckets); NB:MAXD: T5's bidirectional log buckets (NB even >= 4, "
                        "MAXD > NB / 4); usually with --no_pos_encoding; default: none")
    p.add_argument("--sa_norm_first", action="store_true", default=False,
                   help="--self_attention: pre-LN encoder layers (every LayerNorm in front of its sub-layer, a closing LayerNorm behind "
                        "the last layer): trains without a learning-rate warm-up at depth")
    p.add_argument("--sa_macaron", action="store_true", default=False,
                   help="--sa_norm_first with --sa_ffn: the Conformer block -- a second, half-weighted feed-forward sub-layer in front of "
                        "the attention and a closing LayerNorm on every layer")
    return p


def parse_sa_rel_pos(text):
    """--sa_rel_pos L | NB:MAXD -> None, L or (NB, MAXD); a ValueError for anything else (the ranges are the model's to check)"""
    if text is None:
        return None
    parts = [v.strip() for v in str(text).split(":")]
    if len(parts) > 2 or not all(v.isdigit() for v in parts):
        raise ValueError(f"--sa_rel_pos takes L or NB:MAXD with positive integers, got {text!r}")
    return int(parts[0]) if len(parts) == 1 else (int(parts[0]), int(parts[1]))


def parse_sa_window(text):
    """--sa_window L[:R] -> None or (left, right), None for a side given as inf; a ValueError for anything else"""
    if text is None:
        return None
    def side(v):
        v = v.strip().lower()
        if v == "inf":
            return None
        if not v.isdigit():
            raise ValueError(f"--sa_window takes L or L:R with non-negative integers or inf, got {text!r}")
        return int(v)
    parts = str(text).split(":")
    if len(parts) > 2:
        raise ValueError(f"--sa_window takes L or L:R with non-negative integers or inf, got {text!r}")
    return side(parts[0]), side(parts[-1])


def build_semi_parser():
    """The semi-supervised options (this build only), in a parser of their own like the weak-label options."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--mean_teacher", action="store_true",
                   help="this build only: keep a teacher whose weights are an exponential moving average of the model's and add "
                        "the MSE between the model's and the teacher's frame (and, with --weak_labels, clip) probabilities")
    p.add_argument("--ema_decay", type=float, default=0.999, help="--mean_teacher: the EMA factor, in [0, 1)")
    p.add_argument("--consistency_weight", type=float, default=2.0, help="--mean_teacher: factor on the consistency terms (>= 0)")
    p.add_argument("--consistency_rampup", type=int, default=0,
                   help="--mean_teacher: steps over which the consistency weight is ramped up (0 = constant)")
    p.add_argument("--eval_teacher", action="store_true", help="--mean_teacher: the periodic evaluation runs the teacher")
    p.add_argument("--label_kinds", type=str, default=None, metavar="S:W:U",
                   help="--dataset_name synthetic only: the shares of strongly labelled, weakly labelled and unlabelled clips, "
                        "e.g. 1:2:5; the frame-level loss then takes the strong clips and the clip-level loss the labelled ones")
    return p


def build_ranking_parser():
    """The rank-metric evaluation options (this build only), in a parser of their own like the event options."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--eval_ranking", action="store_true", default=False,
                   help="this build only: the periodic evaluation also logs corpus-level AP, ROC-AUC, d' and the best-F1 threshold "
                        "per class, sorted and scanned on the GPU")
    p.add_argument("--eval_clip_pooling", default=None, choices=["max", "mean", "linear", "exp", "att"],
                   help="--eval_ranking: also rank the recordings by their pooled clip probability against the clip label")
    return p


def build_psds_parser():
    """The PSDS evaluation options (this build only), in a parser of their own like the rank-metric options."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--eval_psds", action="store_true", default=False,
                   help="this build only: the periodic evaluation also logs the polyphonic sound detection score (PSDS, the DCASE "
                        "task-4 ranking number) over a 50-threshold sweep, counted on the GPU")
    p.add_argument("--psds_scenario", type=int, default=1, choices=[1, 2],
                   help="--eval_psds: the DCASE 2021-23 task-4 scenario (1: DTC = GTC = 0.7, no cross-trigger cost; 2: DTC = GTC = "
                        "0.1, CTTC = 0.3, cross-trigger cost 0.5)")
    p.add_argument("--psds_median_window", type=float, default=0.0,
                   help="--eval_psds: median-filter length in seconds applied to the probabilities first (0 = none)")
    return p


def build_pcen_parser():
    """The PCEN front-end layer (this build only): models/frontend_layers.py, csrc/sed_pcen.hip."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--pcen", action="store_true", default=False,
                   help="put a trainable PCEN layer (per-channel energy normalisation) between the log-mel features and the CNN; it "
                        "un-normalises the dataset's z-score with the mean / std file values (--train_features Spectogram, single "
                        "process, not with --mean_teacher)")
    p.add_argument("--pcen_fixed", action="store_true", default=False,
                   help="the PCEN layer with fixed parameters (implies --pcen): nothing of it is trained")
    p.add_argument("--pcen_alpha", type=float, default=0.98, help="--pcen: initial gain-control exponent alpha (> 0)")
    p.add_argument("--pcen_delta", type=float, default=2.0, help="--pcen: initial bias delta (> 0)")
    p.add_argument("--pcen_r", type=float, default=0.5, help="--pcen: initial root-compression exponent r (> 0)")
    p.add_argument("--pcen_s", type=float, default=0.025, help="--pcen: initial smoothing coefficient s, in (0, 1)")
    p.add_argument("--pcen_eps", type=float, default=1e-6, help="--pcen: the constant added to the smoother (> 0)")
    p.add_argument("--pcen_gain", type=float, default=1.0, help="--pcen: factor on the mel power before the layer (> 0)")
    return p


def build_schedule_parser():
    """The learning-rate schedule and parameter-group options (this build only): train.py's LRSchedule / param_groups, the kernels
    of csrc/sed_optim.hip.  In a parser of their own like the event options."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--lr_schedule", default="reference", choices=["reference", "constant", "step", "cosine", "linear", "invsqrt"],
                   help="this build only: the learning-rate schedule -- reference: lr *= 0.997 every 200 steps, the reference's (the "
                        "default, today's path); constant; step (the same rule in closed form); cosine / linear decay to --lr_floor x "
                        "lr at --lr_total_steps; invsqrt (Noam's rule); all of them after --warmup_steps of linear warm-up")
    p.add_argument("--warmup_steps", type=int, default=0, help="--lr_schedule: steps of linear warm-up from lr / W to lr (0 = none)")
    p.add_argument("--lr_total_steps", type=int, default=None,
                   help="--lr_schedule cosine / linear: the step at which the decay reaches the floor (default: --num_train_steps)")
    p.add_argument("--lr_floor", type=float, default=0.0, help="--lr_schedule cosine / linear: the final rate as a fraction of lr, in [0, 1]")
    p.add_argument("--no_decay_norm_bias", action="store_true", default=False,
                   help="this build only: no weight decay on biases and BatchNorm / LayerNorm / PCEN vectors (every parameter with "
                        "ndim <= 1), the usual AdamW recipe")
    p.add_argument("--freeze", type=str, default=None, metavar="PREFIX[,PREFIX...]",
                   help="this build only: parameters under these name prefixes (e.g. conv_blocks) are not updated")
    p.add_argument("--lr_scale", action="append", default=None, metavar="PREFIX=SCALE",
                   help="this build only: the learning rate of the parameters under PREFIX is SCALE x lr (repeatable; the first match wins)")
    return p


def build_full_parser():
    """What main() parses: build_parser(), build_event_parser(), build_augment_parser(), build_weak_parser(),
    build_semi_parser(), build_ranking_parser(), build_psds_parser(), build_pcen_parser() and build_schedule_parser() together."""
    return argparse.ArgumentParser(description="SED training on MI355X",
                                   parents=[build_parser(), build_event_parser(), build_augment_parser(), build_weak_parser(),
                                            build_semi_parser(), build_ranking_parser(), build_psds_parser(), build_pcen_parser(),
                                            build_schedule_parser()],
                                   conflict_handler="resolve")


def parse_lr_scale(items):
    """--lr_scale PREFIX=SCALE ... -> [(prefix, scale)]; a ValueError for anything else (the range is train.py's to check)"""
    out = []
    for it in items or []:
        pre, sep, val = str(it).rpartition("=")
        try:
            out.append((pre.strip(), float(val)))
        except ValueError:
            sep = ""
        if not sep or not pre.strip():
            raise ValueError(f"--lr_scale takes PREFIX=SCALE, got {it!r}")
    return out


def schedule_options(args, model=None):
    """train()'s lr_schedule / param_groups of --lr_schedule ... --lr_scale; {} with every flag at its default, the reference's path
    (a Namespace built by hand may lack any of them).  Group order: --freeze, then --lr_scale in the order given, then the
    undecayed remainder (--no_decay_norm_bias needs the model's names; without a model those groups are left out: validate_args
    checks the rest before a model exists)."""
    from .train import LRSchedule, no_decay_groups, selector_matches
    kind = getattr(args, "lr_schedule", "reference")
    sched = None
    if kind != "reference":
        total = getattr(args, "lr_total_steps", None)
        sched = LRSchedule({"constant": "const"}.get(kind, kind), warmup=getattr(args, "warmup_steps", 0),
                           total=int(getattr(args, "num_train_steps", 0)) if total is None else total, floor=getattr(args, "lr_floor", 0.0))
    elif getattr(args, "warmup_steps", 0) or getattr(args, "lr_floor", 0.0) or getattr(args, "lr_total_steps", None) is not None:
        raise ValueError("--warmup_steps / --lr_total_steps / --lr_floor need an --lr_schedule other than reference")
    groups = []
    frozen = [v.strip() for v in (getattr(args, "freeze", None) or "").split(",") if v.strip()]
    if getattr(args, "freeze", None) is not None and not frozen:
        raise ValueError("--freeze takes one or more name prefixes")
    if frozen:
        groups.append({"params": frozen, "frozen": True})
    # --no_decay_norm_bias splits every --lr_scale group and the remainder in two: the first match wins, so the undecayed half of a
    # prefix (its biases and norm vectors, by name) goes in front of the prefix itself
    split = getattr(args, "no_decay_norm_bias", False) and model is not None
    free = [n for n in no_decay_groups(model)[0]["params"] if not selector_matches(frozen, n)] if split and no_decay_groups(model) else []
    for pre, scale in parse_lr_scale(getattr(args, "lr_scale", None)):
        half = [n for n in free if selector_matches([pre], n)]
        if half:
            groups.append({"params": half, "lr_scale": scale, "weight_decay": 0.0})
            free = [n for n in free if n not in half]
        if not half or any(selector_matches([pre], n) and n not in half for n, _ in model.named_parameters()):
            groups.append({"params": [pre], "lr_scale": scale})      # (not for a prefix that holds undecayed vectors only)
    if free:
        groups.append({"params": free, "weight_decay": 0.0})
    out = {}
    if sched is not None:
        out["lr_schedule"] = sched
    if groups or getattr(args, "no_decay_norm_bias", False):
        out["param_groups"] = groups
    return out


def pcen_options(args):
    """None without --pcen / --pcen_fixed, else the PCEN keyword arguments of the command line (a Namespace built by hand may lack
    any of them); mel_bins, mean and std are the dataset's."""
    if not (getattr(args, "pcen", False) or getattr(args, "pcen_fixed", False)):
        return None
    return {"alpha": float(getattr(args, "pcen_alpha", 0.98)), "delta": float(getattr(args, "pcen_delta", 2.0)),
            "r": float(getattr(args, "pcen_r", 0.5)), "s": float(getattr(args, "pcen_s", 0.025)),
            "eps": float(getattr(args, "pcen_eps", 1e-6)), "gain": float(getattr(args, "pcen_gain", 1.0)),
            "trainable": not getattr(args, "pcen_fixed", False)}


def build_pcen(args, mel_bins, mean=None, std=None):
    """The layer of --pcen for a dataset whose features were z-scored with mean / std (scalars or per-bin; None: plain dB), or
    None without the option."""
    opts = pcen_options(args)
    if opts is None:
        return None
    import numpy as np
    from .models.frontend_layers import PCEN
    if mean is not None:
        mean = np.broadcast_to(np.asarray(mean, dtype=np.float32).reshape(-1), (mel_bins,)).copy()
        std = np.broadcast_to(np.asarray(std, dtype=np.float32).reshape(-1), (mel_bins,)).copy()
    return PCEN(mel_bins, input="db", mean=mean, std=std, **opts)


def parse_label_kinds(text):
    """'S:W:U' -> three shares (floats >= 0, not all 0) of strong, weak and unlabelled clips; None for None"""
    if text is None:
        return None
    parts = str(text).split(":")
    try:
        shares = tuple(float(v) for v in parts)
    except ValueError:
        shares = ()
    if len(parts) != 3 or len(shares) != 3 or not all(0.0 <= v < float("inf") for v in shares) or sum(shares) <= 0.0:
        raise ValueError(f"--label_kinds is S:W:U, three shares >= 0 that are not all 0 (e.g. 1:2:5), '{text}' given")
    return shares


def semi_options(args):
    """the train() keyword arguments of --mean_teacher and its parameters (a Namespace built by hand may lack any of them)"""
    if not getattr(args, "mean_teacher", False):
        return {}
    return {"mean_teacher": True, "ema_decay": float(getattr(args, "ema_decay", 0.999)),
            "consistency_weight": float(getattr(args, "consistency_weight", 2.0)),
            "consistency_rampup": int(getattr(args, "consistency_rampup", 0)), "eval_teacher": bool(getattr(args, "eval_teacher", False))}


def weak_options(args):
    """the FusedTrainer keyword arguments of --weak_labels / --weak_pooling / --weak_weight (a Namespace built by hand may lack
    any of them)"""
    labels = getattr(args, "weak_labels", "off")
    if labels == "off":
        return {}
    return {"weak_pooling": getattr(args, "weak_pooling", "linear"), "weak_weight": float(getattr(args, "weak_weight", 1.0)),
            "weak_only": labels == "only"}


def spec_augment_config(args):
    """The SpecAugmentConfig of --spec_augment and its parameters; None with the flag off (a Namespace built by hand may lack any
    of them)."""
    if not getattr(args, "spec_augment", False):
        return None
    from .dataset.spectogram.augment import SpecAugmentConfig
    p = build_augment_parser()
    g = {k: getattr(args, k, p.get_default(k)) for k in ("time_masks", "time_mask_frames", "freq_masks", "freq_mask_bins",
                                                         "time_shift", "mixup_prob", "mixup_alpha", "soft_labels", "filter_augment")}
    return SpecAugmentConfig(time_masks=g["time_masks"], time_mask_frames=g["time_mask_frames"], freq_masks=g["freq_masks"],
                             freq_mask_bins=g["freq_mask_bins"], time_shift=bool(g["time_shift"]), mixup_prob=g["mixup_prob"],
                             mixup_alpha=g["mixup_alpha"], label_mix="soft" if g["soft_labels"] else "max",
                             filter_prob=g["filter_augment"])


def ranking_eval_options(args):
    """train()'s ranking_eval of --eval_ranking / --eval_clip_pooling; None with the flag off (a Namespace built by hand may lack
    them)."""
    if not getattr(args, "eval_ranking", False):
        return None
    pooling = getattr(args, "eval_clip_pooling", None)
    return {} if pooling is None else {"clip_pooling": pooling}


def psds_eval_options(args, fps):
    """train()'s psds_eval of --eval_psds / --psds_scenario / --psds_median_window (seconds -> frames); None with the flag off (a
    Namespace built by hand may lack them)."""
    if not getattr(args, "eval_psds", False):
        return None
    from .utils.event_utils import seconds_to_window
    return {"scenario": int(getattr(args, "psds_scenario", 1)), "fps": float(fps),
            "median_window": seconds_to_window(getattr(args, "psds_median_window", 0.0), fps)}


def event_eval_options(args, fps):
    """The eval_events keyword arguments (frames) of --eval_events and its parameters (seconds); None with the flag off."""
    if not getattr(args, "eval_events", False):
        return None
    from .utils.event_utils import seconds_to_frames, seconds_to_window
    return {"threshold": 0.5, "low_threshold": None, "median_window": seconds_to_window(args.median_window, fps),
            "max_gap": seconds_to_frames(args.max_gap, fps), "min_len": max(1, seconds_to_frames(args.min_event, fps)),
            "seg_frames": max(1, seconds_to_frames(args.segment, fps)), "collar_frames": seconds_to_frames(args.collar, fps)}


def frames_per_second(args):
    """Model output frames per second of the chosen feature type."""
    if args.train_features.lower() == "spectogram":
        from .dataset.spectogram import spectogram_configs as cfgs
        return cfgs.REF_NATIVE.frames_per_second
    from .dataset.waveform import waveform_configs
    return waveform_configs.frames_per_second


def _val_descriptor(v):
    """argparse hands a string for an explicit --val_descriptor; the reference's float default selects
    a percentage split: accept '0.2' as a float as well (main.py:102)."""
    if isinstance(v, float):
        return v
    try:
        return float(v)
    except ValueError:
        return v


def get_spectogram_dataset_model_and_criterion(args, device):
    """main.py:10-46."""
    from .dataset.spectogram import spectogram_configs as cfgs
    from .dataset.spectogram.spectograms_dataset import (SpectogramDataset, preprocess_film_clap_data,
                                                         preprocess_tau_sed_data)
    from .dataset.synthetic import SyntheticSedDataset
    from .models.spectogram_models import Cnn_AvgPooling
    cfg = cfgs.REF_NATIVE
    n_mel = cfg.mel_bins if getattr(args, "mel_bins", None) is None else int(args.mel_bins)
    cfg = dataclasses.replace(cfg, mel_bins=n_mel)
    name = args.dataset_name.lower()
    if name == "synthetic":
        dataset = SyntheticSedDataset(n_train_crops=max(256, 4 * args.batch_size), crop=cfg.train_crop_size * 8,
                                      classes=cfg.classes_num, mel_bins=n_mel,
                                      label_kinds=parse_label_kinds(getattr(args, "label_kinds", None)))
        descriptor = cfg.cfg_descriptor
    else:
        if name == "tau":
            feats_dir, mean_std = preprocess_tau_sed_data(args.dataset_dir, fold_name="eval",
                                                          preprocess_mode=args.preprocess_mode,
                                                          force_preprocess=args.force_preprocess, cfg=cfg)
            descriptor = cfg.cfg_descriptor + "_C-doorslam"
        elif name == "filmclap":
            feats_dir, mean_std = preprocess_film_clap_data(args.dataset_dir, preprocessed_mode=args.preprocess_mode,
                                                            force_preprocess=args.force_preprocess, cfg=cfg)
            descriptor = cfg.cfg_descriptor + "_tm-0.33"
        else:
            raise ValueError(f"Only tau and filmclap datasets are supported, '{args.dataset_name}' given")
        dataset = SpectogramDataset(feats_dir, mean_std, augment_data=args.augment_data,
                                    balance_classes=args.balance_classes,
                                    val_descriptor=_val_descriptor(args.val_descriptor),
                                    preprocessed_mode=args.preprocess_mode, cfg=cfg, device=device,
                                    spec_augment=spec_augment_config(args))
    frontend = build_pcen(args, n_mel, getattr(dataset, "mean", None), getattr(dataset, "std", None))
    model_config, att = [(32, 2), (64, 2), (128, 2), (128, 1)], bool(getattr(args, "attention_head", False))
    if getattr(args, "self_attention", False):
        from .models.spectogram_models import Csa_AvgPooling
        model = Csa_AvgPooling(cfg.classes_num, model_config=model_config, sa_heads=int(args.sa_heads),
                               pos_encoding=not args.no_pos_encoding, mel_bins=n_mel, frontend=frontend, attention=att,
                               sa_layers=int(getattr(args, "sa_layers", 1)), sa_ffn=int(getattr(args, "sa_ffn", 0)),
                               sa_activation=getattr(args, "sa_activation", "relu"),
                               sa_conv_kernel=int(getattr(args, "sa_conv_kernel", 0)),
                               sa_dropout=float(getattr(args, "sa_dropout", 0.0)), sa_dropout_seed=getattr(args, "sa_dropout_seed", None),
                               sa_window=parse_sa_window(getattr(args, "sa_window", None)),
                               sa_rel_pos=parse_sa_rel_pos(getattr(args, "sa_rel_pos", None)),
                               sa_norm_first=bool(getattr(args, "sa_norm_first", False)), sa_macaron=bool(getattr(args, "sa_macaron", False)))
    else:
        model = Cnn_AvgPooling(cfg.classes_num, model_config=model_config, mel_bins=n_mel, frontend=frontend, attention=att)
    model.set_precision(args.precision)
    if args.ckpt != "":
        checkpoint = torch.load(args.ckpt, map_location=device)
        model.load_state_dict(checkpoint["model"])
    criterion = WeightedBCE(recall_factor=args.recall_priority, multi_frame=True)
    return dataset, model, criterion, f"{args.preprocess_mode}-{descriptor}"


def get_waveform_dataset_and_model(args, device):
    """main.py:49-73."""
    from .dataset.waveform.waveform_configs import cfg_descriptor, time_margin
    from .dataset.waveform.waveform_dataset import WaveformDataset, synthetic_waveform_task
    from .models.waveform_models import M5
    name = args.dataset_name.lower()
    waveforms = None
    if name == "synthetic":
        items, waveforms = synthetic_waveform_task()
        val_descriptor = "val_"
    elif name == "tau":
        from .dataset.dataset_utils import get_tau_sed_paths_and_labels, tau_audio_and_meta_dirs
        audio_dir, meta_dir = tau_audio_and_meta_dirs(f"{args.dataset_dir}/Tau_sound_events_2019", fold_name="eval")
        items, val_descriptor = get_tau_sed_paths_and_labels(audio_dir, meta_dir), _val_descriptor(args.val_descriptor)
    elif name == "filmclap":
        from .dataset.dataset_utils import get_film_clap_paths_and_labels
        items = get_film_clap_paths_and_labels(os.path.join(args.dataset_dir, "FilmClap"), time_margin)
        val_descriptor = _val_descriptor(args.val_descriptor)
    else:
        raise ValueError(f"Only tau and filmclap datasets are supported, '{args.dataset_name}' given")
    dataset = WaveformDataset(items, augment_data=args.augment_data, balance_classes=args.balance_classes,
                              val_descriptor=val_descriptor, waveforms=waveforms, device=device)
    model = M5(1, precision=args.precision)
    if args.ckpt != "":
        model.load_state_dict(torch.load(args.ckpt, map_location=device)["model"])
    criterion = WeightedBCE(recall_factor=args.recall_priority, multi_frame=False)
    return dataset, model, criterion, cfg_descriptor


def validate_args(args):
    """Combinations that cannot run, refused before any dataset or device work."""
    if args.train_features.lower() == "waveform" and args.precision not in ("bf16", "fp32"):
        raise ValueError(f"--train_features Waveform (the M5 model) supports --precision bf16 and fp32 only, "
                         f"'{args.precision}' given (f16x3 / bf16x3 exist for the spectrogram models)")
    if getattr(args, "clip_grad_norm", 0.0) < 0:
        raise ValueError(f"--clip_grad_norm must be >= 0 (0 = off), {args.clip_grad_norm} given")
    from .train import check_optimizer_options
    check_optimizer_options(**optimizer_options(args))
    from .train import resolve_param_groups
    sched = schedule_options(args)              # the schedule's own checks; the selectors meet the model's names in train()
    for g in sched.get("param_groups", []):     # each group's scale range, against a stand-in name
        resolve_param_groups(["_"], [dict(g, params=["_"], frozen=False)])
    for name in ("median_window", "max_gap", "min_event", "collar"):
        if getattr(args, name, 0.0) < 0:
            raise ValueError(f"--{name} must be >= 0 seconds, {getattr(args, name)} given")
    if getattr(args, "segment", 1.0) <= 0:
        raise ValueError(f"--segment must be > 0 seconds, {args.segment} given")
    for name in ("time_masks", "time_mask_frames", "freq_masks", "freq_mask_bins", "mixup_prob", "mixup_alpha", "filter_augment"):
        if not getattr(args, name, 0) >= 0:
            raise ValueError(f"--{name} must be >= 0, {getattr(args, name)} given")
    for name in ("mixup_prob", "filter_augment"):
        if not getattr(args, name, 0.0) <= 1:
            raise ValueError(f"--{name} is a probability in [0, 1], {getattr(args, name)} given")
    if getattr(args, "spec_augment", False):
        if args.train_features.lower() == "waveform":
            raise ValueError("--spec_augment works on log-mel features: it needs --train_features Spectogram "
                             "(there is no waveform-domain augmentation for the M5 model)")
        spec_augment_config(args)           # the config's own checks (at most 8 masks of a kind, alpha > 0)
    if getattr(args, "weak_labels", "off") not in ("off", "both", "only"):
        raise ValueError(f"--weak_labels is off, both or only, '{args.weak_labels}' given")
    if weak_options(args):
        if args.train_features.lower() == "waveform":
            raise ValueError("--weak_labels pools frame probabilities over time: it needs --train_features Spectogram "
                             "(the M5 model has no time axis in its output)")
        from .train import check_weak_options
        check_weak_options(**weak_options(args))
    att_head = bool(getattr(args, "attention_head", False))
    if att_head and args.train_features.lower() == "waveform":
        raise ValueError("--attention_head sits beside the frame-wise head: it needs --train_features Spectogram "
                         "(the M5 model has no time axis in its output)")
    if getattr(args, "self_attention", False):
        if args.train_features.lower() == "waveform":
            raise ValueError("--self_attention attends over the frames of the spectrogram models: it needs --train_features Spectogram")
        from .heads import SaConfig
        SaConfig(128, getattr(args, "sa_heads", 4), True, getattr(args, "sa_layers", 1), getattr(args, "sa_ffn", 0),
                 getattr(args, "sa_activation", "relu"), getattr(args, "sa_conv_kernel", 0), getattr(args, "sa_dropout", 0.0), None,
                 parse_sa_window(getattr(args, "sa_window", None)), parse_sa_rel_pos(getattr(args, "sa_rel_pos", None)),
                 bool(getattr(args, "sa_norm_first", False)), bool(getattr(args, "sa_macaron", False)))
    else:
        for name, default in (("sa_heads", 4), ("no_pos_encoding", False), ("sa_layers", 1), ("sa_ffn", 0), ("sa_activation", "relu"),
                              ("sa_conv_kernel", 0), ("sa_dropout", 0.0), ("sa_dropout_seed", None), ("sa_window", None), ("sa_rel_pos", None),
                              ("sa_norm_first", False), ("sa_macaron", False)):
            if getattr(args, name, default) != default:
                raise ValueError(f"--{name} configures the self-attention head: it needs --self_attention")
    for flag, value in (("--weak_pooling", weak_options(args).get("weak_pooling")), ("--eval_clip_pooling", getattr(args, "eval_clip_pooling", None))):
        if value == "att" and not att_head:
            raise ValueError(f"{flag} att pools with the attention head: it needs --attention_head")
    semi = semi_options(args)
    kinds = parse_label_kinds(getattr(args, "label_kinds", None))
    if getattr(args, "eval_teacher", False) and not semi:
        raise ValueError("--eval_teacher needs --mean_teacher")
    if semi or kinds is not None:
        if args.train_features.lower() == "waveform":
            raise ValueError("--mean_teacher and --label_kinds work on frame-wise outputs: they need --train_features Spectogram "
                             "(the M5 model has no time axis in its output)")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1 and semi:
            raise ValueError("--mean_teacher is the single-process path")
    if kinds is not None and args.dataset_name.lower() != "synthetic":
        raise ValueError("--label_kinds assigns kinds to the clips of --dataset_name synthetic only")
    if kinds is not None and getattr(args, "spec_augment", False) and getattr(args, "mixup_prob", 0.0) > 0:
        raise ValueError("--label_kinds with --spec_augment needs --mixup_prob 0: mixup mixes the features and labels of two clips but "
                         "not their kinds, so a strong clip mixed with a weak or unlabelled partner would keep wrong frame labels")
    if semi:
        from .train import check_semi_options
        check_semi_options(**{k: v for k, v in semi.items() if k != "eval_teacher"})
    pcen = pcen_options(args)
    if pcen is not None:
        if args.train_features.lower() == "waveform":
            raise ValueError("--pcen works on log-mel features: it needs --train_features Spectogram (the M5 model reads the raw "
                             "waveform)")
        if semi:
            raise ValueError("--pcen does not go with --mean_teacher")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise ValueError("--pcen is the single-process path (its backward takes the input gradient)")
        for name in ("alpha", "delta", "r", "eps", "gain"):
            if not (0.0 < pcen[name] < float("inf")):
                raise ValueError(f"--pcen_{name} must be finite and > 0, {pcen[name]} given")
        if not (0.0 < pcen["s"] < 1.0):
            raise ValueError(f"--pcen_s must lie in (0, 1), {pcen['s']} given")
    if getattr(args, "eval_clip_pooling", None) is not None:
        if not getattr(args, "eval_ranking", False):
            raise ValueError("--eval_clip_pooling needs --eval_ranking")
        if args.train_features.lower() == "waveform":
            raise ValueError("--eval_clip_pooling pools frame probabilities over time: it needs --train_features Spectogram "
                             "(the M5 model has no time axis in its output)")
        from .train import check_ranking_options
        check_ranking_options(args.eval_clip_pooling)
    if getattr(args, "psds_median_window", 0.0) < 0:
        raise ValueError(f"--psds_median_window must be >= 0 seconds, {args.psds_median_window} given")
    if getattr(args, "eval_psds", False):
        if args.train_features.lower() == "waveform":
            raise ValueError("--eval_psds scores events along time: it needs --train_features Spectogram "
                             "(the M5 model has no time axis in its output)")
        from .train import check_psds_options
        opts = psds_eval_options(args, frames_per_second(args))
        check_psds_options(opts["scenario"], None, opts["median_window"])


def optimizer_options(args):
    """the FusedTrainer keyword arguments of --weight_decay / --adamw / --no_amsgrad / --clip_grad_norm"""
    clip = float(getattr(args, "clip_grad_norm", 0.0))
    return {"weight_decay": float(getattr(args, "weight_decay", 0.0)), "decoupled_weight_decay": bool(getattr(args, "adamw", False)),
            "amsgrad": not getattr(args, "no_amsgrad", False), "max_grad_norm": clip if clip != 0.0 else None}


def synthetic_batch_augment(args):
    """train()'s batch_augment: the spectrogram datasets augment inside their own batch launch; the synthetic dataset hands plain
    tensors over, so --spec_augment is applied to its device batch.  None otherwise."""
    cfg = spec_augment_config(args)
    if cfg is None or args.dataset_name.lower() != "synthetic" or args.train_features.lower() != "spectogram":
        return None
    from .dataset.spectogram.augment import LogMelAugment
    return LogMelAugment(cfg)


def get_dataset_and_model(args, device):
    """main.py:77-83."""
    feats = args.train_features.lower()
    if feats == "spectogram":
        return get_spectogram_dataset_model_and_criterion(args, device)
    if feats == "waveform":
        return get_waveform_dataset_and_model(args, device)
    raise ValueError(f"training features can be raw waveform or spectogram only, '{args.train_features}' given")


def make_loader(dataset, batch_size):
    from .dataset.spectogram.spectograms_dataset import DeviceBatchLoader, SpectogramDataset
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if isinstance(dataset, SpectogramDataset):
        return DeviceBatchLoader(dataset, batch_size, rank=rank, world_size=world)
    from .dataset.waveform.waveform_dataset import WaveformBatchLoader, WaveformDataset
    if isinstance(dataset, WaveformDataset):
        return WaveformBatchLoader(dataset, batch_size, rank=rank, world_size=world,
                                   device=dataset.device or torch.device("cuda"))
    if world > 1:        # map-style dataset under data parallel: rank-sharded index ranges (a plain DataLoader would
        from .train import ShardedBatchLoader      # hand every rank the same batches)
        return ShardedBatchLoader(dataset, batch_size, rank=rank, world_size=world)
    from torch.utils.data import DataLoader
    return DataLoader(dataset, batch_size=batch_size, num_workers=0)


def main(argv=None):
    args = build_full_parser().parse_args(argv)
    validate_args(args)
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X visible: this build has no CPU training path")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    device = torch.device(f"cuda:{local_rank}" if world > 1 else args.device)
    torch.cuda.set_device(device)
    if world > 1:
        import torch.distributed as dist
        from .train import seed_all_ranks
        dist.init_process_group("nccl")          # RCCL
        # the dataset classes shuffle / split with the global host RNGs (like the reference's): every rank must draw the
        # same train/val split and the same start-index permutation before the index ranges are sharded by rank
        seed = seed_all_ranks(int(os.environ["SED_SEED"]) if "SED_SEED" in os.environ else None)
    dataset, model, criterion, cfg_descriptor = get_dataset_and_model(args, device)
    if world > 1:
        from .train import reseed_rank
        reseed_rank(seed, int(os.environ.get("RANK", "0")))       # augmentation draws differ per rank from here on (split / index table are already drawn)
    dataloader = make_loader(dataset, args.batch_size)
    model = model.to(device)
    model.model_description()
    train_name = f"{args.dataset_name}_cfg({cfg_descriptor}_b{args.batch_size}_lr{args.lr}_{args.train_tag}"
    if args.balance_classes:
        train_name += "_BC"
    if args.augment_data:
        train_name += "_AD"
    train(model, dataloader, criterion, num_steps=args.num_train_steps,
          outputs_dir=os.path.join(args.outputs_root, train_name), device=device, lr=args.lr,
          log_freq=args.log_freq, event_eval=event_eval_options(args, frames_per_second(args)),
          batch_augment=synthetic_batch_augment(args), ranking_eval=ranking_eval_options(args),
          psds_eval=psds_eval_options(args, frames_per_second(args)), **optimizer_options(args),
          **weak_options(args), **semi_options(args), **schedule_options(args, model))
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
