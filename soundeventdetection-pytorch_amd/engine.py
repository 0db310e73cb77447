"""Host-side orchestration of the MI355X kernels for the Cnn_AvgPooling training path.

One `CnnEngine` owns, per input shape, a *plan*: every activation / gradient / workspace buffer the
forward and backward passes need (allocated once through PyTorch-ROCm, laid out NHWC with channels
padded to 32 so that 288 GB of HBM holds whole 60 s batches with all pre-BN conv outputs resident
for the backward pass), and enqueues the libsed_hip.so kernels on the current HIP stream in the
order of

    Cnn_AvgPooling.forward / autograd backward      /root/reference/models/spectogram_models.py:185-202
    WeightedBCE.__call__                            /root/reference/utils/common.py:16-30
    Adam(amsgrad) step                              /root/reference/train.py:85,101-103

PyTorch is plumbing here (device memory, streams, nn.Parameter storage); all arithmetic of the path
happens in the HIP kernels.  There is no CPU fallback.
"""
from __future__ import annotations

import math
import os as _os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib as L
from .heads import BN_EPS, BN_MOMENTUM, FcHead, GruHead, SaConfig, SaHead, _stream, pad32


def num_pools_of(model_config) -> int:
    """spectogram_models.py:167-173 (starts at 1 regardless of block 0)."""
    n = 1
    for (_, p) in list(model_config)[1:]:
        if p == 2:
            n += 1
    return n


SPECIALISED_WIDTHS = (8, 16, 32, 64)     # line widths of the specialised conv kernels; others: csrc/sed_conv_anyw.hip
MAX_WIDTH = 256                          # SED_ANYW_MAX_W (include/sed_hip.h)


C1_ROUTES = ("z1", "c1_fused", "c1_stats")


def block0_route(lib, precision: str, mel_bins: int, channels: int, pool: int, generic_first: bool, environ=_os.environ) -> str:
    """How block 0 runs, decided once per plan (host only: no tensor, no device):
      'z1'        conv1's output z1 lives in memory like every other layer's (fp32, the split-operand modes, widths other than 64,
                  channel counts other than 32, generic_first, SED_C1_MODE=0)
      'c1_fused'  C1 mode -- z1 is never written, its consumers rebuild it from the 1-channel input (csrc/conv_common.h) -- with
                  conv2's weight gradient and gated data gradient in one launch (csrc/sed_bwd_fused_c1.hip), which derives conv1's
                  ReLU gate itself: the forward stores no mask
      'c1_stats'  C1 mode with the two-kernel backward (block-0 pool 1, SED_BWD_FUSED=0): sed_conv3x3_wgrad_fused_c1_u, then
                  sed_conv3x3_dgrad_c1_stats gated with the bit mask the forward stores
    A backward that needs g1 in memory (need_dx, eval mode) takes the 'c1_plain' launches in either C1 route: chosen per backward."""
    dt = L.SED_BF16 if precision == "bf16" else L.SED_F32
    if generic_first or environ.get("SED_C1_MODE", "1") == "0" or not lib.sed_c1_mode_supported(dt, mel_bins, channels, channels):
        return "z1"
    if precision == "bf16" and environ.get("SED_BWD_FUSED", "1") != "0" and \
            lib.sed_conv3x3_bwd_fused_c1_supported(dt, mel_bins, channels, pool):
        return "c1_fused"
    return "c1_stats"


def check_pooling(mode) -> int:
    """The SED_POOL_* id of a pooling name of the weak-label loss (host only)."""
    if mode not in L.POOL_MODES:
        raise ValueError(f"unknown pooling {mode!r}: choose one of {', '.join(L.POOL_MODES)}")
    return L.POOL_MODES[mode]


ATT_POOLING = "att"      # the learned pooling of the attention head (csrc/sed_attn.hip); not one of the parameter-free L.POOL_MODES


def check_clip_pooling(mode, model=None):
    """check_pooling() that also takes the attention pooling 'att', which needs a model (or engine) built with attention=True
    (host only).  Returns the mode's name."""
    if mode != ATT_POOLING:
        check_pooling(mode)
        return mode
    if model is not None and not getattr(model, "attention", False):
        raise ValueError("the 'att' pooling needs a model with the attention head (attention=True / --attention_head)")
    return mode


@dataclass
class _Layer:
    """One conv+BN layer of the plan."""
    cin: int
    cout: int
    cinp: int
    coutp: int
    H: int
    W: int
    z: torch.Tensor = None          # pre-BN conv output (NHWC, dtype)
    part: torch.Tensor = None       # stats partials
    scale: torch.Tensor = None
    shift: torch.Tensor = None
    mean: torch.Tensor = None
    invstd: torch.Tensor = None
    wpack: torch.Tensor = None      # forward operator
    wpack_t: torch.Tensor = None    # data-gradient operator
    dwpack: torch.Tensor = None
    coef: torch.Tensor = None       # [3][Cp] ca, cb, cc
    dt_mm: int = 0                  # dtype of the layer's GEMM-shaped launches (operator packing, forward, gradients)


@dataclass
class _Plan:
    B: int
    T: int
    F: int
    layers: List[List[_Layer]] = field(default_factory=list)   # [block][0|1]
    y: List[torch.Tensor] = field(default_factory=list)        # pooled block outputs
    dy: List[torch.Tensor] = field(default_factory=list)
    scratch: List[torch.Tensor] = field(default_factory=list)  # two dz-sized buffers
    m: torch.Tensor = None
    pre: torch.Tensor = None
    dpre: torch.Tensor = None
    loss: torch.Tensor = None
    loss_partial: torch.Tensor = None
    head_ws: torch.Tensor = None
    wgrad_ws: torch.Tensor = None
    c1_ws: torch.Tensor = None
    bwd_part: torch.Tensor = None
    t_out: int = 0
    w_out: int = 0
    x_ref: torch.Tensor = None      # the input of the last forward (first layer wgrad re-reads it)
    trained: bool = False
    gru: dict = None                # buffers of the recurrent head (head == 'gru')
    sa: dict = None                 # buffers of the self-attention head (head == 'sa')
    keep: bool = False              # the last forward ran with keep_for_grad (input-gradient / eval-mode backward possible)
    dx_in: torch.Tensor = None      # (B, 1, T, F) fp32 input gradient of the Cin = 1 model path (the last backward(need_dx=True))
    weak_ws: torch.Tensor = None    # workspace of the weak-label loss (csrc/sed_weak.hip), allocated at its first use
    clip_prob: torch.Tensor = None  # (B, K) clip probabilities of the last weak-label loss / clip_probs()
    semi_ws: torch.Tensor = None    # workspace of the label-kind / mean-teacher losses (csrc/sed_semi.hip), allocated at their first use
    consistency: torch.Tensor = None    # (2,) the frame and clip consistency terms of the last mean-teacher loss
    teacher_clip: torch.Tensor = None   # (B, K) the teacher's pooled clip probabilities
    att: torch.Tensor = None        # (B, t, K) attention logits of the last forward (engines with attention=True; csrc/sed_attn.hip)
    datt: torch.Tensor = None       # (B, t, K) their gradient, written by loss_and_grad(weak=("att", ...))
    att_pending: bool = False       # the last loss_and_grad on this plan produced datt: backward() takes the attention route
    datt_clip: torch.Tensor = None  # (B, t, K) datt of the clip consistency term of a mean teacher, added to datt
    att_ws: torch.Tensor = None     # workspace of sed_att_loss_fwd_bwd
    att_dcat: torch.Tensor = None   # (B*t, 2K) dpre | datt and
    att_wcat: torch.Tensor = None   # (2K, C) event_fc.weight; att_fc.weight: the operands of the two layers' backward through sed_head_bwd
    att_dw: torch.Tensor = None     # (2K, C) and
    att_db: torch.Tensor = None     # (2K,) its results, split into the four gradient tensors


class KernelTimer:
    """HIP-event timing of individual kernel launches on the stream they are enqueued on (torch's
    current stream).  Used by bench.py for the live per-kernel roofline numbers."""

    def __init__(self):
        self.records = []

    def launch(self, label, fn, args):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*args)
        e1.record()
        self.records.append((label, e0, e1))
        return rc

    def samples(self):
        """label -> [ms of every launch]; call after torch.cuda.synchronize()."""
        out = {}
        for label, e0, e1 in self.records:
            out.setdefault(label, []).append(e0.elapsed_time(e1))
        return out

    def summary(self, outlier_factor: float = 4.0):
        """label -> (launches, total_ms).  An event pair also spans any host stall between the two
        records (the GPU idles while Python is late with the launch), so launches longer than
        `outlier_factor` x the label's median are dropped from both numbers."""
        out = {}
        self.dropped = {}
        for label, ms in self.samples().items():
            srt = sorted(ms)
            med = srt[len(srt) // 2]
            keep = [v for v in ms if v <= outlier_factor * med] if len(ms) >= 3 else ms
            if len(keep) != len(ms):
                self.dropped[label] = len(ms) - len(keep)
            out[label] = (len(keep), sum(keep))
        return out


class OptimizerExtMixin:
    """grad_norm() and the extended optimizer step (weight decay, AdamW, amsgrad off, clip factor) for an engine with
    self.lib and self._k -- shared by CnnEngine and M5Engine.  Nothing here runs unless FusedTrainer was given an option."""

    def grad_norm(self, flat_g, partial, out, grad_scale: float = 1.0, max_norm: float = 0.0):
        """out[0] = ||flat_g * grad_scale||_2, out[1] = clip_grad_norm_'s factor (1 when max_norm <= 0).  partial: float64
        workspace of sed_grad_norm_nparts(n) elements; out: fp32 (2,).  Two launches, no sync."""
        self._k("sed_grad_norm", self.lib.sed_grad_norm, L.ptr(flat_g), flat_g.numel(), float(grad_scale), float(max_norm),
                L.ptr(partial), partial.numel(), L.ptr(out), _stream())

    def adam_step_ex(self, flat_p, flat_g, flat_m, flat_v, flat_vmax, lr: float, step: int, grad_scale: float = 1.0,
                     betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, decoupled: bool = False, coef=None):
        """flat_vmax None: amsgrad off; coef: device fp32 (1,) clip factor or None"""
        self._k("sed_adam_step_ex", self.lib.sed_adam_step_ex, L.ptr(flat_p), L.ptr(flat_g), L.ptr(flat_m), L.ptr(flat_v),
                L.ptr(flat_vmax), flat_p.numel(), float(lr), float(betas[0]), float(betas[1]), float(eps), int(step),
                float(grad_scale), float(weight_decay), int(bool(decoupled)), L.ptr(coef), _stream())

    def adam_step_ex_dev(self, flat_p, flat_g, flat_m, flat_v, flat_vmax, hyper, step_dev, grad_scale: float, lr_decay: float,
                         decay_every: int, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                         decoupled: bool = False, coef=None):
        """the same with the scalars in device memory (graph replay); hyper holds 4 floats (sed_hip.h)"""
        self._k("sed_adam_step_ex_dev", self.lib.sed_adam_step_ex_dev, L.ptr(flat_p), L.ptr(flat_g), L.ptr(flat_m), L.ptr(flat_v),
                L.ptr(flat_vmax), flat_p.numel(), L.ptr(hyper), L.ptr(step_dev), float(betas[0]), float(betas[1]), float(eps),
                float(grad_scale), float(lr_decay), int(decay_every), float(weight_decay), int(bool(decoupled)), L.ptr(coef),
                _stream())

    def grad_norm_groups(self, flat_g, tiles, groups, partial, out, grad_scale: float = 1.0, max_norm: float = 0.0):
        """grad_norm() over the tiles of the non-frozen groups (train.py's build_tiles makes the two tables); partial: float64
        workspace of one element per tile."""
        self._k("sed_grad_norm_groups", self.lib.sed_grad_norm_groups, L.ptr(flat_g), flat_g.numel(), L.ptr(tiles), tiles.shape[0],
                L.ptr(groups), float(grad_scale), float(max_norm), L.ptr(partial), L.ptr(out), _stream())

    def adam_groups_step(self, flat_p, flat_g, flat_m, flat_v, flat_vmax, tiles, groups, gh, hyper, step_dev, base_lr: float,
                         schedule, grad_scale: float = 1.0, betas=(0.9, 0.999), eps: float = 1e-8, decoupled: bool = False,
                         coef=None):
        """the grouped step (sed_hip.h): the step counter, the schedule's learning rate and every group's scalars stay in device
        memory, for eager and captured steps alike.  schedule: train.py's LRSchedule; gh: fp32 (NG, 4); hyper: fp32 (>= 3,)"""
        self._k("sed_adam_groups_step", self.lib.sed_adam_groups_step, L.ptr(flat_p), L.ptr(flat_g), L.ptr(flat_m), L.ptr(flat_v),
                L.ptr(flat_vmax), flat_p.numel(), L.ptr(tiles), tiles.shape[0], L.ptr(groups), groups.shape[0], L.ptr(gh),
                L.ptr(hyper), L.ptr(step_dev), float(base_lr), L.SCHED_KINDS[schedule.kind], int(schedule.warmup),
                int(schedule.total), int(schedule.every), float(schedule.gamma), float(schedule.floor), float(betas[0]),
                float(betas[1]), float(eps), float(grad_scale), int(bool(decoupled)), L.ptr(coef), _stream())


class CnnEngine(OptimizerExtMixin):
    def __init__(self, classes_num: int, model_config: Sequence[Tuple[int, int]], in_channels: int = 1,
                 precision: str = "bf16", head: str = "fc", gru_hidden: int = 256, generic_first: bool = False,
                 mel_bins: Optional[int] = None, attention: bool = False, sa_heads: int = 4, pos_encoding: bool = True,
                 sa_layers: int = 1, sa_ffn: int = 0, sa_activation: str = "relu", sa_conv_kernel: int = 0,
                 sa_dropout: float = 0.0, sa_dropout_seed: Optional[int] = None, sa_window=None, sa_rel_pos=None,
                 sa_norm_first: bool = False, sa_macaron: bool = False):
        """head: 'fc' (Cnn_AvgPooling: heads.FcHead), 'gru' (CRNN: heads.GruHead, gru_hidden units), 'sa' (Csa_AvgPooling: heads.SaHead;
        pos_encoding and the sa_* options are heads.SaConfig's fields, described and checked there, and belong to this head alone)
        or 'none' (a bare stack of ConvBlocks: forward() stops at the last pooled output plan.y[-1], backward() takes its gradient).
        attention: the attention pooling beside event_fc (heads._Head); False launches exactly what it always did.
        generic_first: the first conv runs through the general Cin >= 1 kernels on an NHWC copy of the (B, Cin, T, F) input and
        backward() also produces the input gradient plan.dx -- the standalone ConvBlock of spectogram_models.py:128-160; the model path
        keeps the dedicated Cin = 1 kernels (no input gradient exists there).  mel_bins: None -> every block's width must be one the
        specialised kernels are built for (8 / 16 / 32 / 64); an integer F -> inputs must be F wide (1 <= F <= 256) and blocks at other
        widths run the width-general kernels (csrc/sed_conv_anyw.hip; under 'f16x3' / 'bf16x3' those layers take the exact fp32 kernels)."""
        if precision not in ("bf16", "fp32", "bf16x3", "f16x3"):
            raise ValueError("precision must be 'bf16', 'fp32', 'f16x3' or 'bf16x3'")
        if head not in ("fc", "gru", "sa", "none"):
            raise ValueError("head must be 'fc' (Cnn_AvgPooling), 'gru' (CRNN), 'sa' (self-attention) or 'none' (ConvBlock stack)")
        if head == "gru" and (gru_hidden % 32 or not 32 <= gru_hidden <= 256):
            raise ValueError("gru_hidden must be a multiple of 32 in [32, 256]")
        self.head, self.Hd = head, int(gru_hidden)
        sa = (sa_heads, pos_encoding, sa_layers, sa_ffn, sa_activation, sa_conv_kernel, sa_dropout, sa_dropout_seed, sa_window, sa_rel_pos,
              sa_norm_first, sa_macaron)
        self.sa_config = SaConfig(int(list(model_config)[-1][0]), *sa) if head == "sa" else None
        for kw, v in (self.sa_config.keywords(every=True) if head == "sa" else SaConfig.absent(*sa)).items():
            setattr(self, kw, v)            # engine.sa_heads, engine.sa_dropout, ...: the checked options (the defaults without the head)
        self.attention = bool(attention)
        if self.attention and head == "none":
            raise ValueError("the attention head sits beside event_fc: it needs a model with a classification head")
        self.mel_bins = self.check_mel_bins(mel_bins)
        for (_, p) in model_config:
            if p not in (1, 2):
                raise ValueError("pool sizes must be 1 or 2")
        self.generic_first = bool(generic_first) or in_channels != 1
        self.cin0 = int(in_channels)
        if self.cin0 < 1:
            raise ValueError("in_channels must be >= 1")
        self.K = int(classes_num)
        self.cfg = [(int(c), int(p)) for (c, p) in model_config]
        self.precision = precision
        self.dt = L.SED_BF16 if precision == "bf16" else L.SED_F32
        self.tdtype = torch.bfloat16 if precision == "bf16" else torch.float32
        # "f16x3" / "bf16x3" (round 6): fp32 tensors like "fp32", but the GEMM-shaped launches (operator packing, forward / data gradient,
        # weight gradient) take dtype SED_F32H3 / SED_F32X3 -- every operand split into two 16-bit pieces, three 16-bit MFMAs per product
        # (csrc/sed_conv_x3.hip); every other kernel of the step is the fp32 mode's.  f16x3 (fp16 pieces, ~5e-7 per product) is the fast
        # reference-exact mode; bf16x3 (bf16 pieces, ~1e-5) holds the logit / decision gate but not the fp32 kernels' gradient noise level.
        self.dt_mm = {"bf16x3": L.SED_F32X3, "f16x3": L.SED_F32H3}.get(precision, self.dt)
        self.ratio = 2 ** num_pools_of(self.cfg)
        self._plans: Dict[Tuple[int, int, int, str], _Plan] = {}
        self.lib = L.lib()
        self.timer: Optional[KernelTimer] = None   # set to a KernelTimer to time every launch
        self._tag = ""
        # SyncBN (optional, data parallel): an object with .world and .all_reduce(tensor) (in-place SUM over the ranks, ordered
        # on the current stream).  Every BatchNorm then normalises with the statistics of the GLOBAL batch, like the
        # reference's single process does (spectogram_models.py:142-143 under train.py:95-97): the per-workgroup partial
        # sums are reduced to one row per rank, summed over the ranks, and finalized with count * world.
        self.bn_sync = None
        self._e_shift = 0                    # f16x3 pre-scale shift of the running backward (_grad_dtype; 0 outside the new backward kinds)
        self.head_impl = None               # the head's launches and buffers (heads.py); None for head == 'none'
        if head == "fc":
            self.head_impl = FcHead(self)
        elif head == "gru":
            self.head_impl = GruHead(self)
        elif head == "sa":
            self.head_impl = SaHead(self, self.sa_config)
            self.sa_dropout_seed = self.head_impl.seed      # (None resolved to torch.initial_seed())

    # names of the self-attention head that tools, tests and the models reach through the engine (heads.SaConfig / heads.SaHead)
    RELPOS_MAX_BUCKETS = SaConfig.RELPOS_MAX_BUCKETS
    check_sa_dropout, check_sa_window, check_sa_rel_pos, rel_pos_buckets, rel_pos_map, sa_layer_names, sa_conv_names, sa_rel_name = map(
        staticmethod, (SaConfig.check_dropout, SaConfig.check_window, SaConfig.check_rel_pos, SaConfig.rel_pos_buckets,
                       SaConfig.rel_pos_map, SaConfig.layer_names, SaConfig.conv_names, SaConfig.rel_name))
    drop_state = property(lambda self: self.head_impl.drop_state)
    _sa_layer_out = lambda self, ly: self.head_impl.layer_out(ly)     # (tests/test_gpu_sa_at_size.py reads a layer's output through it)

    def drop_state_words(self):
        return self.head_impl.drop_state_words()

    def set_drop_state(self, words) -> None:
        self.head_impl.set_drop_state(words)

    @staticmethod
    def check_mel_bins(mel_bins):
        """None or a positive int (the range against the kernels' limit is checked when a plan is built)"""
        if mel_bins is None:
            return None
        if isinstance(mel_bins, bool) or not isinstance(mel_bins, int) or mel_bins < 1:
            raise ValueError(f"mel_bins must be None or a positive integer, got {mel_bins!r}")
        return int(mel_bins)

    def _check_width(self, T: int, F: int) -> None:
        """plan-time width checks of a declared model (before any launch)"""
        if F != self.mel_bins:
            raise ValueError(f"input width {F} differs from the declared mel_bins={self.mel_bins}")
        if F > MAX_WIDTH:
            raise ValueError(f"mel_bins={F} unsupported: the width-general kernels cover 1..{MAX_WIDTH}")
        W = F
        for bi, (_, pool) in enumerate(self.cfg):
            if W < 1:
                raise ValueError(f"mel_bins={F}: the pooling stack leaves block {bi} with width {W}")
            W //= pool
        if W < 1:
            raise ValueError(f"mel_bins={F}: the pooling stack leaves the head with width {W}")

    def _grad_dtype(self, B: int, H: int, W: int) -> int:
        """dtype argument of a GEMM-shaped BACKWARD launch.  f16x3: fp16 pieces have five exponent bits and a loss gradient is ~1/(B*H*W)
        per element (mean-reduced BCE spread over the layer's pixels), so the streamed gradient operand is scaled by 2^e before the
        split, e = round(log2(B*H*W)) + 2 (the kernel scales the result back; bits 8..15 of dtype, include/sed_hip.h).  fp16's normal
        range leaves ~13 binades either side of that estimate."""
        if W not in SPECIALISED_WIDTHS:
            return self.dt           # width-general kernels: exact fp32 under the split-operand modes, no pre-scale exponent
        if self.dt_mm != L.SED_F32H3:
            return self.dt_mm
        e = max(-100, min(100, int(round(math.log2(max(1, B * H * W)))) + 2 - self._e_shift))
        return L.SED_F32H3 | ((e & 0xff) << 8)

    def _upstream_shift(self, p: _Plan, src: torch.Tensor, n_ref: int) -> int:
        """Binades between the upstream gradient's largest magnitude and what the mean-reduced loss gives at this shape
        (~1/n_ref per element): the f16x3 pre-scale of an input-gradient or eval-mode backward is shifted by it, so that a
        sum-reduced or one-hot upstream gradient does not saturate the fp16 pieces.  0 when the gradient is all zeros."""
        if getattr(p, "amax", None) is None:
            p.amax = torch.empty(1, dtype=torch.float32, device=src.device)
        self._k("sed_absmax", self.lib.sed_absmax, L.ptr(src), src.numel(), L.ptr(p.amax), _stream())
        a = float(p.amax.item())
        if not (a > 0.0 and math.isfinite(a)):
            return 0
        return int(round(math.log2(a * n_ref)))

    def _sync_row(self, part, nparts: int, n: int, out):
        """this rank's partial rows [nparts][n] -> out[n] = sum over rows and over ranks"""
        self._k("sed_sum_partials", self.lib.sed_sum_partials, L.ptr(part), nparts, n, L.ptr(out), _stream())
        self.bn_sync.all_reduce(out)
        return out

    def _k(self, name, fn, *args):
        if self.timer is not None:
            rc = self.timer.launch(f"{name}:{self._tag}" if self._tag else name, fn, args)
        else:
            rc = fn(*args)
        L.check(rc, name)

    # ------------------------------------------------------------------------------------------
    def plan(self, B: int, T: int, F: int, device) -> _Plan:
        key = (B, T, F, str(device))
        if key in self._plans:
            return self._plans[key]
        if self.mel_bins is not None:
            self._check_width(T, F)
        lib = self.lib
        dev = device
        p = _Plan(B, T, F)
        H, W, cin = T, F, self.cin0
        f32 = dict(dtype=torch.float32, device=dev)
        maxact = 0
        max_wgrad_ws = 0
        max_bwd_parts = 0
        for bi, (c, pool) in enumerate(self.cfg):
            if W not in SPECIALISED_WIDTHS and self.mel_bins is None:
                raise ValueError(f"mel width {W} at block {bi} unsupported (need 8/16/32/64)")
            if pool == 2 and (H < 2 or W < 2):
                raise ValueError("input too short for the pooling stack")
            blk = []
            for j, (ci, co) in enumerate(((cin, c), (c, c))):
                first = (bi == 0 and j == 0 and not self.generic_first)     # the dedicated Cin = 1 kernels
                cinp = 1 if first else pad32(ci)
                ly = _Layer(ci, co, cinp, pad32(co), H, W)
                # the split-operand modes cover the specialised widths only: the width-general kernels run those layers in exact fp32
                ly.dt_mm = self.dt_mm if W in SPECIALISED_WIDTHS else self.dt
                nparts = lib.sed_conv_c1_nparts(B, H, W) if first else lib.sed_conv_nparts(B, H, W)
                ly.z = torch.empty((B, H, W, ly.coutp), dtype=self.tdtype, device=dev)
                ly.part = torch.empty((nparts, 2, ly.coutp), **f32)
                ly.scale = torch.empty(ly.coutp, **f32)
                ly.shift = torch.empty(ly.coutp, **f32)
                ly.mean = torch.empty(ly.coutp, **f32)
                ly.invstd = torch.empty(ly.coutp, **f32)
                ly.coef = torch.empty((3, ly.coutp), **f32)
                if not first:
                    ly.wpack = torch.empty(9 * ly.cinp * ly.coutp, dtype=self.tdtype, device=dev)
                    ly.dwpack = torch.empty(9 * ly.cinp * ly.coutp, **f32)
                    max_wgrad_ws = max(max_wgrad_ws, lib.sed_conv_wgrad_ws_floats(B, H, W, ly.cinp, ly.coutp))
                    ly.wpack_t = torch.empty(9 * ly.cinp * ly.coutp, dtype=self.tdtype, device=dev)
                else:
                    ly.dwpack = torch.empty(9 * ly.coutp, **f32)
                maxact = max(maxact, B * H * W * ly.coutp)
                max_bwd_parts = max(max_bwd_parts, lib.sed_pool_bwd_nparts(B, H, W, ly.coutp) * 2 * ly.coutp,
                                    nparts * 2 * ly.coutp, lib.sed_conv_nparts(B, H, W) * 2 * pad32(ci))
                blk.append(ly)
            p.layers.append(blk)
            Ho, Wo = H // pool, W // pool
            p.y.append(torch.empty((B, Ho, Wo, pad32(c)), dtype=self.tdtype, device=dev))
            p.dy.append(torch.empty((B, Ho, Wo, pad32(c)), dtype=self.tdtype, device=dev))
            H, W, cin = Ho, Wo, c
        if H < 1:
            raise ValueError("input too short for the pooling stack")
        p.t_out, p.w_out = H, W
        p.m = torch.empty((B, H, pad32(cin)), **f32)
        p.pre = torch.empty((B, H, self.K), **f32)
        p.dpre = torch.empty((B, H, self.K), **f32)
        p.loss = torch.zeros(1, **f32)
        p.loss_partial = torch.empty(max(1, (B * H * self.ratio * self.K + 255) // 256), **f32)
        if self.head_impl is not None:
            self.head_impl.plan(p, B, H, cin, dev)
        p.wgrad_ws = torch.empty(max(1, max_wgrad_ws), **f32)
        l0 = p.layers[0][0]
        p.c1_ws = torch.empty((lib.sed_conv_c1_nparts(B, T, F), 9, l0.coutp), **f32)
        p.c1_gram = torch.empty((lib.sed_conv_c1_gram_nparts(B, T, F), 54), **f32)
        # "C1 mode": block 0 without conv1's output in memory (csrc/conv_common.h): conv2's forward and weight gradient
        # rebuild relu(bn1(conv1(x))) on the matrix pipe from the 1-channel input, the data gradient gates with conv1's ReLU
        # decisions, BN1's statistics and backward come from Gram statistics of the input patches.
        # Removes 4 of block 0's 12.75 HBM passes (6.41 -> 6.2 ms/step); SED_C1_MODE=0 restores the z1 dataflow.
        p.c1_route = block0_route(lib, self.precision, F, self.cfg[0][0], self.cfg[0][1], self.generic_first)
        p.c1_mode = p.c1_route != "z1"
        if self.generic_first:
            c0p = pad32(self.cin0)
            p.x_nhwc = torch.zeros((B, T, F, c0p), dtype=self.tdtype, device=dev)
            p.dx = torch.empty((B, T, F, c0p), dtype=self.tdtype, device=dev)
        p.c1_A = torch.empty((9, l0.coutp), **f32)
        # block 0's gated data gradient in C1 mode: per-workgroup partials and sums of [A (9 taps); sum g]
        p.c1_a10_part = torch.empty((lib.sed_conv_dgrad_c1_nparts(), 10, 32), **f32)
        p.c1_a10 = torch.empty((10, 32), **f32)
        # conv1's ReLU decisions as a bit mask, stored by the training forward for the one route whose backward reads it
        p.c1_mask = torch.empty((B, T, F, 2), dtype=torch.int16, device=dev) if p.c1_route == "c1_stats" else None
        # Pool + ReLU + BN2 backward statistics from POOLED tensors (include/sed_hip.h, sed_conv3x3_dgrad_poolstats): a 2x2-pooled
        # block whose output gradient comes from the next block's conv1 data gradient gets its statistics in that kernel's
        # epilogue (forward: active-pixel counts beside the pooled activation) -- no separate pass over z2.  SED_POOL_STATS=z
        # keeps the per-pixel pass everywhere.
        nb = len(self.cfg)
        p.pool_fused, p.pool_cnt, p.pool_nparts = [False] * nb, [None] * nb, [0] * nb
        if _os.environ.get("SED_POOL_STATS", "p") != "z":
            for bi in range(nb - 1):
                l2, n1 = p.layers[bi][1], p.layers[bi + 1][0]
                if self.cfg[bi][1] == 2 and lib.sed_dgrad_poolstats_supported(self.dt, n1.W, n1.coutp, n1.cinp) and n1.cinp == l2.coutp:
                    p.pool_fused[bi] = True
                    p.pool_cnt[bi] = torch.empty((B, n1.H, n1.W, l2.coutp), dtype=torch.uint8, device=dev)
                    p.pool_nparts[bi] = lib.sed_conv_nparts(B, n1.H, n1.W)       # (the conditional per-pixel pass adapts its grid)
                    max_bwd_parts = max(max_bwd_parts, p.pool_nparts[bi] * 2 * l2.coutp)
        # Fused weight + data gradient (csrc/sed_bwd_fused.hip): dz of a layer lives only in LDS.  SED_BWD_FUSED=0 restores the
        # two-kernel backward (weight gradient writes dz, the data-gradient launch reads it back).
        p.bwd_fused = [[False, False] for _ in range(nb)]
        if self.precision == "bf16" and _os.environ.get("SED_BWD_FUSED", "1") != "0":
            for bi in range(nb):
                l1, l2 = p.layers[bi]
                if not (bi == 0 and not self.generic_first):
                    epi1 = L.EPI_POOLSTATS if (bi > 0 and p.pool_fused[bi - 1]) else L.EPI_STORE
                    if bi > 0 or self.generic_first:
                        p.bwd_fused[bi][0] = bool(lib.sed_conv3x3_bwd_fused_supported(self.dt, l1.W, l1.cinp, l1.coutp, L.DZ_BN, L.PRO_NONE, epi1))
                # conv2's fused form produces dz from the block's (pooled) output gradient: the library answers per pooling size
                # (W = 32: one dy item per 2x2 window, pool 2 only -- pool-1 blocks keep the two-kernel backward)
                if not (p.c1_mode and bi == 0):
                    p.bwd_fused[bi][1] = bool(lib.sed_conv3x3_bwd_fused_supported_pool(self.dt, l2.W, l2.cinp, l2.coutp, L.DZ_POOL, L.PRO_BNRELU,
                                                                                        L.EPI_RELUBWD, self.cfg[bi][1]))
        # block 0's conv1 backward tail in C1 mode (sed_c1_bwd_tail) takes the Gram statistics the forward's finalize reduced
        p.c1_gsum = torch.empty(54, dtype=torch.float64, device=dev)
        p.pool_flag = torch.zeros(nb, dtype=torch.int32, device=dev)
        p.bwd_part = torch.empty(max(1, max_bwd_parts), **f32)
        maxc = max(ly.coutp for blk in p.layers for ly in blk)
        p.sync_row = torch.empty(2 * maxc, **f32)          # SyncBN: one all-reduced row of (sum, sum-of-squares) / backward sums
        p.sync_gram = torch.empty(54, **f32)
        p.sync_a10 = torch.empty((10, 32), **f32)
        p.scratch = [torch.empty(maxact, dtype=self.tdtype, device=dev) for _ in range(2)]
        self._plans[key] = p
        return p

    # ------------------------------------------------------------------------------------------
    def _bn_names(self, bi, j):
        pre = f"conv_blocks.{bi}.bn{j + 1}."
        return pre + "weight", pre + "bias", pre + "running_mean", pre + "running_var"

    def _pack_weights(self, p: _Plan, P: Dict[str, torch.Tensor], training: bool) -> None:
        """Every conv layer's MFMA operand images in ONE launch: the forward operators and, for a train step, the
        data-gradient operators (the weights do not change between a step's forward and backward).  The descriptor table
        lives on the device and is rebuilt only when a parameter tensor moved."""
        ents = []
        for bi in range(len(self.cfg)):
            for j in range(2):
                if bi == 0 and j == 0 and not self.generic_first:
                    continue
                ly = p.layers[bi][j]
                w = P[f"conv_blocks.{bi}.conv{j + 1}.weight"]
                ents.append((ly.dt_mm, (w.data_ptr(), ly.wpack.data_ptr(), ly.cout, ly.cin, ly.coutp, ly.cinp, 0)))
                if training:
                    ents.append((ly.dt_mm, (w.data_ptr(), ly.wpack_t.data_ptr(), ly.cout, ly.cin, ly.cinp, ly.coutp, 1)))
        cache = getattr(p, "pack_tables", None)
        if cache is None:
            cache = p.pack_tables = {}
        # one launch per operator dtype (a single one unless a split-operand model has layers at non-specialised widths)
        for dtm in sorted({d for d, _ in ents}, key=lambda d: d != self.dt_mm):
            key = (dtm,) + tuple(e for d, e in ents if d == dtm)
            if key not in cache:
                rows, blk = [], 0
                for (wp, op, co, ci, pop, pip_, tf) in key[1:]:
                    rows.append([wp, op, co, ci, pop, pip_, tf, blk])
                    blk += (pip_ * 9 * pop + 1023) // 1024
                cache[key] = (torch.tensor(rows, dtype=torch.int64).to(p.layers[0][0].z.device), len(rows), blk)
            desc, n, blocks = cache[key]
            if n:
                self._k("sed_pack_conv_weights_batch", self.lib.sed_pack_conv_weights_batch, dtm, L.ptr(desc), n, blocks, _stream())

    def forward(self, x: torch.Tensor, P: Dict[str, torch.Tensor], training: bool,
                feat_mean: Optional[torch.Tensor] = None, feat_std: Optional[torch.Tensor] = None,
                update_running_stats: bool = True, keep_for_grad: bool = False) -> _Plan:
        """x: (B, 1, T, F) float32 cuda contiguous.  P: name -> fp32 cuda tensors (state_dict names).
        Leaves pre-interpolation logits in plan.pre (B, t, K).  keep_for_grad: the forward keeps what an input-gradient
        backward (training) or an eval-mode backward needs beyond today's train step -- in C1 mode conv1's ReLU mask, under
        the recurrent head the saved gates of an eval forward.  Outputs are the same bits either way; False keeps today's launches."""
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == self.cin0):
            raise ValueError(f"expected a float32 CUDA tensor of shape (B, {self.cin0}, T, F)")
        x = x.contiguous()
        B, _, T, F = x.shape
        p = self.plan(B, T, F, x.device)
        lib, dt, st = self.lib, self.dt, _stream()
        p.x_ref = x
        p.trained = training
        p.keep = bool(keep_for_grad)
        p.att_pending = False
        keep_mask = None
        if p.keep and p.c1_mode:
            if p.c1_mask is None and getattr(p, "c1_mask_keep", None) is None:
                p.c1_mask_keep = torch.empty((B, T, F, 2), dtype=torch.int16, device=x.device)
            keep_mask = p.c1_mask if p.c1_mask is not None else p.c1_mask_keep
        p.feat_mean, p.feat_std = feat_mean, feat_std
        prev = None
        if self.generic_first:
            if feat_mean is not None or feat_std is not None:
                raise ValueError("the z-score on load belongs to the Cin = 1 model path")
            self._k("sed_nchw_to_nhwc", lib.sed_nchw_to_nhwc, dt, L.ptr(x), L.ptr(p.x_nhwc), B, self.cin0, T, F,
                    p.x_nhwc.shape[3], st)
            prev = p.x_nhwc
        self._tag = ""
        self._pack_weights(p, P, training or p.keep)      # (a kept eval forward packs the data-gradient operators too)
        for bi, (c, pool) in enumerate(self.cfg):
            for j in range(2):
                ly = p.layers[bi][j]
                w = P[f"conv_blocks.{bi}.conv{j + 1}.weight"]
                gname, bname, rmname, rvname = self._bn_names(bi, j)
                first = (bi == 0 and j == 0 and not self.generic_first)
                self._tag = f"fwd b{bi}c{j + 1} {ly.cin}->{ly.cout} H{ly.H} W{ly.W}"
                part = ly.part if training else None
                c1m = p.c1_mode and bi == 0
                if first and c1m:
                    pass        # z1 is never materialised: its consumers recompute it from x (BN1 statistics: Gram, below)
                elif first:
                    self._k("sed_conv3x3_c1_fwd", self.lib.sed_conv3x3_c1_fwd, dt, L.ptr(x), L.ptr(feat_mean), L.ptr(feat_std), L.ptr(w),
                                                   L.ptr(ly.z), L.ptr(part), B, ly.H, ly.W, ly.cout, ly.coutp, st)
                elif c1m and j == 1:
                    l1 = p.layers[bi][0]
                    # (the kernel writes conv1's ReLU mask in its statistics epilogue: an eval forward kept for a backward takes that
                    #  epilogue with unused statistics; z2 is stored the same either way)
                    mask = (L.ptr(p.c1_mask) if (training and p.c1_mask is not None) else None) if keep_mask is None else L.ptr(keep_mask)
                    self._k("sed_conv3x3_fwd_c1", self.lib.sed_conv3x3_fwd_c1, dt, L.EPI_STATS if (training or keep_mask is not None) else L.EPI_STORE,
                            L.ptr(x), L.ptr(feat_mean), L.ptr(feat_std), L.ptr(P["conv_blocks.0.conv1.weight"]), L.ptr(l1.scale), L.ptr(l1.shift),
                            L.ptr(ly.wpack), L.ptr(ly.z), L.ptr(ly.part if keep_mask is not None else part), mask, B, ly.H, ly.W,
                            ly.coutp, st)
                else:
                    if j == 0:
                        src, pro, ps, ph = prev, L.PRO_NONE, None, None
                    else:
                        l1 = p.layers[bi][0]
                        src, pro, ps, ph = l1.z, L.PRO_BNRELU, l1.scale, l1.shift
                    self._k("sed_conv3x3_fwd", self.lib.sed_conv3x3_fwd, ly.dt_mm, pro, L.EPI_STATS if training else L.EPI_STORE, L.ptr(src),
                                                L.ptr(ps), L.ptr(ph), L.ptr(ly.wpack), L.ptr(ly.z), None, None, None,
                                                None, None, L.ptr(part), B, ly.H, ly.W, ly.cinp, ly.coutp, st)
                if training and first and c1m:
                    rm = P[rmname] if update_running_stats else None
                    rv = P[rvname] if update_running_stats else None
                    self._k("sed_conv3x3_c1_gram", self.lib.sed_conv3x3_c1_gram, L.ptr(x), L.ptr(feat_mean), L.ptr(feat_std),
                            L.ptr(p.c1_gram), B, ly.H, ly.W, st)
                    gram, ng, cnt = p.c1_gram, p.c1_gram.shape[0], float(B * ly.H * ly.W)
                    if self.bn_sync is not None:
                        gram, ng, cnt = self._sync_row(p.c1_gram, ng, 54, p.sync_gram), 1, cnt * self.bn_sync.world
                    if self.bn_sync is None:      # (the backward's tail kernel reads the reduced Gram statistics: p.c1_gsum)
                        self._k("sed_bn_train_finalize_c1", self.lib.sed_bn_train_finalize_c1_g, L.ptr(gram), ng,
                                cnt, L.ptr(w), L.ptr(P[gname]), L.ptr(P[bname]), L.ptr(rm), L.ptr(rv), BN_MOMENTUM, BN_EPS,
                                L.ptr(ly.scale), L.ptr(ly.shift), L.ptr(ly.mean), L.ptr(ly.invstd), ly.cout, ly.coutp, L.ptr(p.c1_gsum), st)
                        continue
                    self._k("sed_bn_train_finalize_c1", self.lib.sed_bn_train_finalize_c1, L.ptr(gram), ng,
                            cnt, L.ptr(w), L.ptr(P[gname]), L.ptr(P[bname]), L.ptr(rm), L.ptr(rv), BN_MOMENTUM, BN_EPS,
                            L.ptr(ly.scale), L.ptr(ly.shift), L.ptr(ly.mean), L.ptr(ly.invstd), ly.cout, ly.coutp, st)
                    continue
                if training:
                    rm = P[rmname] if update_running_stats else None
                    rv = P[rvname] if update_running_stats else None
                    part, npart, cnt = ly.part, ly.part.shape[0], float(B * ly.H * ly.W)
                    if self.bn_sync is not None:
                        part, npart, cnt = self._sync_row(ly.part, npart, 2 * ly.coutp, p.sync_row), 1, cnt * self.bn_sync.world
                    self._k("sed_bn_train_finalize", self.lib.sed_bn_train_finalize, L.ptr(part), npart, cnt,
                                                      L.ptr(P[gname]), L.ptr(P[bname]), L.ptr(rm), L.ptr(rv),
                                                      BN_MOMENTUM, BN_EPS, L.ptr(ly.scale), L.ptr(ly.shift),
                                                      L.ptr(ly.mean), L.ptr(ly.invstd), ly.cout, ly.coutp, st)
                else:
                    self._k("sed_bn_eval_coeffs", self.lib.sed_bn_eval_coeffs, L.ptr(P[gname]), L.ptr(P[bname]), L.ptr(P[rmname]),
                                                   L.ptr(P[rvname]), BN_EPS, L.ptr(ly.scale), L.ptr(ly.shift),
                                                   ly.cout, ly.coutp, st)
            l2 = p.layers[bi][1]
            self._tag = f"fwd b{bi}"
            if training and p.pool_fused[bi]:
                self._k("sed_bn_relu_pool_cnt_fwd", self.lib.sed_bn_relu_pool_cnt_fwd, dt, L.ptr(l2.z), L.ptr(l2.scale), L.ptr(l2.shift),
                        L.ptr(p.y[bi]), L.ptr(p.pool_cnt[bi]), B, l2.H, l2.W, l2.coutp, st)
            else:
                self._k("sed_bn_relu_pool_fwd", self.lib.sed_bn_relu_pool_fwd, dt, L.ptr(l2.z), L.ptr(l2.scale), L.ptr(l2.shift), L.ptr(p.y[bi]), B,
                                                 l2.H, l2.W, l2.coutp, pool, st)
            prev = p.y[bi]
        self._tag = ""
        if self.head_impl is not None:
            self.head_impl.forward(p, P, prev, training or p.keep, training, update_running_stats)
        return p

    def interpolate(self, p: _Plan) -> torch.Tensor:
        out = torch.empty((p.B, p.t_out * self.ratio, self.K), dtype=torch.float32, device=p.pre.device)
        self._k("sed_interpolate", self.lib.sed_interpolate, L.ptr(p.pre), L.ptr(out), p.B, p.t_out, self.K, self.ratio, _stream())
        return out

    def loss_and_grad(self, p: _Plan, target: torch.Tensor, recall_factor: float, need_grad: bool = True,
                      grad_scale: float = 1.0, weak=None, kind=None, teacher_pre=None, consistency=None,
                      teacher_att=None) -> torch.Tensor:
        """WeightedBCE on the virtually interpolated logits; fills plan.dpre; returns plan.loss (1,).
        weak: None, or (mode, weight, only) -- the pooled clip-level loss of csrc/sed_weak.hip, mode one of max / mean / linear /
        exp, scaled by weight -- or "att" on an engine with attention=True, the attention pooling of csrc/sed_attn.hip, which
        also fills plan.datt; backward() then takes both linear layers (with a teacher, teacher_att is its plan.att, and the clip
        consistency term pools the teacher with its own attention).
        only=False: the strong kernel runs as always, then the weak loss of the same (B, T, K) target is
        added on top of plan.loss and plan.dpre.  only=True: the weak loss alone; the target may then be (B, K) clip labels.
        kind: None, or an integer (B,) device tensor, 0 = strongly labelled, 1 = weakly labelled, 2 = unlabelled: the strong term
        then takes the clips with kind == 0 (sed_bce_sel_fwd_bwd) and the weak term those with kind <= 1 (sed_weak_bce_fwd_bwd_ex);
        the clip label of the weak term is the maximum over the clip's target frames as always, so a weak clip's target carries
        its clip label on every frame.  Each term is a mean over its own clips.
        teacher_pre: None, or the (B, t, K) logits a mean teacher gave for the same clips; consistency is then the weight of the
        consistency terms over all clips, added on top: the frame MSE (csrc/sed_semi.hip) and, with a weak pooling, the MSE of
        the pooled clip probabilities.  Their values land in plan.consistency (2,): frame, clip.
        All of them None launches exactly what it always did."""
        p.att_pending = False       # set below only where datt is written: backward() follows the LAST loss on this plan
        if weak is None and kind is None and teacher_pre is None:
            if not (target.is_cuda and target.dtype == torch.float32 and target.dim() == 3):
                raise ValueError("target must be a float32 CUDA tensor (B, T, K)")
            target = target.contiguous()
            self._strong_loss(p, target, recall_factor, need_grad, grad_scale)
            return p.loss
        if self.head == "none":
            raise ValueError("the weak-label loss needs a model with a classification head" if weak is not None else
                             "label kinds and the mean teacher need a model with a classification head")
        mode, weight, only = weak if weak is not None else (None, 0.0, False)
        att = weak is not None and mode == ATT_POOLING
        if att and not self.attention:
            raise ValueError("the 'att' pooling needs a model with the attention head (attention=True)")
        mode_id = check_pooling(mode) if weak is not None and not att else None
        if not (target.is_cuda and target.dtype == torch.float32 and target.dim() in ((2, 3) if only else (3,))):
            raise ValueError("target must be a float32 CUDA tensor (B, T, K) or, for the weak loss alone, (B, K) clip labels")
        if target.shape[0] != p.B or target.shape[-1] != self.K:
            raise ValueError(f"target {tuple(target.shape)} does not fit {p.B} clips of {self.K} classes")
        target = target.contiguous()
        sel_strong = sel_weak = None
        if kind is not None:
            if not (kind.is_cuda and kind.dim() == 1 and kind.shape[0] == p.B and not kind.dtype.is_floating_point
                    and kind.dtype != torch.bool):
                raise ValueError(f"kind must be an integer CUDA tensor ({p.B},): 0 strong, 1 weak, 2 unlabelled")
            sel_strong, sel_weak = (kind == 0).to(torch.uint8), (kind <= 1).to(torch.uint8)
        if teacher_pre is not None:
            if not (teacher_pre.is_cuda and teacher_pre.dtype == torch.float32 and teacher_pre.shape == p.pre.shape
                    and teacher_pre.is_contiguous()):
                raise ValueError(f"teacher_pre must be a contiguous float32 CUDA tensor {tuple(p.pre.shape)}")
            if consistency is None or not (0.0 <= float(consistency) < float("inf")):
                raise ValueError(f"teacher_pre needs a finite consistency weight >= 0 (got {consistency!r})")
            if att and not (teacher_att is not None and teacher_att.is_cuda and teacher_att.dtype == torch.float32
                            and teacher_att.shape == p.pre.shape and teacher_att.is_contiguous()):
                raise ValueError("the 'att' pooling with a teacher needs teacher_att, a contiguous float32 CUDA tensor "
                                 f"{tuple(p.pre.shape)}")
        if kind is not None or teacher_pre is not None:
            self._semi_bufs(p)
        dpre = L.ptr(p.dpre) if need_grad else None
        frames = target.shape[1] if target.dim() == 3 else 0
        Tt = frames if frames else p.t_out * self.ratio
        dims = (p.B, p.t_out, self.K, self.ratio, Tt)
        if not only:
            if kind is None:
                self._strong_loss(p, target, recall_factor, need_grad, grad_scale)
            else:
                self._k("sed_bce_sel_fwd_bwd", self.lib.sed_bce_sel_fwd_bwd, L.ptr(p.pre), L.ptr(target), L.ptr(sel_strong), L.ptr(p.loss),
                        dpre, 0, *dims, float(recall_factor), 1.0, float(grad_scale), L.ptr(p.semi_ws), _stream())
        datt = L.ptr(p.datt) if need_grad and att else None
        if att:
            self._k("sed_att_loss_fwd_bwd", self.lib.sed_att_loss_fwd_bwd, L.ptr(p.pre), L.ptr(p.att), L.ptr(target), frames,
                    L.ptr(sel_weak), L.CRIT_BCE, L.ptr(p.clip_prob), L.ptr(p.loss), dpre, datt, 0 if only else 1, *dims,
                    float(recall_factor), float(weight), float(grad_scale), L.ptr(p.att_ws), _stream())
            p.att_pending = bool(need_grad)
        elif weak is not None:
            self._weak_bufs(p)
            if kind is None:
                self._k("sed_weak_bce_fwd_bwd", self.lib.sed_weak_bce_fwd_bwd, L.ptr(p.pre), L.ptr(target), frames, L.ptr(p.clip_prob),
                        L.ptr(p.loss), dpre, 0 if only else 1, *dims, mode_id, float(recall_factor), float(weight), float(grad_scale),
                        L.ptr(p.weak_ws), _stream())
            else:
                self._k("sed_weak_bce_fwd_bwd_ex", self.lib.sed_weak_bce_fwd_bwd_ex, L.ptr(p.pre), L.ptr(target), frames,
                        L.ptr(sel_weak), L.CRIT_BCE, L.ptr(p.clip_prob), L.ptr(p.loss), dpre, 0 if only else 1, *dims, mode_id,
                        float(recall_factor), float(weight), float(grad_scale), L.ptr(p.weak_ws), _stream())
        if teacher_pre is None:
            return p.loss
        cw = float(consistency)
        # each term into its own zeroed cell (0 + term is the term), the gradient on top of plan.dpre; then one add per term
        p.consistency.zero_()
        self._k("sed_frame_mse_fwd_bwd", self.lib.sed_frame_mse_fwd_bwd, L.ptr(p.pre), L.ptr(teacher_pre), None, L.ptr(p.consistency),
                dpre, 1, *dims, cw, float(grad_scale), L.ptr(p.semi_ws), _stream())
        p.loss.add_(p.consistency[0:1])
        if att:
            # the teacher's clip probabilities pooled with its own attention; the student's MSE term against them
            self._k("sed_att_pool_fwd", self.lib.sed_att_pool_fwd, L.ptr(teacher_pre), L.ptr(teacher_att), L.ptr(p.teacher_clip), *dims,
                    _stream())
            self._k("sed_att_loss_fwd_bwd", self.lib.sed_att_loss_fwd_bwd, L.ptr(p.pre), L.ptr(p.att), L.ptr(p.teacher_clip), 0, None,
                    L.CRIT_MSE, L.ptr(p.clip_prob), L.ptr(p.consistency[1:2]), dpre, L.ptr(p.datt_clip) if need_grad else None, 1,
                    *dims, float(recall_factor), cw, float(grad_scale), L.ptr(p.att_ws), _stream())
            if need_grad:
                p.datt.add_(p.datt_clip)          # (datt is overwritten by every call: one add per element, like the loss terms)
            p.loss.add_(p.consistency[1:2])
        elif weak is not None:
            self._k("sed_clip_pool_fwd", self.lib.sed_clip_pool_fwd, L.ptr(teacher_pre), L.ptr(p.teacher_clip), p.B, p.t_out, self.K,
                    self.ratio, Tt, mode_id, _stream())
            self._k("sed_weak_bce_fwd_bwd_ex", self.lib.sed_weak_bce_fwd_bwd_ex, L.ptr(p.pre), L.ptr(p.teacher_clip), 0, None, L.CRIT_MSE,
                    L.ptr(p.clip_prob), L.ptr(p.consistency[1:2]), dpre, 1, *dims, mode_id, float(recall_factor), cw,
                    float(grad_scale), L.ptr(p.weak_ws), _stream())
            p.loss.add_(p.consistency[1:2])
        return p.loss

    def _semi_bufs(self, p: _Plan):
        if p.semi_ws is None:
            dev = p.pre.device
            nb = max(self.lib.sed_bce_sel_ws_bytes(p.B, p.t_out, self.K), self.lib.sed_frame_mse_ws_bytes(p.B, p.t_out, self.K))
            p.semi_ws = torch.empty(max(1, nb // 8), dtype=torch.float64, device=dev)
            p.consistency = torch.zeros(2, dtype=torch.float32, device=dev)
            p.teacher_clip = torch.empty((p.B, self.K), dtype=torch.float32, device=dev)

    def _strong_loss(self, p: _Plan, target: torch.Tensor, recall_factor: float, need_grad: bool, grad_scale: float):
        self._k("sed_bce_fwd_bwd", self.lib.sed_bce_fwd_bwd, L.ptr(p.pre), L.ptr(target), L.ptr(p.loss),
                                         L.ptr(p.dpre) if need_grad else None, L.ptr(p.loss_partial), p.B, p.t_out,
                                         self.K, self.ratio, target.shape[1], float(recall_factor), float(grad_scale),
                                         _stream())

    def _weak_bufs(self, p: _Plan):
        if p.clip_prob is None:
            dev = p.pre.device
            p.clip_prob = torch.empty((p.B, self.K), dtype=torch.float32, device=dev)
            p.weak_ws = torch.empty(max(1, self.lib.sed_weak_bce_ws_bytes(p.B, p.t_out, self.K) // 8), dtype=torch.float64, device=dev)

    def clip_probs(self, p: _Plan, mode: str) -> torch.Tensor:
        """(B, K) clip probabilities of the last forward's logits, pooled over all t_out * ratio output frames by `mode` (max /
        mean / linear / exp, or "att": the attention pooling of an engine with attention=True).  Returns plan.clip_prob: valid
        until the next call on this plan."""
        if self.head == "none":
            check_clip_pooling(mode)
            raise ValueError("clip_probs needs a model with a classification head")
        if check_clip_pooling(mode, self) == ATT_POOLING:
            self._k("sed_att_pool_fwd", self.lib.sed_att_pool_fwd, L.ptr(p.pre), L.ptr(p.att), L.ptr(p.clip_prob), p.B, p.t_out, self.K,
                    self.ratio, p.t_out * self.ratio, _stream())
            return p.clip_prob
        mode_id = check_pooling(mode)
        self._weak_bufs(p)
        self._k("sed_clip_pool_fwd", self.lib.sed_clip_pool_fwd, L.ptr(p.pre), L.ptr(p.clip_prob), p.B, p.t_out, self.K, self.ratio,
                p.t_out * self.ratio, mode_id, _stream())
        return p.clip_prob

    # ------------------------------------------------------------------------------------------
    def backward(self, p: _Plan, P: Dict[str, torch.Tensor], G: Dict[str, torch.Tensor],
                 dlogits: Optional[torch.Tensor] = None, debug: Optional[dict] = None, on_group_done=None,
                 need_dx: bool = False):
        """Backward of the last forward on plan p.  Gradient source: `dlogits`
        (B, t*ratio, K) w.r.t. the interpolated logits, or plan.dpre when None.  Writes fp32 gradients
        into G[name] (tensors shaped like the parameters; overwritten, not accumulated).
        need_dx: also the input gradient of the Cin = 1 model path into plan.dx_in (B, 1, T, F) fp32 (csrc/sed_c1_dx.hip; the
        generic_first path always fills plan.dx).  An eval-mode forward (BatchNorm with running statistics) can be differentiated
        when it ran with keep_for_grad=True; so must a C1-mode training forward whose backward takes need_dx.  Without need_dx, a
        training-mode backward launches exactly what it did before these two kinds existed."""
        if dlogits is not None and p.att_pending:
            raise RuntimeError("backward(dlogits=...) after loss_and_grad(weak=('att', ...)): the attention gradient of that loss is "
                               "pending on this plan (run backward() without dlogits, or a new forward)")
        eval_bwd = not p.trained
        if eval_bwd and not p.keep:
            raise RuntimeError("backward() needs a training-mode forward (batch statistics) or a forward with keep_for_grad=True")
        need_dx = bool(need_dx) and not self.generic_first
        if need_dx and p.c1_mode and not p.keep:
            raise RuntimeError("the input gradient in C1 mode needs a forward with keep_for_grad=True (conv1's ReLU mask)")
        if (eval_bwd or need_dx) and self.bn_sync is not None:
            raise RuntimeError("input-gradient and eval-mode backward are not available with SyncBN")
        new_kind = eval_bwd or need_dx
        c1_plain = new_kind and p.c1_mode     # C1 mode: the unfused block-0 route, which writes g1 and takes the forward's mask
        lib, dt, st = self.lib, self.dt, _stream()
        B = p.B
        if self.head == "none":
            src, ratio = None, 1
        elif dlogits is None:
            src, ratio = p.dpre, 1
        else:
            src, ratio = dlogits.contiguous(), self.ratio
        nb = len(self.cfg)
        self._e_shift = 0
        if new_kind and self.dt_mm == L.SED_F32H3:
            if self.head == "none":
                self._e_shift = self._upstream_shift(p, p.dy[nb - 1], B * self.cfg[-1][0] * p.t_out * p.w_out)
            else:
                self._e_shift = self._upstream_shift(p, src, B * p.t_out * self.ratio * self.K)
        if eval_bwd:
            # BatchNorm as the fixed affine map of its running statistics: (mean, invstd) for the backward statistics kernels
            for bi in range(nb):
                for j in range(2):
                    ly = p.layers[bi][j]
                    _, _, rmn, rvn = self._bn_names(bi, j)
                    self._k("sed_bn_eval_stats", lib.sed_bn_eval_stats, L.ptr(P[rmn]), L.ptr(P[rvn]), BN_EPS, L.ptr(ly.mean),
                            L.ptr(ly.invstd), ly.cout, ly.coutp, st)
        # an eval forward keeps no pooled-tensor statistics (active-pixel counts): the per-pixel pass everywhere
        pool_fused = [False] * nb if eval_bwd else p.pool_fused
        try:
            self._backward_blocks(p, P, G, src, ratio, debug, on_group_done or (lambda name: None), eval_bwd, pool_fused, c1_plain)
        finally:
            self._e_shift = 0
        if need_dx:
            l1 = p.layers[0][0]
            p.dx_in = torch.empty((B, 1, p.T, p.F), dtype=torch.float32, device=p.x_ref.device)     # (fresh: autograd keeps it)
            # dzB holds g1 (conv2's gated data gradient of block 0); (ca, cb, cc) of BN1 are in l1.coef
            self._tag = f"bwd b0 dx H{p.T} W{p.F}"
            self._k("sed_conv3x3_c1_dgrad", lib.sed_conv3x3_c1_dgrad, dt, L.ptr(p.scratch[1]), None if p.c1_mode else L.ptr(l1.z),
                    L.ptr(p.x_ref), L.ptr(p.feat_mean), L.ptr(p.feat_std), L.ptr(P["conv_blocks.0.conv1.weight"]), L.ptr(l1.coef[0]),
                    L.ptr(l1.coef[1]), L.ptr(l1.coef[2]), L.ptr(p.dx_in), B, p.T, p.F, l1.cout, l1.coutp, st)
            self._tag = ""

    def _bn_bwd_fin(self, eval_bwd, bpart, nparts, count, gamma, ly, dg, db):
        ca, cb, cc = ly.coef[0], ly.coef[1], ly.coef[2]
        if eval_bwd:
            self._k("sed_bn_eval_bwd_finalize", self.lib.sed_bn_eval_bwd_finalize, L.ptr(bpart), nparts, L.ptr(gamma), L.ptr(ly.mean),
                    L.ptr(ly.invstd), L.ptr(dg), L.ptr(db), L.ptr(ca), L.ptr(cb), L.ptr(cc), ly.cout, ly.coutp, _stream())
            return
        self._k("sed_bn_bwd_finalize", self.lib.sed_bn_bwd_finalize, L.ptr(bpart), nparts, count, L.ptr(gamma), L.ptr(ly.mean),
                L.ptr(ly.invstd), L.ptr(dg), L.ptr(db), L.ptr(ca), L.ptr(cb), L.ptr(cc), ly.cout, ly.coutp, _stream())

    def _backward_blocks(self, p, P, G, src, ratio, debug, done, eval_bwd, pool_fused, c1_plain):
        lib, dt, st = self.lib, self.dt, _stream()
        B = p.B
        nb = len(self.cfg)
        if self.head_impl is not None:        # (without a head the caller filled plan.dy[-1], the gradient of the last pooled block output)
            self.head_impl.backward(p, P, G, src, ratio, p.dy[nb - 1], done)
        dzA, dzB = p.scratch
        if any(pool_fused):
            p.pool_flag.zero_()

        def snap(name, buf, ly):
            if debug is not None:
                debug[name] = buf[: B * ly.H * ly.W * ly.coutp].view(B, ly.H, ly.W, ly.coutp).float().clone()

        if debug is not None:
            debug[f"dy{nb - 1}"] = p.dy[nb - 1].float().clone()
        for bi in reversed(range(nb)):
            c, pool = self.cfg[bi]
            l1, l2 = p.layers[bi]
            H, W = l2.H, l2.W
            count = float(B * H * W)
            dtg = self._grad_dtype(B, H, W)
            self._tag = f"bwd b{bi}c2 {l2.cin}->{l2.cout} H{H} W{W}"
            g2n, b2n, _, _ = self._bn_names(bi, 1)
            g1n, b1n, _, _ = self._bn_names(bi, 0)
            # ---- pool + ReLU + BN2 backward -> dz2 -------------------------------------------------
            if pool_fused[bi]:
                # the statistics came out of the data gradient that produced dy[bi] (end of the previous iteration); the per-pixel
                # pass runs only if that kernel met a channel with gamma = 0 (device-side flag: the launch returns at once)
                nparts = p.pool_nparts[bi]
                self._k("sed_pool_relu_bwd_stats_if", self.lib.sed_pool_relu_bwd_stats_if, L.ptr(p.pool_flag[bi:]), dt, L.ptr(p.dy[bi]),
                        L.ptr(l2.z), L.ptr(l2.scale), L.ptr(l2.shift), L.ptr(l2.mean), L.ptr(l2.invstd), L.ptr(p.bwd_part), nparts,
                        B, H, W, l2.coutp, pool, st)
            else:
                nparts = lib.sed_pool_bwd_nparts(B, H, W, l2.coutp)
                self._k("sed_pool_relu_bwd_stats", self.lib.sed_pool_relu_bwd_stats, dt, L.ptr(p.dy[bi]), L.ptr(l2.z), L.ptr(l2.scale), L.ptr(l2.shift),
                                                    L.ptr(l2.mean), L.ptr(l2.invstd), L.ptr(p.bwd_part), B, H, W,
                                                    l2.coutp, pool, st)
            ca, cb, cc = l2.coef[0], l2.coef[1], l2.coef[2]
            sync = self.bn_sync
            gcount = count * (sync.world if sync is not None else 1)
            bpart = p.bwd_part
            if sync is not None:        # (dgamma / dbeta then come out as GLOBAL sums: pre-divided by world, the gradient
                bpart, nparts = self._sync_row(p.bwd_part, nparts, 2 * l2.coutp, p.sync_row), 1     # all-reduce sums them back)
            self._bn_bwd_fin(eval_bwd, bpart, nparts, gcount, P[g2n], l2, G[g2n], G[b2n])
            if sync is not None:
                G[g2n].mul_(1.0 / sync.world)
                G[b2n].mul_(1.0 / sync.world)
            # ---- conv2 weight gradient; dz2 = BN2/ReLU/pool backward is produced on load inside the kernel
            #      (and written to dzA for the data-gradient call); its input a1 = relu(bn1(z1)) is
            #      recomputed on load as well -----------------------------------------------------------
            w2n = f"conv_blocks.{bi}.conv2.weight"
            if bi == 0 and p.c1_mode:
                if debug is not None:
                    raise RuntimeError("stage snapshots need conv1's output in memory: set SED_C1_MODE=0 (or use precision='fp32')")
                self._backward_block0_c1(p, P, G, eval_bwd, c1_plain, gcount)
                done("conv_blocks.0")
                continue
            fused2 = p.bwd_fused[bi][1] and debug is None
            if fused2:
                # weight gradient AND gated data gradient from one dz2 tile in LDS: dz2 is never written, z1 is read once
                self._k("sed_conv3x3_bwd_fused", self.lib.sed_conv3x3_bwd_fused, dt, L.PRO_BNRELU, L.ptr(l1.z), L.ptr(l1.scale), L.ptr(l1.shift),
                        L.DZ_POOL, L.ptr(p.dy[bi]), L.ptr(l2.z), L.ptr(l2.scale), L.ptr(l2.shift), L.ptr(ca), L.ptr(cb), L.ptr(cc), pool,
                        L.ptr(l2.wpack_t), L.ptr(dzB), L.EPI_RELUBWD, L.ptr(l1.z), None, L.ptr(l1.scale), L.ptr(l1.shift), L.ptr(l1.mean),
                        L.ptr(l1.invstd), L.ptr(p.bwd_part), lib.sed_conv_nparts(B, H, W), None, L.ptr(l2.dwpack), L.ptr(p.wgrad_ws),
                        B, H, W, l2.cinp, l2.coutp, L.ptr(G[w2n]), l2.cout, l2.cin, st)
            else:
                self._k("sed_conv3x3_wgrad_fused", self.lib.sed_conv3x3_wgrad_fused_u, dtg, L.PRO_BNRELU, L.ptr(l1.z),
                        L.ptr(l1.scale), L.ptr(l1.shift), L.DZ_POOL, L.ptr(p.dy[bi]), L.ptr(l2.z), L.ptr(l2.scale),
                        L.ptr(l2.shift), L.ptr(ca), L.ptr(cb), L.ptr(cc), pool, L.ptr(dzA), L.ptr(l2.dwpack), L.ptr(p.wgrad_ws),
                        B, H, W, l2.cinp, l2.coutp, L.ptr(G[w2n]), l2.cout, l2.cin, st)
            snap(f"dz2_{bi}", dzA, l2)
            # (the reduction kernel of the weight gradient stores G[w2n] in torch layout itself; the data-gradient operator
            #  wpack_t was packed with the forward operators, sed_pack_conv_weights_batch)
            # ---- conv2: data gradient with fused ReLU mask + BN1 backward statistics ---------------
            nparts = lib.sed_conv_nparts(B, H, W)
            if not fused2:
                self._k("sed_conv3x3_fwd", self.lib.sed_conv3x3_fwd, dtg, L.PRO_NONE, L.EPI_RELUBWD, L.ptr(dzA), None, None, L.ptr(l2.wpack_t),
                                            L.ptr(dzB), L.ptr(l1.z), L.ptr(l1.scale), L.ptr(l1.shift), L.ptr(l1.mean),
                                            L.ptr(l1.invstd), L.ptr(p.bwd_part), B, H, W, l2.coutp, l2.cinp, st)
            snap(f"g1_{bi}", dzB, l1)
            ca, cb, cc = l1.coef[0], l1.coef[1], l1.coef[2]
            bpart = p.bwd_part
            if sync is not None:
                bpart, nparts = self._sync_row(p.bwd_part, nparts, 2 * l1.coutp, p.sync_row), 1
            self._bn_bwd_fin(eval_bwd, bpart, nparts, gcount, P[g1n], l1, G[g1n], G[b1n])
            if sync is not None:
                G[g1n].mul_(1.0 / sync.world)
                G[b1n].mul_(1.0 / sync.world)
            w1n = f"conv_blocks.{bi}.conv1.weight"
            xin = p.y[bi - 1] if bi > 0 else getattr(p, "x_nhwc", None)
            dxout = p.dy[bi - 1] if bi > 0 else getattr(p, "dx", None)
            if bi == 0 and not self.generic_first:
                # first layer (Cin = 1): direct weight-gradient kernel with dz1 = BN1 backward computed on load
                # from (g1, z1); block 0 has no data gradient, so dz1 is never written to memory
                self._tag = f"bwd b{bi}c1 {l1.cin}->{l1.cout} H{H} W{W}"
                if debug is not None:
                    tmp = torch.empty_like(dzB[: B * H * W * l1.coutp])
                    self._k("sed_bn_bwd_apply", self.lib.sed_bn_bwd_apply, dt, L.ptr(dzB), L.ptr(l1.z), L.ptr(ca), L.ptr(cb),
                            L.ptr(cc), L.ptr(tmp), B * H * W, l1.coutp, st)
                    snap(f"dz1_{bi}", tmp, l1)
                # dW1 = ca*A + cb*(w1.G) + cc*sx: A = plain weight gradient of g1, G / sx = Gram statistics of the
                # input patches -- z1 is not read (csrc/sed_c1.hip: conv_c1_gram_kernel)
                self._k("sed_conv3x3_c1_gram", self.lib.sed_conv3x3_c1_gram, L.ptr(p.x_ref), L.ptr(p.feat_mean),
                        L.ptr(p.feat_std), L.ptr(p.c1_gram), B, H, W, st)
                self._k("sed_conv3x3_c1_wgrad", self.lib.sed_conv3x3_c1_wgrad, dt, L.ptr(p.x_ref), L.ptr(p.feat_mean),
                        L.ptr(p.feat_std), L.ptr(dzB), L.ptr(p.c1_ws), B, H, W, l1.coutp, st)
                self._k("sed_sum_partials", self.lib.sed_sum_partials, L.ptr(p.c1_ws), p.c1_ws.shape[0], 9 * l1.coutp,
                        L.ptr(p.c1_A), st)
                self._k("sed_conv3x3_c1_wgrad_combine", self.lib.sed_conv3x3_c1_wgrad_combine_u, L.ptr(p.c1_A), L.ptr(p.c1_gram),
                        p.c1_gram.shape[0], L.ptr(P[w1n]), L.ptr(ca), L.ptr(cb), L.ptr(cc), L.ptr(l1.dwpack), l1.cout,
                        l1.coutp, L.ptr(G[w1n]), st)
            else:
                # conv1 weight gradient with dz1 = BN1 backward produced on load from (g1, z1); dz1 lands
                # in dzA (dz2 is dead by now) for the data-gradient call below
                self._tag = f"bwd b{bi}c1 {l1.cin}->{l1.cout} H{H} W{W}"
                # (the fused form was chosen for the plan's epilogue: an eval backward without pooled statistics takes the two kernels)
                if p.bwd_fused[bi][0] and debug is None and not (eval_bwd and bi > 0 and p.pool_fused[bi - 1]):
                    pst = bi > 0 and pool_fused[bi - 1]
                    q2 = p.layers[bi - 1][1] if pst else None
                    self._k("sed_conv3x3_bwd_fused", self.lib.sed_conv3x3_bwd_fused, dt, L.PRO_NONE, L.ptr(xin), None, None, L.DZ_BN, L.ptr(dzB),
                            L.ptr(l1.z), None, None, L.ptr(ca), L.ptr(cb), L.ptr(cc), 1, L.ptr(l1.wpack_t), L.ptr(dxout),
                            L.EPI_POOLSTATS if pst else L.EPI_STORE, L.ptr(p.y[bi - 1]) if pst else None,
                            L.ptr(p.pool_cnt[bi - 1]) if pst else None, L.ptr(q2.scale) if pst else None, L.ptr(q2.shift) if pst else None,
                            L.ptr(q2.mean) if pst else None, L.ptr(q2.invstd) if pst else None, L.ptr(p.bwd_part) if pst else None,
                            p.pool_nparts[bi - 1] if pst else 0, L.ptr(p.pool_flag[bi - 1:]) if pst else None, L.ptr(l1.dwpack), L.ptr(p.wgrad_ws),
                            B, H, W, l1.cinp, l1.coutp, L.ptr(G[w1n]), l1.cout, l1.cin, st)
                    done(f"conv_blocks.{bi}")
                    continue
                self._k("sed_conv3x3_wgrad_fused", self.lib.sed_conv3x3_wgrad_fused_u, dtg, L.PRO_NONE, L.ptr(xin),
                        None, None, L.DZ_BN, L.ptr(dzB), L.ptr(l1.z), None, None, L.ptr(ca), L.ptr(cb), L.ptr(cc), 1,
                        L.ptr(dzA), L.ptr(l1.dwpack), L.ptr(p.wgrad_ws), B, H, W, l1.cinp, l1.coutp, L.ptr(G[w1n]), l1.cout,
                        l1.cin, st)
                snap(f"dz1_{bi}", dzA, l1)
                if bi > 0 and pool_fused[bi - 1]:
                    q2 = p.layers[bi - 1][1]      # the block whose pooled output this gradient belongs to
                    self._k("sed_conv3x3_dgrad_poolstats", self.lib.sed_conv3x3_dgrad_poolstats, dt, L.ptr(dzA), L.ptr(l1.wpack_t),
                            L.ptr(dxout), L.ptr(p.y[bi - 1]), L.ptr(p.pool_cnt[bi - 1]), L.ptr(q2.scale), L.ptr(q2.shift), L.ptr(q2.mean),
                            L.ptr(q2.invstd), L.ptr(p.bwd_part), p.pool_nparts[bi - 1], L.ptr(p.pool_flag[bi - 1:]), B, H, W,
                            l1.coutp, l1.cinp, st)
                else:
                    self._k("sed_conv3x3_fwd", self.lib.sed_conv3x3_fwd, dtg, L.PRO_NONE, L.EPI_STORE, L.ptr(dzA), None, None,
                            L.ptr(l1.wpack_t), L.ptr(dxout), None, None, None, None, None, None, B, H, W, l1.coutp,
                            l1.cinp, st)
                if debug is not None and bi > 0:
                    debug[f"dy{bi - 1}"] = p.dy[bi - 1].float().clone()
            done(f"conv_blocks.{bi}")
        self._tag = ""

    def _backward_block0_c1(self, p, P, G, eval_bwd, plain, gcount):
        """Block 0's backward in C1 mode, from the pooled gradient plan.dy[0] (BN2's coefficients are in place) to dW2, BN1's
        gradients and dW1.  One section per route (block0_route); `plain`: this backward needs g1 in memory (need_dx, eval mode)."""
        lib, dt, st, sync = self.lib, self.dt, _stream(), self.bn_sync
        l1, l2 = p.layers[0]
        B, H, W, pool = p.B, l2.H, l2.W, self.cfg[0][1]
        dzA, dzB = p.scratch
        w1n, w2n = "conv_blocks.0.conv1.weight", "conv_blocks.0.conv2.weight"
        g1n, b1n, _, _ = self._bn_names(0, 0)
        ca, cb, cc = l1.coef[0], l1.coef[1], l1.coef[2]
        tag1 = f"bwd b0c1 {l1.cin}->{l1.cout} H{H} W{W}"
        # conv2's weight-gradient launches rebuild a1 = relu(bn1(conv1(x))) from the input; dz2 = BN2 / ReLU / pool backward on load
        conv2 = (dt, L.ptr(p.x_ref), L.ptr(p.feat_mean), L.ptr(p.feat_std), L.ptr(P[w1n]), L.ptr(l1.scale), L.ptr(l1.shift),
                 L.ptr(p.dy[0]), L.ptr(l2.z), L.ptr(l2.scale), L.ptr(l2.shift), L.ptr(l2.coef[0]), L.ptr(l2.coef[1]), L.ptr(l2.coef[2]), pool)
        dw2 = (L.ptr(l2.dwpack), L.ptr(p.wgrad_ws), B, H, W, l2.coutp, L.ptr(G[w2n]), l2.cout, l2.cin, st)

        if plain:
            # ---- c1_plain: g1 is written (dzB; backward() turns it into the input gradient), with the mask of the kept forward --------
            mask = p.c1_mask if p.c1_mask is not None else p.c1_mask_keep
            self._k("sed_conv3x3_wgrad_fused_c1", lib.sed_conv3x3_wgrad_fused_c1_u, *conv2, L.ptr(dzA), *dw2)
            self._k("sed_conv3x3_dgrad_c1", lib.sed_conv3x3_dgrad_c1, dt, L.ptr(dzA), L.ptr(l2.wpack_t), L.ptr(dzB),
                    L.ptr(mask), L.ptr(p.bwd_part), B, H, W, l2.coutp, st)
            # BN1 backward needs sum g*z1 = w1 . A with A = the plain first-layer weight gradient of g1: that kernel runs first
            self._tag = tag1
            self._k("sed_conv3x3_c1_wgrad", lib.sed_conv3x3_c1_wgrad, dt, L.ptr(p.x_ref), L.ptr(p.feat_mean),
                    L.ptr(p.feat_std), L.ptr(dzB), L.ptr(p.c1_ws), B, H, W, l1.coutp, st)
            self._k("sed_sum_partials", lib.sed_sum_partials, L.ptr(p.c1_ws), p.c1_ws.shape[0], 9 * l1.coutp, L.ptr(p.c1_A), st)
            fin = (L.ptr(p.c1_A), L.ptr(P[w1n]), L.ptr(P[g1n]), L.ptr(l1.mean), L.ptr(l1.invstd), L.ptr(G[g1n]),
                   L.ptr(G[b1n]), L.ptr(ca), L.ptr(cb), L.ptr(cc), l1.cout, l1.coutp, st)
            nparts = lib.sed_conv_nparts(B, H, W)
            if eval_bwd:
                self._k("sed_bn_eval_bwd_finalize_c1", lib.sed_bn_eval_bwd_finalize_c1, L.ptr(p.bwd_part), nparts, *fin)
                # (dW1 = ca*A: the Gram statistics enter with cb = cc = 0, but an eval forward did not compute them)
                self._k("sed_conv3x3_c1_gram", lib.sed_conv3x3_c1_gram, L.ptr(p.x_ref), L.ptr(p.feat_mean),
                        L.ptr(p.feat_std), L.ptr(p.c1_gram), B, H, W, st)
            else:
                self._k("sed_bn_bwd_finalize_c1", lib.sed_bn_bwd_finalize_c1, L.ptr(p.bwd_part), nparts, float(B * H * W), *fin)
            self._c1_combine(p, P, G, p.c1_A)
            return

        if p.c1_route == "c1_fused":
            # ---- c1_fused: dW2 and the [A; sum g] partials of the gated data gradient from one dz2 tile in LDS; dz2 and g are never
            #      written, the ReLU gate is derived in the kernel (mask NULL) ------------------------------------------------------
            self._k("sed_conv3x3_bwd_fused_c1", lib.sed_conv3x3_bwd_fused_c1, *conv2, L.ptr(l2.wpack_t), None, L.ptr(p.c1_a10_part), *dw2)
        else:
            # ---- c1_stats: dz2 through memory (dzA); g is never written: the data gradient gates conv2^T(dz2) with the forward's
            #      mask in registers and reduces it to A = sum_px g (x) patch and sum g on the matrix pipe -----------------------------
            self._k("sed_conv3x3_wgrad_fused_c1", lib.sed_conv3x3_wgrad_fused_c1_u, *conv2, L.ptr(dzA), *dw2)
            self._k("sed_conv3x3_dgrad_c1_stats", lib.sed_conv3x3_dgrad_c1_stats, dt, L.ptr(dzA), L.ptr(l2.wpack_t),
                    L.ptr(p.x_ref), L.ptr(p.feat_mean), L.ptr(p.feat_std), L.ptr(p.c1_mask), L.ptr(p.c1_a10_part), B, H, W, st)
        # ---- the tail of both: [A; sum g] partial rows -> BN1 backward coefficients -> dW1 --------------------------------------------
        self._tag = tag1
        if sync is None:
            # one launch, with the Gram statistics the forward's finalize reduced
            self._k("sed_c1_bwd_tail", lib.sed_c1_bwd_tail, L.ptr(p.c1_a10_part), p.c1_a10_part.shape[0], L.ptr(p.c1_gsum), gcount,
                    L.ptr(P[w1n]), L.ptr(P[g1n]), L.ptr(l1.mean), L.ptr(l1.invstd), L.ptr(G[g1n]), L.ptr(G[b1n]), L.ptr(ca), L.ptr(cb),
                    L.ptr(cc), L.ptr(p.c1_a10), L.ptr(l1.dwpack), l1.cout, l1.coutp, L.ptr(G[w1n]), st)
            return
        # SyncBN: BN1's backward statistics over the global batch; dW1's combine keeps the LOCAL A / Gram
        self._k("sed_sum_partials", lib.sed_sum_partials, L.ptr(p.c1_a10_part), p.c1_a10_part.shape[0], 10 * 32, L.ptr(p.c1_a10), st)
        p.sync_a10.copy_(p.c1_a10)
        sync.all_reduce(p.sync_a10)
        a10 = p.sync_a10          # rows 0..8 = A, row 9 = sum g (read as a one-row statistics partial)
        self._k("sed_bn_bwd_finalize_c1", lib.sed_bn_bwd_finalize_c1, L.ptr(a10[9]), 1, gcount, L.ptr(a10), L.ptr(P[w1n]),
                L.ptr(P[g1n]), L.ptr(l1.mean), L.ptr(l1.invstd), L.ptr(G[g1n]), L.ptr(G[b1n]), L.ptr(ca), L.ptr(cb), L.ptr(cc),
                l1.cout, l1.coutp, st)
        G[g1n].mul_(1.0 / sync.world)
        G[b1n].mul_(1.0 / sync.world)
        self._c1_combine(p, P, G, p.c1_a10)

    def _c1_combine(self, p, P, G, a_sum):
        """dW1 = ca*A + cb*(w1.G) + cc*sx: A = the weight gradient of g1 (rows 0..8 of a_sum), G / sx = Gram statistics of the input patches"""
        l1, w1n = p.layers[0][0], "conv_blocks.0.conv1.weight"
        self._k("sed_conv3x3_c1_wgrad_combine", self.lib.sed_conv3x3_c1_wgrad_combine_u, L.ptr(a_sum), L.ptr(p.c1_gram),
                p.c1_gram.shape[0], L.ptr(P[w1n]), L.ptr(l1.coef[0]), L.ptr(l1.coef[1]), L.ptr(l1.coef[2]), L.ptr(l1.dwpack), l1.cout,
                l1.coutp, L.ptr(G[w1n]), _stream())

    # ------------------------------------------------------------------------------------------
    def adam_step_dev(self, flat_p, flat_g, flat_m, flat_v, flat_vmax, hyper, step_dev, grad_scale: float, lr_decay: float,
                      decay_every: int, betas=(0.9, 0.999), eps: float = 1e-8):
        """Adam-amsgrad with the step counter / learning rate / bias corrections in device memory (graph replay)."""
        self._k("sed_adam_amsgrad_step_dev", self.lib.sed_adam_amsgrad_step_dev, L.ptr(flat_p), L.ptr(flat_g), L.ptr(flat_m),
                L.ptr(flat_v), L.ptr(flat_vmax), flat_p.numel(), L.ptr(hyper), L.ptr(step_dev), float(betas[0]), float(betas[1]),
                float(eps), float(grad_scale), float(lr_decay), int(decay_every), _stream())

    def adam_step(self, flat_p, flat_g, flat_m, flat_v, flat_vmax, lr: float, step: int, grad_scale: float = 1.0,
                  betas=(0.9, 0.999), eps: float = 1e-8):
        self._k("sed_adam_amsgrad_step", self.lib.sed_adam_amsgrad_step, L.ptr(flat_p), L.ptr(flat_g), L.ptr(flat_m), L.ptr(flat_v),
                                               L.ptr(flat_vmax), flat_p.numel(), float(lr), float(betas[0]),
                                               float(betas[1]), float(eps), int(step), float(grad_scale), _stream())
