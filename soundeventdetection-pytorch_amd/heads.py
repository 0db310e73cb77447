"""The temporal heads of CnnEngine -- what runs between the last pooled conv block and the logits -- and the attention pooling beside
them: FcHead (Cnn_AvgPooling), GruHead (Crnn_AvgPooling) and SaHead (Csa_AvgPooling, configured by a SaConfig).  An engine has one
(engine.head_impl, None for head='none').  A head allocates its buffers into the engine's plan (a captured step allocates nothing)
and enqueues its launches through the engine it was given: engine.lib, dt, tdtype, K, cfg, Hd, attention, _k and _tag.
SaConfig is host-only: no device, no library call."""
from __future__ import annotations

import ctypes as _C
import os as _os
from dataclasses import dataclass, fields
from typing import Optional

import numpy as np
import torch

from . import _lib as L

BN_EPS = 1e-5
BN_MOMENTUM = 0.1
LN_EPS = 1e-5        # the self-attention head's LayerNorm (torch.nn.LayerNorm's default)


def pad32(c: int) -> int:
    return (c + 31) // 32 * 32


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _integer(x) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


@dataclass
class SaConfig:
    """The options of the self-attention head, checked once against the last block's channel count C (a ValueError for what the
    kernels do not cover) and kept in their checked form.  With R = B*t rows:
    heads: H heads of width C / H (32 or 64) in every layer; pos_encoding adds the fixed sinusoidal table to the mel-mean rows.
    layers post-LN encoder layers, each with a feed-forward sub-layer of width ffn > 0 and activation 'relu' / 'gelu' behind the
    attention (csrc/sed_ffn.hip) -- torch.nn.TransformerEncoderLayer(C, heads, ffn, dropout=0, norm_first=False) semantics.
    conv_kernel = k > 0, odd in [3, 31], puts the Conformer convolution module -- pointwise conv, GLU, depthwise conv of k taps along
    time, BatchNorm, SiLU, pointwise conv, residual LayerNorm -- between the two (csrc/sed_convmod.hip).
    dropout = p in [0, 1): torch.nn.TransformerEncoderLayer(dropout=p)'s placement in TRAINING forwards and their backwards -- the
    attention probabilities, each sub-layer's output before its residual add, the FFN hidden activation -- with masks generated inside
    the kernels from the counter-based state (seed_lo, seed_hi, step, 0) (csrc/philox.h); dropout_seed: the 64-bit seed, None ->
    torch.initial_seed() when the head is built (no random number is drawn).
    window = None, an int w or a pair (left, right), None on a side for unbounded: the local attention window of every head of every
    layer (key j takes part for query i iff i - left <= j <= i + right; torch's src_mask), in every forward and backward.
    rel_pos = None, an int L >= 1 (clipped distances, 2L + 1 buckets) or a pair (num_buckets, max_distance) (T5's bidirectional log
    buckets): a learned bias per head and bucket of the distance j - i on every score of every layer, P["rel_pos*.weight"]
    (H, num_buckets).  It composes with window and dropout.
    norm_first: pre-LN layers -- every sub-layer is x <- x + f(LayerNorm(x)) on a residual stream (its norm attn_norm* / conv_norm* /
    ffn_norm* in FRONT of it), and the last layer ends with a closing LayerNorm out_norm*, which event_fc reads:
    torch.nn.TransformerEncoder(TransformerEncoderLayer(norm_first=True), N, norm=LayerNorm(C)).  One launch adds sub-layer j's
    output and normalises for sub-layer j + 1 (sed_resid_layernorm_fwd / _bwd, csrc/sed_layernorm.hip).
    macaron (needs norm_first and ffn > 0): the Conformer block -- a second FFN ffn_mac* behind ffn_mac_norm* in front of the
    attention, both FFNs added with the weight 1/2, and a closing norm on EVERY layer.
    Every option at its default launches what the one-layer head always did."""
    channels: int
    heads: int = 4
    pos_encoding: bool = True
    layers: int = 1
    ffn: int = 0
    activation: str = "relu"
    conv_kernel: int = 0
    dropout: float = 0.0
    dropout_seed: Optional[int] = None
    window: object = None
    rel_pos: object = None
    norm_first: bool = False
    macaron: bool = False

    RELPOS_MAX_BUCKETS = 4096

    def __post_init__(self):
        C, H, D, k = self.channels, self.heads, self.ffn, self.conv_kernel
        self.dropout, self.window, self.rel_pos = self.check_dropout(self.dropout), self.check_window(self.window), self.check_rel_pos(self.rel_pos)
        self.dropout_seed = None if self.dropout_seed is None else int(self.dropout_seed)
        self.pos_encoding = bool(self.pos_encoding)
        if not _integer(H) or H < 1:
            raise ValueError(f"sa_heads must be a positive integer, got {H!r}")
        if C % 4:
            raise ValueError(f"the self-attention head needs a channel count that is a multiple of 4, got {C}")
        if C % H:
            raise ValueError(f"the last block's {C} channels do not divide into sa_heads={H} heads")
        if C // H not in (32, 64):
            raise ValueError(f"head width {C // H} unsupported (channels {C} / sa_heads {H}): the attention kernels cover head widths 32 and 64")
        if not _integer(self.layers) or self.layers < 1:
            raise ValueError(f"sa_layers must be a positive integer, got {self.layers!r}")
        if not _integer(D) or D < 0 or D % 32 or D > 4096:
            raise ValueError(f"sa_ffn must be 0 (no feed-forward sub-layer) or a multiple of 32 up to 4096, got {D!r}")
        if D and C > 512:
            raise ValueError(f"sa_ffn: the feed-forward kernel takes at most 512 channels, the last block has {C}")
        if self.activation not in L.FFN_ACT:
            raise ValueError(f"sa_activation must be 'relu' or 'gelu', got {self.activation!r}")
        if not _integer(k) or (k != 0 and (k < 3 or k > 31 or k % 2 == 0)):
            raise ValueError(f"sa_conv_kernel must be 0 (no convolution module) or an odd integer in [3, 31], got {k!r}")
        self.norm_first, self.macaron = bool(self.norm_first), bool(self.macaron)
        if self.macaron and not self.norm_first:
            raise ValueError("sa_macaron needs sa_norm_first: the macaron half-step FFNs belong to the pre-LN block")
        if self.macaron and not D:
            raise ValueError("sa_macaron needs a feed-forward sub-layer (sa_ffn > 0)")

    @staticmethod
    def keyword(name: str) -> str:
        """the keyword of CnnEngine / Csa_AvgPooling (and the attribute they keep) for the field `name`"""
        return name if name == "pos_encoding" else "sa_" + name

    BLOCK_SWITCHES = ("norm_first", "macaron")

    def keywords(self, every: bool = False) -> dict:
        """the options under the keywords of CnnEngine / Csa_AvgPooling, in their checked form; the block switches norm_first and
        macaron only where one is set (a post-LN configuration has the keywords it always had), or with every=True"""
        skip = () if every or self.norm_first else self.BLOCK_SWITCHES
        return {self.keyword(f.name): getattr(self, f.name) for f in fields(self)[1:] if f.name not in skip}

    @classmethod
    def absent(cls, *options) -> dict:
        """the options (in the fields' order) of an engine without the head, under their keywords: a ValueError unless all are defaults"""
        for f, v in zip(fields(cls)[1:], options):
            if f.name in ("dropout", "window", "rel_pos"):
                v = getattr(cls, "check_" + f.name)(v)
            if v != f.default:
                raise ValueError(f"{cls.keyword(f.name)} belongs to the self-attention head (head='sa')")
        return {cls.keyword(f.name): f.default for f in fields(cls)[1:]}

    @staticmethod
    def check_dropout(p) -> float:
        """a probability in [0, 1) (NaN refused)"""
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= float(p) < 1.0:
            raise ValueError(f"sa_dropout must be a probability in [0, 1), got {p!r}")
        return float(p)

    @staticmethod
    def check_window(w):
        """None, an int w >= 0 (left = right = w) or a pair (left, right) of ints >= 0 / None (unbounded) -> None or the pair"""
        def side(v):
            if v is None:
                return None
            if not _integer(v) or v < 0:
                raise ValueError(f"a side of sa_window must be None (unbounded) or an integer >= 0, got {v!r}")
            return v
        if w is None:
            return None
        if isinstance(w, (tuple, list)):
            if len(w) != 2:
                raise ValueError(f"sa_window must be None, an integer or a pair (left, right), got {w!r}")
            return side(w[0]), side(w[1])
        if not _integer(w):
            raise ValueError(f"sa_window must be None, an integer or a pair (left, right), got {w!r}")
        return side(w), side(w)

    @staticmethod
    def check_rel_pos(v):
        """None, an int L >= 1 or a pair (num_buckets even >= 4, max_distance > num_buckets / 4) -> None, ("clip", L) or
        ("log", num_buckets, max_distance); at most RELPOS_MAX_BUCKETS buckets"""
        most = SaConfig.RELPOS_MAX_BUCKETS
        if v is None:
            return None
        if isinstance(v, (tuple, list)):
            if len(v) == 2 and v[0] == "clip":         # (what this function returned)
                v = v[1]
            elif len(v) == 3 and v[0] == "log":
                v = v[1:]
        if isinstance(v, (tuple, list)):
            if len(v) != 2 or not _integer(v[0]) or not _integer(v[1]):
                raise ValueError(f"sa_rel_pos must be None, an integer L >= 1 or a pair of integers (num_buckets, max_distance), got {v!r}")
            nb, maxd = v
            if nb < 4 or nb % 2:
                raise ValueError(f"sa_rel_pos: num_buckets must be even and >= 4, got {nb}")
            if 4 * maxd <= nb:
                raise ValueError(f"sa_rel_pos: max_distance must exceed num_buckets / 4, got {maxd} with {nb} buckets")
            if nb > most:
                raise ValueError(f"sa_rel_pos: at most {most} buckets, got {nb}")
            return "log", nb, maxd
        if not _integer(v) or v < 1:
            raise ValueError(f"sa_rel_pos must be None, an integer L >= 1 or a pair of integers (num_buckets, max_distance), got {v!r}")
        if 2 * v + 1 > most:
            raise ValueError(f"sa_rel_pos: at most {most} buckets, L = {v} gives {2 * v + 1}")
        return "clip", v

    @staticmethod
    def rel_pos_buckets(cfg):
        """the number of buckets of a checked rel_pos"""
        return 2 * cfg[1] + 1 if cfg[0] == "clip" else cfg[1]

    @staticmethod
    def rel_pos_map(cfg, t):
        """int32 (2t - 1,): the bucket of distance d = j - i at index d + t - 1.  clip: clamp(d, -L, L) + L.  log (T5, bidirectional),
        n = nb / 2, a = |d|, m = n / 2: (n if d > 0 else 0) + (a if a < m else min(n - 1, m + floor(ln(a / m) / ln(maxd / m) * (n - m)))),
        evaluated in float64 as written"""
        d = np.arange(-(t - 1), t, dtype=np.int64)
        if cfg[0] == "clip":
            return (np.clip(d, -cfg[1], cfg[1]) + cfg[1]).astype(np.int32)
        nb, maxd = cfg[1], cfg[2]
        n = nb // 2
        m = n // 2
        a = np.abs(d)
        big = m + np.floor(np.log(np.maximum(a, 1).astype(np.float64) / m) / np.log(float(maxd) / m) * (n - m)).astype(np.int64)
        return (np.where(d > 0, n, 0) + np.where(a < m, a, np.minimum(n - 1, big))).astype(np.int32)

    @staticmethod
    def layer_names(l):
        """(attn, attn_norm, ffn, ffn_norm) module names of encoder layer l: layer 0 keeps the one-layer head's names"""
        sfx = "" if l == 0 else f"_l{l}"
        return "attn" + sfx, "attn_norm" + sfx, "ffn" + sfx, "ffn_norm" + sfx

    @staticmethod
    def conv_names(l):
        """(convm, conv_norm) module names of encoder layer l's convolution module (between attn_norm* and ffn* of layer_names)"""
        sfx = "" if l == 0 else f"_l{l}"
        return "convm" + sfx, "conv_norm" + sfx

    @staticmethod
    def macaron_names(l):
        """(ffn_mac, ffn_mac_norm) module names of encoder layer l's macaron FFN (norm_first + macaron: in front of attn_norm*)"""
        sfx = "" if l == 0 else f"_l{l}"
        return "ffn_mac" + sfx, "ffn_mac_norm" + sfx

    @staticmethod
    def out_name(l):
        """module name of encoder layer l's closing LayerNorm (norm_first: every layer with macaron, else the last layer)"""
        return "out_norm" if l == 0 else f"out_norm_l{l}"

    def has_out_norm(self, l) -> bool:
        """whether layer l ends with a closing LayerNorm"""
        return self.norm_first and (self.macaron or l == self.layers - 1)

    def sublayers(self, l):
        """norm_first: layer l's sub-layers in forward order as (kind, module, norm module, residual weight, dropout site of the
        output before its add); kind 'mac' / 'attn' / 'conv' / 'ffn'"""
        an, nn_, fn, fnn = self.layer_names(l)
        out = []
        if self.macaron:
            mn, mnn = self.macaron_names(l)
            out.append(("mac", mn, mnn, 0.5, 6))
        out.append(("attn", an, nn_, 1.0, 1))
        if self.conv_kernel:
            cm, cn = self.conv_names(l)
            out.append(("conv", cm, cn, 1.0, 2))
        if self.ffn:
            out.append(("ffn", fn, fnn, 0.5 if self.macaron else 1.0, 4))
        return out

    def module_order(self):
        """the head's parameter modules in registration order (event_fc / att_fc excluded): post-LN attn, rel_pos, attn_norm, convm,
        conv_norm, ffn, ffn_norm per layer; norm_first ffn_mac_norm, ffn_mac, attn_norm, attn, rel_pos, conv_norm, convm, ffn_norm,
        ffn, out_norm -- each norm before its sub-layer, because its gradient completes after the sub-layer's"""
        names = []
        for l in range(self.layers):
            an, nn_, fn, fnn = self.layer_names(l)
            rel = [self.rel_name(l)] if self.rel_pos is not None else []
            if self.norm_first:
                for kind, mod, norm, _, _ in self.sublayers(l):
                    names += [norm, mod] + (rel if kind == "attn" else [])
                if self.has_out_norm(l):
                    names.append(self.out_name(l))
            else:
                names += [an] + rel + [nn_]
                if self.conv_kernel:
                    names += list(self.conv_names(l))
                if self.ffn:
                    names += [fn, fnn]
        return names

    @staticmethod
    def rel_name(l):
        """module name of encoder layer l's relative-position table (between attn* and attn_norm* of layer_names)"""
        return "rel_pos" if l == 0 else f"rel_pos_l{l}"


class _Head:
    """What the three heads share: event_fc on top of whatever operands() describes, forward and backward, and the attention pooling
    beside it (engine.attention: a second linear layer att_fc scores every frame per class, csrc/sed_attn.hip -- forward() also leaves
    the attention logits in plan.att, loss_and_grad(weak=("att", ...)) pools with them and backward() then takes both layers)."""
    tag = ""        # the KernelTimer tag of the head's launches

    def __init__(self, eng):
        self.eng = eng

    def plan(self, p, B, t, C, dev, W=None):
        """Buffers of the head, allocated with the plan; W: the width event_fc (and att_fc) read, the last block's channels C unless
        given.  With attention: the logits and their gradients, the loss workspace, and the packed operands / results of the two
        layers' backward through sed_head_bwd."""
        eng, K, W = self.eng, self.eng.K, W or C
        f32 = dict(dtype=torch.float32, device=dev)
        p.head_ws = torch.empty(max(1, eng.lib.sed_head_bwd_ws_floats(B, t, W, max(1, K) * (2 if eng.attention else 1))), **f32)
        if eng.attention:
            p.att = torch.empty((B, t, K), **f32)
            p.datt = torch.empty((B, t, K), **f32)
            p.datt_clip = torch.empty((B, t, K), **f32)      # the clip consistency term's, added to datt
            p.att_ws = torch.empty(max(1, eng.lib.sed_att_loss_ws_bytes(B, t, K) // 8), dtype=torch.float64, device=dev)
            p.att_dcat = torch.empty((B * t, 2 * K), **f32)
            p.att_wcat = torch.empty((2 * K, W), **f32)
            p.att_dw = torch.empty((2 * K, W), **f32)
            p.att_db = torch.empty(2 * K, **f32)
            p.clip_prob = torch.empty((B, K), **f32)
            p.weak_ws = torch.empty(max(1, eng.lib.sed_weak_bce_ws_bytes(B, t, K) // 8), dtype=torch.float64, device=dev)

    def operands(self, p):
        """(dtype, m, rows, Wf, C, Cp, feature gradient) of the linear layer(s) on top: the mel-mean the head forward leaves behind"""
        raise NotImplementedError

    def _forward(self, p, P, feat, keep, training, update_running_stats):
        """the launches in front of event_fc; returns what event_fc reads"""
        return feat

    def _backward(self, p, P, G, dfeat, done):
        """the launches behind event_fc's backward: operands()' feature gradient -> dfeat"""

    def forward(self, p, P, feat, keep, training, update_running_stats):
        """feat: the last pooled block output -> plan.pre (and plan.att).  keep: keep what a backward reads; training: batch
        statistics and dropout (a kept eval forward has keep without training)."""
        eng, st = self.eng, _stream()
        eng._tag = self.tag
        x = self._forward(p, P, feat, keep, training, update_running_stats)
        dt, m, rows, Wf, C, Cp, _ = self.operands(p)
        eng._k("sed_head_fwd", eng.lib.sed_head_fwd, dt, L.ptr(x), L.ptr(P["event_fc.weight"]), L.ptr(P["event_fc.bias"]), L.ptr(m),
               L.ptr(p.pre), p.B, p.t_out, Wf, C, Cp, eng.K, st)
        if eng.attention:
            eng._k("sed_att_logits_fwd", eng.lib.sed_att_logits_fwd, L.ptr(m), L.ptr(P["att_fc.weight"]), L.ptr(P["att_fc.bias"]),
                   L.ptr(p.att), rows, C, Cp, eng.K, st)
        eng._tag = ""

    def backward(self, p, P, G, src, ratio, dfeat, done):
        """src: the gradient of plan.pre (ratio 1) or of the interpolated logits -> G of the head's parameters and dfeat, the
        gradient of the last pooled block output.  done(name): a parameter group's gradients are enqueued.
        First event_fc's backward into operands()' feature gradient.  After loss_and_grad(weak=("att", ...)): both layers through ONE
        sed_head_bwd on the packed [rows][2K] gradients and [2K][C] weight -- the feature gradient is (dpre@fc_w + datt@att_w)/Wf,
        summed in fp32 and rounded once.  Otherwise event_fc alone, and att_fc's gradient (where there is one) is zero: the flat
        gradient buffer is overwritten every step and must not keep stale values.  Then the head's own launches (_backward)."""
        eng, lib, st, K = self.eng, self.eng.lib, _stream(), self.eng.K
        dt, m, rows, Wf, C, Cp, dhead = self.operands(p)
        eng._tag = self.tag
        if p.att_pending:
            eng._k("sed_att_bwd_pack", lib.sed_att_bwd_pack, L.ptr(p.dpre), L.ptr(p.datt), L.ptr(P["event_fc.weight"]),
                   L.ptr(P["att_fc.weight"]), L.ptr(p.att_dcat), L.ptr(p.att_wcat), rows, C, K, st)
            eng._k("sed_head_bwd", lib.sed_head_bwd, dt, L.ptr(p.att_dcat), L.ptr(m), L.ptr(p.att_wcat), L.ptr(p.att_dw),
                   L.ptr(p.att_db), L.ptr(dhead), L.ptr(p.head_ws), p.B, p.t_out, Wf, C, Cp, 2 * K, 1, st)
            eng._k("sed_att_bwd_split", lib.sed_att_bwd_split, L.ptr(p.att_dw), L.ptr(p.att_db), L.ptr(G["event_fc.weight"]),
                   L.ptr(G["event_fc.bias"]), L.ptr(G["att_fc.weight"]), L.ptr(G["att_fc.bias"]), C, K, st)
        else:
            eng._k("sed_head_bwd", lib.sed_head_bwd, dt, L.ptr(src), L.ptr(m), L.ptr(P["event_fc.weight"]),
                   L.ptr(G["event_fc.weight"]), L.ptr(G["event_fc.bias"]), L.ptr(dhead), L.ptr(p.head_ws), p.B, p.t_out, Wf,
                   C, Cp, K, ratio, st)
            if eng.attention:
                G["att_fc.weight"].zero_()
                G["att_fc.bias"].zero_()
        if eng.attention:
            done("att_fc")
        done("event_fc")
        self._backward(p, P, G, dfeat, done)
        eng._tag = ""


class FcHead(_Head):
    """Cnn_AvgPooling's head: event_fc on the mel-mean of the conv features, one launch each way."""

    def operands(self, p):
        Cl = self.eng.cfg[-1][0]
        return self.eng.dt, p.m, p.B * p.t_out, p.w_out, Cl, pad32(Cl), p.dy[-1]


class GruHead(_Head):
    """The CRNN's bidirectional GRU of engine.Hd hidden units between the mel-mean and event_fc (csrc/sed_gru.hip)."""
    tag = "gru"
    DIRS = ("", "_reverse")

    def operands(self, p):
        g, W = p.gru, 2 * self.eng.Hd
        return L.SED_F32, g["fc_m"], g["R"], 1, W, W, g["dhseq"]

    def plan(self, p, B, t, C, dev):
        """Buffers of the recurrent head; R = B*t rows."""
        super().plan(p, B, t, C, dev, 2 * self.eng.Hd)
        eng, lib, Hd = self.eng, self.eng.lib, self.eng.Hd
        if C % 4:
            raise ValueError("the GRU head needs a channel count that is a multiple of 4")
        f32 = dict(dtype=torch.float32, device=dev)
        R = B * t
        g = p.gru = dict(R=R)
        for name, rows, cols in (("m", R, C), ("gi", R, 6 * Hd), ("hseq", R, 2 * Hd), ("saved", R, 8 * Hd), ("fc_m", R, 2 * Hd),
                                 ("dhseq", R, 2 * Hd), ("dgi", R, 6 * Hd), ("dgh", R, 6 * Hd), ("wihT", C, 6 * Hd), ("dm", R, C),
                                 ("bhh", 2, 3 * Hd)):
            g[name] = torch.empty((rows, cols), **f32)
        n = lib.sed_gru_pack_elems(Hd)
        g["pack_f"] = torch.empty(n, dtype=eng.tdtype, device=dev)
        g["pack_b"] = torch.empty(n, dtype=eng.tdtype, device=dev)
        # split-K of the weight-gradient GEMMs (K = B*t rows): SED_GRU_KSPLIT, read here -- when the plan is built, like the other engine-side
        # SED_* knobs -- and kept with the plan, because the workspace below is sized for it
        g["ksplit"] = max(1, int(_os.environ.get("SED_GRU_KSPLIT", "64")))
        ws = max(lib.sed_gemm_nt_ws_floats(3 * Hd, C, g["ksplit"]), lib.sed_gemm_nt_ws_floats(3 * Hd, Hd, g["ksplit"]),
                 lib.sed_gemm_tn_ws_floats(3 * Hd, C, g["ksplit"]), lib.sed_gemm_tn_ws_floats(3 * Hd, Hd, g["ksplit"]))
        # the BPTT tail's weight / bias gradients come straight from the row-major gate gradients, all four products in one launch
        # (sed_gemm_tn_batch: reduction index on the rows, shifted hidden-state rows, column sums as a by-product): a workspace each
        g["ws4"] = [torch.empty(max(1, ws), **f32) for _ in range(4)]
        g["tn_desc"] = (L.GemmTnDesc * 4)()

    def _forward(self, p, P, feat, keep, training, update_running_stats):
        eng, lib, dt, st, Hd, g = self.eng, self.eng.lib, self.eng.dt, _stream(), self.eng.Hd, p.gru
        B, t = p.B, p.t_out
        Cl = eng.cfg[-1][0]
        R = g["R"]
        eng._k("sed_mel_mean_fwd", lib.sed_mel_mean_fwd, dt, L.ptr(feat), L.ptr(g["m"]), R, p.w_out, Cl, pad32(Cl), st)
        for d, sfx in enumerate(self.DIRS):
            eng._k("sed_gemm_nt", lib.sed_gemm_nt, dt, L.ptr(g["m"]), Cl, L.ptr(P["gru.weight_ih_l0" + sfx]), Cl,
                   L.ptr(P["gru.bias_ih_l0" + sfx]), g["gi"].data_ptr() + 4 * d * 3 * Hd, 6 * Hd, R, 3 * Hd, Cl, 1, None, st)
            g["bhh"][d].copy_(P["gru.bias_hh_l0" + sfx])
        eng._k("sed_gru_pack_weights", lib.sed_gru_pack_weights, dt, L.ptr(P["gru.weight_hh_l0"]),
               L.ptr(P["gru.weight_hh_l0_reverse"]), L.ptr(g["pack_f"]), L.ptr(g["pack_b"]), Hd, st)
        eng._k("sed_gru_seq_fwd", lib.sed_gru_seq_fwd, dt, L.ptr(g["gi"]), L.ptr(g["bhh"]), L.ptr(g["pack_f"]),
               L.ptr(g["hseq"]), L.ptr(g["saved"]) if keep else None, B, t, Hd, st)
        return g["hseq"]

    def _backward(self, p, P, G, dfeat, done):
        eng, lib, dt, st, Hd, g = self.eng, self.eng.lib, self.eng.dt, _stream(), self.eng.Hd, p.gru
        B, t = p.B, p.t_out
        Cl = eng.cfg[-1][0]
        R = g["R"]
        eng._k("sed_gru_seq_bwd", lib.sed_gru_seq_bwd, dt, L.ptr(g["dhseq"]), L.ptr(g["hseq"]), L.ptr(g["saved"]),
               L.ptr(g["pack_b"]), L.ptr(g["dgi"]), L.ptr(g["dgh"]), B, t, Hd, st)
        ks = max(1, min(g["ksplit"], R // 256))
        # dW_ih = dgi_d^T . m (+ db_ih = column sums of dgi_d);  dW_hh = dgh_d^T . h_prev (+ db_hh), both directions: ONE product
        # launch and ONE reduction launch.  h_prev = hseq shifted by one step inside each clip's sequence (the forward direction looks
        # one step back, the reverse one step ahead)
        ds = g["tn_desc"]
        for d, sfx in enumerate(self.DIRS):
            for j, (a, b, ldb, wname, bname, n, shift) in enumerate((
                    (g["dgi"].data_ptr() + 4 * d * 3 * Hd, L.ptr(g["m"]), Cl, "gru.weight_ih_l0", "gru.bias_ih_l0", Cl, 0),
                    (g["dgh"].data_ptr() + 4 * d * 3 * Hd, g["hseq"].data_ptr() + 4 * d * Hd, 2 * Hd, "gru.weight_hh_l0", "gru.bias_hh_l0", Hd,
                     1 if d == 0 else -1))):
                e = ds[2 * d + j]
                e.A, e.B, e.C, e.colsum = a, b, L.ptr(G[wname + sfx]), L.ptr(G[bname + sfx])
                e.workspace = L.ptr(g["ws4"][2 * d + j]) if ks > 1 else None
                e.lda, e.ldb, e.ldc, e.M, e.N, e.K, e.seq, e.shift, e.ksplit = 6 * Hd, ldb, n, 3 * Hd, n, R, t, shift, ks
        eng._k("sed_gemm_tn_batch", lib.sed_gemm_tn_batch, dt, _C.cast(ds, _C.c_void_p), 4, st)
        for d, sfx in enumerate(self.DIRS):
            eng._k("sed_transpose_shift", lib.sed_transpose_shift, L.ptr(P["gru.weight_ih_l0" + sfx]), Cl,
                   g["wihT"].data_ptr() + 4 * d * 3 * Hd, 6 * Hd, 3 * Hd, Cl, 3 * Hd, 0, st)
        done("gru")
        # dm = dgi . [W_ih ; W_ih_reverse]  (both directions in one K = 6*Hd product), then back through the mel mean
        eng._k("sed_gemm_nt", lib.sed_gemm_nt, dt, L.ptr(g["dgi"]), 6 * Hd, L.ptr(g["wihT"]), 6 * Hd, None, L.ptr(g["dm"]),
               Cl, R, Cl, 6 * Hd, 1, None, st)
        eng._k("sed_mel_mean_bwd", lib.sed_mel_mean_bwd, dt, L.ptr(g["dm"]), L.ptr(dfeat), R, p.w_out, Cl, pad32(Cl), st)


class SaHead(_Head):
    """Csa_AvgPooling's head: cfg.layers self-attention encoder layers between the mel-mean and event_fc (SaConfig describes the
    options).  Per option, what replaces the default launches: dropout the _drop entries; a window sed_mhsa_fwd_win / sed_mhsa_bwd_win in
    the places of the plain / _drop core launches, no new buffers; rel_pos sed_relpos_expand + sed_mhsa_fwd_rel in the place of the
    core launch, sed_mhsa_bwd_rel + sed_relpos_fold into G["rel_pos*.weight"] in the backward -- the map, the per-layer distance tables
    and the workspace belong to the plan.  cfg.norm_first: the pre-LN chain (_plan_chain, _forward_pre, _backward_pre) -- one
    sed_resid_layernorm_fwd / _bwd per LayerNorm, each doing the previous sub-layer's residual add (forward) or adding its input gradient to
    the running stream gradient in place (backward), around the same sub-layer launches; no torch add on that path."""
    tag = "sa"

    def __init__(self, eng, cfg: SaConfig):
        super().__init__(eng)
        self.cfg = cfg
        self.act = L.FFN_ACT[cfg.activation]
        # the window's sides as the C entries take them
        self._win = None if cfg.window is None else tuple(L.WIN_UNBOUNDED if v is None else min(v, L.WIN_UNBOUNDED) for v in cfg.window)
        # the effective (left, right): what the relative-position entries take where no window is set
        self._win_sides = self._win if self._win is not None else (L.WIN_UNBOUNDED, L.WIN_UNBOUNDED)
        self.seed = (torch.initial_seed() if cfg.dropout_seed is None else cfg.dropout_seed) & 0xFFFFFFFFFFFFFFFF
        self._drop_state = None              # (4,) int32 on the device holding the uint32 words, made with the first plan (on its device)
        self._drop_dev = "cuda"
        self._drop_host = [self.seed & 0xFFFFFFFF, self.seed >> 32, 0, 0]

    # ---- the dropout state: (seed_lo, seed_hi, step, 0), uint32 words in an int32 device tensor ---------------------------------
    @property
    def drop_state(self) -> torch.Tensor:
        """The (4,) device tensor the NEXT training forward's masks come from (that forward ends by adding 1 to the step word)."""
        if self._drop_state is None:
            words = [w - (1 << 32) if w >= (1 << 31) else w for w in self._drop_host]
            self._drop_state = torch.tensor(words, dtype=torch.int32, device=self._drop_dev)
        return self._drop_state

    def drop_state_words(self):
        """the four uint32 words as Python ints (synchronises)"""
        if self._drop_state is None:
            return list(self._drop_host)
        return [int(v) & 0xFFFFFFFF for v in self._drop_state.cpu().tolist()]

    def set_drop_state(self, words) -> None:
        """overwrite the state in place (a captured graph keeps reading the same tensor)"""
        words = [int(w) & 0xFFFFFFFF for w in words]
        if len(words) != 4:
            raise ValueError("the dropout state is four uint32 words (seed_lo, seed_hi, step, 0)")
        self._drop_host = words
        if self._drop_state is not None:
            self._drop_state.copy_(torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32))

    def operands(self, p):
        g, C = p.sa, self.eng.cfg[-1][0]
        return L.SED_F32, g["fc_m"], g["R"], 1, C, C, g["dh"]

    def plan(self, p, B, t, C, dev):
        """Buffers of the self-attention head (every one allocated here: a captured step allocates nothing); R = B*t rows.  What a
        layer's backward reads of its forward is kept per layer (g["layers"]); the gradients in flight are shared by the layers."""
        super().plan(p, B, t, C, dev)
        c, lib = self.cfg, self.eng.lib
        Hh, D, kc = c.heads, c.ffn, c.conv_kernel
        f32 = dict(dtype=torch.float32, device=dev)
        R = B * t
        g = p.sa = dict(R=R)
        for name, cols in (("m", C), ("fc_m", C), ("dh", C), ("dres", C), ("dctx", C), ("dqkv", 3 * C), ("dm", C)):
            g[name] = torch.empty((R, cols), **f32)
        g["layers"] = []
        pre = c.norm_first
        for _ in range(c.layers):
            ly = {name: torch.empty((R, cols), **f32) for name, cols in (("qkv", 3 * C), ("ctx", C), ("a", C))
                  + (() if pre else (("h", C), ("stats", 2)))}
            ly["lse"] = torch.empty((B, Hh, t), **f32)
            if D:
                ly.update({name: torch.empty((R, cols), **f32) for name, cols in (("u", D), ("f", C)) + (() if pre else (("h2", C), ("stats2", 2)))})
            if c.macaron:
                ly.update({name: torch.empty((R, cols), **f32) for name, cols in (("mu", D), ("mf", C))})
            if kc:
                # the convolution module: the GLU's input and output, the depthwise output, the activation, the module's output, the
                # residual LayerNorm's output and statistics, and the BatchNorm's per-channel vectors (Cp = C)
                ly.update({name: torch.empty((R, cols), **f32) for name, cols in (("cg", 2 * C), ("cv", C), ("cz", C), ("cs", C), ("co", C))
                           + (() if pre else (("hc", C), ("stats3", 2)))})
                ly.update({name: torch.empty(C, **f32) for name in ("cscale", "cshift", "cmean", "cinvstd")})
            g["layers"].append(ly)
        if pre:
            self._plan_chain(g, R, C, f32)
        g["h"] = g["chain"][-1]["y"] if pre else self.layer_out(g["layers"][-1])          # what event_fc (and att_fc) read
        g["woT"] = torch.empty((C, C), **f32)
        g["winT"] = torch.empty((C, 3 * C), **f32)
        if D:
            # the FFN backward: a and the hidden gradient (da, then du in place), the gradient behind the FFN, the transposed weights
            g["ffa"], g["fda"] = torch.empty((R, D), **f32), torch.empty((R, D), **f32)
            g["dh1"] = torch.empty((R, C), **f32)
            g["w2T"], g["w1T"] = torch.empty((D, C), **f32), torch.empty((C, D), **f32)
        if kc:
            # shared by the layers: the statistics partials of the forward and the backward, the BatchNorm backward's coefficients, the
            # gradients of the activation (ds, then gz in place) and of g, the filter-gradient workspace, the transposed pointwise weights
            g["cpart"] = torch.empty(max(1, lib.sed_dwconv_glu_fwd_ws_floats(B, t, C)), **f32)
            g["cbpart"] = torch.empty((max(1, lib.sed_bn_silu_bwd_nparts(R)), 2, C), **f32)
            g["ccoef"] = torch.empty((3, C), **f32)
            g["cds"], g["cdg"], g["dhc"] = torch.empty((R, C), **f32), torch.empty((R, 2 * C), **f32), torch.empty((R, C), **f32)
            g["cw_ws"] = torch.empty(max(1, lib.sed_dwconv_glu_bwd_ws_floats(B, t, C, kc)), **f32)
            g["cw2T"], g["cw1T"] = torch.empty((C, C), **f32), torch.empty((2 * C, C), **f32)
        if c.dropout:
            if self._drop_state is None:
                self._drop_dev = dev
            _ = self.drop_state                      # made here, never inside a captured step
        if c.dropout or c.macaron:
            # the gradient of a sub-layer's output a (da = s m sd dres: dropout, or a residual weight other than 1)
            g["da"] = torch.empty((R, C), **f32)
        if c.dropout:
            # the state the plan's last training forward drew its masks from (what its backward regenerates them from)
            g["rng"] = torch.zeros(4, dtype=torch.int32, device=dev)
        g["pe"] = None
        if c.pos_encoding:
            # the standard table, built on the host in float64 and rounded once to fp32: pe[i][2j] = sin(i / 10000^(2j/C)), pe[i][2j+1] = cos(.)
            i = torch.arange(t, dtype=torch.float64)[:, None]
            j2 = (torch.arange(C) // 2 * 2).to(torch.float64)[None, :]
            ang = i / torch.pow(torch.tensor(10000.0, dtype=torch.float64), j2 / C)
            g["pe"] = torch.where((torch.arange(C) % 2 == 0)[None, :], torch.sin(ang), torch.cos(ang)).to(torch.float32).to(dev)
        g["core_ws"] = torch.empty(max(1, lib.sed_mhsa_bwd_ws_floats(B, t, Hh, C // Hh)), **f32)
        if c.rel_pos is not None:
            # the bucket map over the 2t - 1 distances (checked here, on the host: the kernels do not), a distance table and its gradient
            # per layer, and the core backward's workspace with the per-wave diagonal partials behind D
            m = np.ascontiguousarray(c.rel_pos_map(c.rel_pos, t))
            L.check(lib.sed_relpos_map_check(m.ctypes.data, c.rel_pos_buckets(c.rel_pos), t), "sed_relpos_map_check")
            g["rel_map"] = torch.from_numpy(m).to(dev)
            for ly in g["layers"]:
                ly["rel"], ly["drel"] = torch.empty((Hh, 2 * t - 1), **f32), torch.empty((Hh, 2 * t - 1), **f32)
            g["core_ws"] = torch.empty(max(1, lib.sed_mhsa_bwd_rel_ws_floats(B, t, Hh, C // Hh, *self._win_sides)), **f32)
        g["ln_ws"] = torch.empty(max(1, (lib.sed_resid_layernorm_bwd_ws_floats if pre else lib.sed_add_layernorm_bwd_ws_floats)(R, C)), **f32)
        # split-K of the weight-gradient products (K = R rows), as the recurrent head's tail: SED_GRU_KSPLIT, read with the plan
        g["ksplit"] = max(1, int(_os.environ.get("SED_GRU_KSPLIT", "64")))
        tn = [lib.sed_gemm_tn_ws_floats(3 * C, C, g["ksplit"])]
        if D:
            tn += [lib.sed_gemm_tn_ws_floats(C, D, g["ksplit"]), lib.sed_gemm_tn_ws_floats(D, C, g["ksplit"])]
        if kc:
            tn += [lib.sed_gemm_tn_ws_floats(2 * C, C, g["ksplit"])]
        g["tn_ws"] = torch.empty(max(1, max(tn)), **f32)

    def layer_out(self, ly):
        """the output of a layer, given its buffers: the next layer's input, or what event_fc reads (norm_first: the closing norm's
        output, or the residual stream behind the layer's last add)"""
        if self.cfg.norm_first:
            return ly["out"]
        return ly["h2"] if self.cfg.ffn else ly["hc"] if self.cfg.conv_kernel else ly["h"]

    def _plan_chain(self, g, R, C, f32):
        """norm_first: the chain of LayerNorm launches, one node per launch in forward order.  A node normalises the residual stream
        node["x"]: with node["add"] = (a, s, site, l) it first forms x = src + s m sd a in its own buffer (the previous sub-layer's add,
        across a layer boundary where there is no closing norm), else x is src itself -- the mel-mean rows, or a closing norm's
        output.  node["y"], node["stats"]: the LayerNorm's output (the sub-layer's input) and statistics; node["sub"] = (kind, module,
        layer, buffers) of the sub-layer that reads y, None for a closing norm; node["new"]: x is a new stream (no gradient arrives
        on it from later adds other than through this node)."""
        c = self.cfg
        chain, src, add = [], g["m"], None
        new = lambda cols: torch.empty((R, cols), **f32)
        def node(norm, sub):
            nonlocal src, add
            n = dict(norm=norm, src=src, add=add, x=new(C) if add is not None else src, y=new(C), stats=new(2), sub=sub)
            chain.append(n)
            src, add = n["x"], None
            return n
        for l, ly in enumerate(g["layers"]):
            for kind, mod, norm, s, site in c.sublayers(l):
                node(norm, (kind, mod, l, ly))
                add = (ly[{"mac": "mf", "attn": "a", "conv": "co", "ffn": "f"}[kind]], s, site, l)
            if c.has_out_norm(l):
                n = node(c.out_name(l), None)
                src = ly["out"] = n["y"]
            else:
                ly["out"] = None                       # (the stream behind the layer: the next node's x, set below)
        for i, n in enumerate(chain):
            if n["sub"] is not None and n["sub"][0] == ("mac" if c.macaron else "attn") and n["sub"][2] > 0:
                prev = g["layers"][n["sub"][2] - 1]
                if prev["out"] is None:
                    prev["out"] = n["x"]
        g["chain"] = chain
        g["dn"], g["ds"] = new(C), [new(C), new(C)]     # the gradient of a node's y; the stream gradient (two: a closing norm's dy and dx)

    def _add_ln_fwd(self, g, x, a, gamma, beta, y, stats, R, C, sid):
        """y = LayerNorm(x + a); sid: the dropout stream of a, None = no dropout (the plain launch)"""
        sfx, opts = ("", ()) if sid is None else ("_drop", (self.cfg.dropout, L.ptr(g["rng"]), sid))
        self.eng._k("sed_add_layernorm_fwd" + sfx, getattr(self.eng.lib, "sed_add_layernorm_fwd" + sfx), L.ptr(x), L.ptr(a), L.ptr(gamma),
                    L.ptr(beta), L.ptr(y), L.ptr(stats), R, C, LN_EPS, *opts, _stream())

    def _add_ln_bwd(self, g, dy, x, a, gamma, stats, dgamma, dbeta, R, C, sid):
        """the residual LayerNorm's backward: g["dres"] = the gradient of x; returns the gradient of a (g["dres"], or g["da"] = m s dres
        under dropout stream sid)"""
        eng, lib, st = self.eng, self.eng.lib, _stream()
        if sid is None:
            eng._k("sed_add_layernorm_bwd", lib.sed_add_layernorm_bwd, L.ptr(dy), L.ptr(x), L.ptr(a), L.ptr(gamma), L.ptr(stats),
                   L.ptr(g["dres"]), L.ptr(dgamma), L.ptr(dbeta), L.ptr(g["ln_ws"]), R, C, st)
            return g["dres"]
        eng._k("sed_add_layernorm_bwd_drop", lib.sed_add_layernorm_bwd_drop, L.ptr(dy), L.ptr(x), L.ptr(a), L.ptr(gamma), L.ptr(stats),
               L.ptr(g["dres"]), L.ptr(g["da"]), L.ptr(dgamma), L.ptr(dbeta), L.ptr(g["ln_ws"]), R, C, self.cfg.dropout, L.ptr(g["rng"]),
               sid, st)
        return g["da"]

    def _lin_dx(self, dy, W, wT, dx, rows, n_out, n_in):
        """dx[rows][n_in] = dy[rows][n_out] . W[n_out][n_in], through W's transpose in wT[n_in][n_out]"""
        eng, lib, st = self.eng, self.eng.lib, _stream()
        eng._k("sed_transpose_shift", lib.sed_transpose_shift, L.ptr(W), n_in, L.ptr(wT), n_out, n_out, n_in, n_out, 0, st)
        eng._k("sed_gemm_nt", lib.sed_gemm_nt, eng.dt, L.ptr(dy), n_out, L.ptr(wT), n_out, None, L.ptr(dx), n_in, rows, n_in, n_out, 1,
               None, st)

    def _lin_dw(self, dy, x, dW, db, rows, n_out, n_in, t, ks, ws):
        """dW[n_out][n_in] = dy^T . x over the rows, db = the column sums of dy (split-K ks with the workspace ws)"""
        self.eng._k("sed_gemm_tn", self.eng.lib.sed_gemm_tn, self.eng.dt, L.ptr(dy), n_out, L.ptr(x), n_in, L.ptr(dW), n_in, L.ptr(db),
                    n_out, n_in, rows, t, 0, ks, ws, _stream())

    def _mhsa_opts(self, g, ly, l, drop):
        """The core entry of layer l, the same for the forward and the backward: its suffix and its arguments between the sizes and
        the tables' gradient / the stream.  A table takes _rel (with the window, or both sides unbounded), else a window _win, else
        dropout _drop, else the plain entry."""
        rng = L.ptr(g["rng"]) if drop else None
        if self.cfg.rel_pos is not None:
            return "_rel", (*self._win_sides, drop, rng, 8 * l + 0, L.ptr(ly["rel"]))
        if self._win is not None:
            return "_win", (*self._win, drop, rng, 8 * l + 0)
        if drop:
            return "_drop", (drop, rng, 8 * l + 0)
        return "", ()

    def _mhsa_fwd(self, g, ly, l, keep, drop):
        """ly["qkv"] -> ly["ctx"]; lse is kept for a backward (keep) and wherever the masks are drawn"""
        (B, Hh, t), C = ly["lse"].shape, ly["ctx"].shape[1]
        sfx, opts = self._mhsa_opts(g, ly, l, drop)
        self.eng._k("sed_mhsa_fwd" + sfx, getattr(self.eng.lib, "sed_mhsa_fwd" + sfx), self.eng.dt, L.ptr(ly["qkv"]), L.ptr(ly["ctx"]),
                    L.ptr(ly["lse"]) if keep or drop else None, B, t, Hh, C // Hh, *opts, _stream())

    def _mhsa_bwd(self, g, ly, l, drop):
        """g["dctx"] -> g["dqkv"] (and ly["drel"] where there is a table)"""
        (B, Hh, t), C = ly["lse"].shape, ly["ctx"].shape[1]
        sfx, opts = self._mhsa_opts(g, ly, l, drop)
        if sfx == "_rel":
            opts += (L.ptr(ly["drel"]),)
        self.eng._k("sed_mhsa_bwd" + sfx, getattr(self.eng.lib, "sed_mhsa_bwd" + sfx), self.eng.dt, L.ptr(ly["qkv"]), L.ptr(ly["ctx"]),
                    L.ptr(g["dctx"]), L.ptr(ly["lse"]), L.ptr(g["dqkv"]), L.ptr(g["core_ws"]), B, t, Hh, C // Hh, *opts, _stream())

    def _conv_forward(self, p, P, l, ly, keep, training, update_running_stats):
        """The convolution module of layer l behind attn_norm: ly["h"] -> ly["hc"].  keep: keep what a backward reads;
        training: batch statistics (and the running update) instead of the running statistics."""
        g, C, R = p.sa, self.eng.cfg[-1][0], p.sa["R"]
        cn = self.cfg.conv_names(l)[1]
        self._conv_inner_forward(p, P, l, ly, ly["h"], keep, training, update_running_stats)
        self._add_ln_fwd(g, ly["h"], ly["co"], P[cn + ".weight"], P[cn + ".bias"], ly["hc"], ly["stats3"] if keep else None, R, C,
                         8 * l + 2 if training and self.cfg.dropout else None)

    def _conv_inner_forward(self, p, P, l, ly, xin, keep, training, update_running_stats):
        """The inner convolution module of layer l between given buffers: xin -> ly["co"] (pointwise conv, GLU + depthwise conv,
        BatchNorm, SiLU, pointwise conv)."""
        eng, lib, dt, st, g, kc = self.eng, self.eng.lib, self.eng.dt, _stream(), p.sa, self.cfg.conv_kernel
        B, t, C, R = p.B, p.t_out, eng.cfg[-1][0], p.sa["R"]
        cm, cn = self.cfg.conv_names(l)
        eng._k("sed_gemm_nt", lib.sed_gemm_nt, dt, L.ptr(xin), C, L.ptr(P[cm + ".pointwise1.weight"]), C,
               L.ptr(P[cm + ".pointwise1.bias"]), L.ptr(ly["cg"]), 2 * C, R, 2 * C, C, 1, None, st)
        eng._k("sed_dwconv_glu_fwd", lib.sed_dwconv_glu_fwd, L.ptr(ly["cg"]), L.ptr(P[cm + ".depthwise.weight"]),
               L.ptr(P[cm + ".depthwise.bias"]), L.ptr(ly["cz"]), L.ptr(ly["cv"]) if keep else None,
               L.ptr(g["cpart"]) if training else None, B, t, C, kc, st)
        if training:
            rm = P[cm + ".bn.running_mean"] if update_running_stats else None
            rv = P[cm + ".bn.running_var"] if update_running_stats else None
            eng._k("sed_bn_train_finalize", lib.sed_bn_train_finalize, L.ptr(g["cpart"]), lib.sed_dwconv_nparts(B, t), float(R),
                   L.ptr(P[cm + ".bn.weight"]), L.ptr(P[cm + ".bn.bias"]), L.ptr(rm), L.ptr(rv), BN_MOMENTUM, BN_EPS,
                   L.ptr(ly["cscale"]), L.ptr(ly["cshift"]), L.ptr(ly["cmean"]), L.ptr(ly["cinvstd"]), C, C, st)
        else:
            eng._k("sed_bn_eval_coeffs", lib.sed_bn_eval_coeffs, L.ptr(P[cm + ".bn.weight"]), L.ptr(P[cm + ".bn.bias"]),
                   L.ptr(P[cm + ".bn.running_mean"]), L.ptr(P[cm + ".bn.running_var"]), BN_EPS, L.ptr(ly["cscale"]),
                   L.ptr(ly["cshift"]), C, C, st)
        eng._k("sed_bn_silu_fwd", lib.sed_bn_silu_fwd, L.ptr(ly["cz"]), L.ptr(ly["cscale"]), L.ptr(ly["cshift"]), L.ptr(ly["cs"]), R, C, st)
        eng._k("sed_gemm_nt", lib.sed_gemm_nt, dt, L.ptr(ly["cs"]), C, L.ptr(P[cm + ".pointwise2.weight"]), C,
               L.ptr(P[cm + ".pointwise2.bias"]), L.ptr(ly["co"]), C, R, C, C, 1, None, st)

    def _conv_backward(self, p, P, G, l, ly, gcur, eval_bwd, ks, ws, done):
        """Backward of layer l's convolution module: gcur = the gradient of ly["hc"]; returns the gradient of ly["h"] (g["dhc"])."""
        eng, lib, st, g, kc = self.eng, self.eng.lib, _stream(), p.sa, self.cfg.conv_kernel
        B, t, C, R = p.B, p.t_out, eng.cfg[-1][0], p.sa["R"]
        cm, cn = self.cfg.conv_names(l)
        ga = self._add_ln_bwd(g, gcur, ly["h"], ly["co"], P[cn + ".weight"], ly["stats3"], G[cn + ".weight"], G[cn + ".bias"], R, C,
                              8 * l + 2 if p.trained and self.cfg.dropout else None)
        done(cn)
        self._conv_inner_backward(p, P, G, l, ly, ga, ly["h"], g["dhc"], eval_bwd, ks, ws, done)
        g["dhc"].add_(g["dres"])
        return g["dhc"]

    def _conv_inner_backward(self, p, P, G, l, ly, ga, xin, dxin, eval_bwd, ks, ws, done):
        """Backward of layer l's inner convolution module: ga = the gradient of ly["co"], xin the module's input -> its parameters'
        gradients and dxin, the gradient of xin through the module (no residual)."""
        eng, lib, st, g, kc = self.eng, self.eng.lib, _stream(), p.sa, self.cfg.conv_kernel
        B, t, C, R = p.B, p.t_out, eng.cfg[-1][0], p.sa["R"]
        cm, cn = self.cfg.conv_names(l)
        w1, w2 = cm + ".pointwise1.weight", cm + ".pointwise2.weight"
        # ds = ga . pointwise2.weight;  d pointwise2.weight = ga^T . s, its bias gradient the column sums of ga (ga = dres, or m s dres
        # under dropout: the gradient of the module's output)
        self._lin_dx(ga, P[w2], g["cw2T"], g["cds"], R, C, C)
        self._lin_dw(ga, ly["cs"], G[w2], G[cm + ".pointwise2.bias"], R, C, C, t, ks, ws)
        # through the SiLU (gz over ds) and the BatchNorm: statistics, the finalisation, then dz = ca gz + cb z + cc on load
        if eval_bwd:
            eng._k("sed_bn_eval_stats", lib.sed_bn_eval_stats, L.ptr(P[cm + ".bn.running_mean"]), L.ptr(P[cm + ".bn.running_var"]), BN_EPS,
                   L.ptr(ly["cmean"]), L.ptr(ly["cinvstd"]), C, C, st)
        nparts = lib.sed_bn_silu_bwd_nparts(R)
        eng._k("sed_bn_silu_bwd_reduce", lib.sed_bn_silu_bwd_reduce, L.ptr(g["cds"]), L.ptr(ly["cz"]), L.ptr(ly["cscale"]),
               L.ptr(ly["cshift"]), L.ptr(ly["cmean"]), L.ptr(ly["cinvstd"]), L.ptr(g["cds"]), L.ptr(g["cbpart"]), R, C, st)
        ca, cb, cc = g["ccoef"][0], g["ccoef"][1], g["ccoef"][2]
        if eval_bwd:
            eng._k("sed_bn_eval_bwd_finalize", lib.sed_bn_eval_bwd_finalize, L.ptr(g["cbpart"]), nparts, L.ptr(P[cm + ".bn.weight"]),
                   L.ptr(ly["cmean"]), L.ptr(ly["cinvstd"]), L.ptr(G[cm + ".bn.weight"]), L.ptr(G[cm + ".bn.bias"]), L.ptr(ca), L.ptr(cb),
                   L.ptr(cc), C, C, st)
        else:
            eng._k("sed_bn_bwd_finalize", lib.sed_bn_bwd_finalize, L.ptr(g["cbpart"]), nparts, float(R), L.ptr(P[cm + ".bn.weight"]),
                   L.ptr(ly["cmean"]), L.ptr(ly["cinvstd"]), L.ptr(G[cm + ".bn.weight"]), L.ptr(G[cm + ".bn.bias"]), L.ptr(ca), L.ptr(cb),
                   L.ptr(cc), C, C, st)
        eng._k("sed_dwconv_glu_bwd", lib.sed_dwconv_glu_bwd, L.ptr(g["cds"]), L.ptr(ly["cz"]), L.ptr(ca), L.ptr(cb), L.ptr(cc),
               L.ptr(ly["cv"]), L.ptr(ly["cg"]), L.ptr(P[cm + ".depthwise.weight"]), L.ptr(g["cdg"]), L.ptr(G[cm + ".depthwise.weight"]),
               L.ptr(G[cm + ".depthwise.bias"]), L.ptr(g["cw_ws"]), B, t, C, kc, st)
        # d pointwise1.weight = dg^T . h, its bias gradient the column sums of dg;  dh = dg . pointwise1.weight + dres (the residual)
        self._lin_dw(g["cdg"], xin, G[w1], G[cm + ".pointwise1.bias"], R, 2 * C, C, t, ks, ws)
        done(cm)
        self._lin_dx(g["cdg"], P[w1], g["cw1T"], dxin, R, 2 * C, C)

    # ---- the sub-layers between given buffers: the post-LN loop (_forward, _backward) and the pre-LN chain (_forward_pre, _backward_pre)
    # launch them from here, as they do the inner convolution module ---------------------------------------------------------------------
    def _attn_forward(self, p, P, l, ly, mod, xin, keep, drop):
        """The attention sub-layer of layer l (module mod): xin -> ly["qkv"] -> ly["ctx"] -> ly["a"]"""
        c, eng, lib, dt, st, g = self.cfg, self.eng, self.eng.lib, self.eng.dt, _stream(), p.sa
        Hh, t, C, R = c.heads, p.t_out, eng.cfg[-1][0], p.sa["R"]
        eng._k("sed_gemm_nt", lib.sed_gemm_nt, dt, L.ptr(xin), C, L.ptr(P[mod + ".in_proj_weight"]), C, L.ptr(P[mod + ".in_proj_bias"]),
               L.ptr(ly["qkv"]), 3 * C, R, 3 * C, C, 1, None, st)
        if c.rel_pos is not None:
            eng._k("sed_relpos_expand", lib.sed_relpos_expand, L.ptr(P[c.rel_name(l) + ".weight"]), L.ptr(g["rel_map"]),
                   L.ptr(ly["rel"]), Hh, c.rel_pos_buckets(c.rel_pos), t, st)
        self._mhsa_fwd(g, ly, l, keep, drop)
        eng._k("sed_gemm_nt", lib.sed_gemm_nt, dt, L.ptr(ly["ctx"]), C, L.ptr(P[mod + ".out_proj.weight"]), C,
               L.ptr(P[mod + ".out_proj.bias"]), L.ptr(ly["a"]), C, R, C, C, 1, None, st)

    def _attn_backward(self, p, P, G, l, ly, mod, ga, xin, dxin, drop, ks, ws, done):
        """Backward of layer l's attention sub-layer: ga = the gradient of ly["a"] (dres, or m s dres under dropout), xin the sub-layer's
        input -> its parameters' gradients and dxin, the gradient of xin through the sub-layer (no residual)."""
        c, eng, lib, st, g = self.cfg, self.eng, self.eng.lib, _stream(), p.sa
        Hh, t, C, R = c.heads, p.t_out, eng.cfg[-1][0], p.sa["R"]
        # d out_proj.weight = ga^T . ctx, d out_proj.bias = column sums of ga;  dctx = ga . out_proj.weight
        self._lin_dw(ga, ly["ctx"], G[mod + ".out_proj.weight"], G[mod + ".out_proj.bias"], R, C, C, t, ks, ws)
        self._lin_dx(ga, P[mod + ".out_proj.weight"], g["woT"], g["dctx"], R, C, C)
        self._mhsa_bwd(g, ly, l, drop)
        if c.rel_pos is not None:
            # ly["rel"] is the table this layer's forward read (the weights do not change between a step's forward and backward)
            rn = c.rel_name(l)
            eng._k("sed_relpos_fold", lib.sed_relpos_fold, L.ptr(ly["drel"]), L.ptr(g["rel_map"]), L.ptr(G[rn + ".weight"]), Hh,
                   c.rel_pos_buckets(c.rel_pos), t, st)
            done(rn)
        # d in_proj_weight = dqkv^T . x', d in_proj_bias = column sums of dqkv;  dx' = dqkv . in_proj_weight
        self._lin_dw(g["dqkv"], xin, G[mod + ".in_proj_weight"], G[mod + ".in_proj_bias"], R, 3 * C, C, t, ks, ws)
        done(mod)
        self._lin_dx(g["dqkv"], P[mod + ".in_proj_weight"], g["winT"], dxin, R, 3 * C, C)

    def _ffn_fwd(self, g, P, fn, x, f, u, keep, drop, sid, R, C, D):
        """f = ffn(x) of module fn, both products and the activation in one launch; u for a backward (and wherever the hidden mask is
        drawn); sid: the hidden activation's stream"""
        eng, lib = self.eng, self.eng.lib
        sfx, opts = ("_drop", (drop, L.ptr(g["rng"]), sid)) if drop else ("", ())
        eng._k("sed_ffn_fwd" + sfx, getattr(lib, "sed_ffn_fwd" + sfx), eng.dt, self.act, L.ptr(x), L.ptr(P[fn + ".linear1.weight"]),
               L.ptr(P[fn + ".linear1.bias"]), L.ptr(P[fn + ".linear2.weight"]), L.ptr(P[fn + ".linear2.bias"]), L.ptr(f),
               L.ptr(u) if keep or drop else None, R, C, D, *opts, _stream())

    def _ffn_backward(self, p, P, G, fn, ga, xin, u, sid, dxin, drop, ks, ws, done):
        """Backward of the FFN module fn: ga = the gradient of its output (dres, or m s dres under dropout), xin its input, u its kept
        hidden pre-activation, sid the hidden activation's stream -> its parameters' gradients and dxin, the gradient of xin through
        the module (no residual)."""
        eng, lib, st, g = self.eng, self.eng.lib, _stream(), p.sa
        t, C, R, D = p.t_out, eng.cfg[-1][0], p.sa["R"], self.cfg.ffn
        w1, w2 = fn + ".linear1.weight", fn + ".linear2.weight"
        # da = ga . w2, then a = act(u) and du = da act'(u) (du over da; under dropout a = m s act(u), du = da m s act'(u))
        self._lin_dx(ga, P[w2], g["w2T"], g["fda"], R, C, D)
        if drop:
            eng._k("sed_ffn_act_bwd_drop", lib.sed_ffn_act_bwd_drop, self.act, L.ptr(u), L.ptr(g["fda"]), L.ptr(g["ffa"]),
                   L.ptr(g["fda"]), R, D, drop, L.ptr(g["rng"]), sid, st)
        else:
            eng._k("sed_ffn_act_bwd", lib.sed_ffn_act_bwd, self.act, L.ptr(u), L.ptr(g["fda"]), L.ptr(g["ffa"]),
                   L.ptr(g["fda"]), R * D, st)
        # d linear2.weight = ga^T . a, d linear1.weight = du^T . x, the biases' gradients their column sums;  dx = du . w1
        self._lin_dw(ga, g["ffa"], G[w2], G[fn + ".linear2.bias"], R, C, D, t, ks, ws)
        self._lin_dw(g["fda"], xin, G[w1], G[fn + ".linear1.bias"], R, D, C, t, ks, ws)
        done(fn)
        self._lin_dx(g["fda"], P[w1], g["w1T"], dxin, R, D, C)

    def _forward(self, p, P, feat, keep, training, update_running_stats):
        c, eng, lib, dt, st, g = self.cfg, self.eng, self.eng.lib, self.eng.dt, _stream(), p.sa
        D = c.ffn
        B, t = p.B, p.t_out
        C = eng.cfg[-1][0]
        R = g["R"]
        drop = c.dropout if training else 0.0                # training-mode forwards only (a kept eval forward never drops)
        if drop:
            g["rng"].copy_(self.drop_state)                  # this forward's masks, and its backward's
        eng._k("sed_mel_mean_fwd", lib.sed_mel_mean_fwd, dt, L.ptr(feat), L.ptr(g["m"]), R, p.w_out, C, pad32(C), st)
        if g["pe"] is not None:
            g["m"].view(B, t, C).add_(g["pe"])          # x' = x + pe[frame], in place: the residual and the projections read x'
        if c.norm_first:
            return self._forward_pre(p, P, keep, training, update_running_stats, drop)
        xin = g["m"]
        for l, ly in enumerate(g["layers"]):
            an, nn_, fn, fnn = c.layer_names(l)
            self._attn_forward(p, P, l, ly, an, xin, keep, drop)
            self._add_ln_fwd(g, xin, ly["a"], P[nn_ + ".weight"], P[nn_ + ".bias"], ly["h"], ly["stats"] if keep else None, R, C,
                             8 * l + 1 if drop else None)
            xin = ly["h"]
            if c.conv_kernel:
                self._conv_forward(p, P, l, ly, keep, training, update_running_stats)
                xin = ly["hc"]
            if D:
                self._ffn_fwd(g, P, fn, xin, ly["f"], ly["u"], keep, drop, 8 * l + 3, R, C, D)       # h2 = LayerNorm(h + ffn(h))
                self._add_ln_fwd(g, xin, ly["f"], P[fnn + ".weight"], P[fnn + ".bias"], ly["h2"], ly["stats2"] if keep else None, R, C,
                                 8 * l + 4 if drop else None)
                xin = ly["h2"]
        if drop:
            self.drop_state[2:3].add_(1)                     # the next training forward draws new masks (captured with the step)
        return g["h"]

    def _backward(self, p, P, G, dfeat, done):
        c, eng, lib, st, g = self.cfg, self.eng, self.eng.lib, _stream(), p.sa
        D = c.ffn
        C = eng.cfg[-1][0]
        R = g["R"]
        ks = max(1, min(g["ksplit"], R // 256))
        ws = L.ptr(g["tn_ws"]) if ks > 1 else None
        gcur = g["dh"]                                   # the gradient of the current layer's output
        drop = c.dropout if p.trained else 0.0           # the masks of the forward this backward belongs to (g["rng"])
        if c.norm_first:
            return self._backward_pre(p, P, G, dfeat, done, drop, ks, ws)
        for l in reversed(range(c.layers)):
            ly = g["layers"][l]
            xin = g["m"] if l == 0 else self.layer_out(g["layers"][l - 1])
            an, nn_, fn, fnn = c.layer_names(l)
            fin = ly["hc"] if c.conv_kernel else ly["h"]        # the FFN sub-layer's input
            if D:
                ga = self._add_ln_bwd(g, gcur, fin, ly["f"], P[fnn + ".weight"], ly["stats2"], G[fnn + ".weight"], G[fnn + ".bias"], R, C,
                                      8 * l + 4 if drop else None)
                done(fnn)
                self._ffn_backward(p, P, G, fn, ga, fin, ly["u"], 8 * l + 3, g["dh1"], drop, ks, ws, done)
                g["dh1"].add_(g["dres"])                 # the residual branch
                gcur = g["dh1"]
            if c.conv_kernel:
                gcur = self._conv_backward(p, P, G, l, ly, gcur, not p.trained, ks, ws, done)
            ga = self._add_ln_bwd(g, gcur, xin, ly["a"], P[nn_ + ".weight"], ly["stats"], G[nn_ + ".weight"], G[nn_ + ".bias"], R, C,
                                  8 * l + 1 if drop else None)
            done(nn_)
            self._attn_backward(p, P, G, l, ly, an, ga, xin, g["dm"], drop, ks, ws, done)
            g["dm"].add_(g["dres"])                      # the residual branch: the gradient of the layer's input
            gcur = g["dm"]
        # back through the mel mean
        eng._k("sed_mel_mean_bwd", lib.sed_mel_mean_bwd, eng.dt, L.ptr(g["dm"]), L.ptr(dfeat), R, p.w_out, C, pad32(C), st)

    def _forward_pre(self, p, P, keep, training, update_running_stats, drop):
        c, eng, lib, st, g = self.cfg, self.eng, self.eng.lib, _stream(), p.sa
        D, C, R = c.ffn, self.eng.cfg[-1][0], p.sa["R"]
        rng = L.ptr(g["rng"]) if drop else None
        for n in g["chain"]:
            # the previous sub-layer's add (where there is one) and this node's LayerNorm
            a, s, site, la = n["add"] if n["add"] is not None else (None, 1.0, 0, 0)
            eng._k("sed_resid_layernorm_fwd", lib.sed_resid_layernorm_fwd, L.ptr(n["src"]), L.ptr(a), s, L.ptr(P[n["norm"] + ".weight"]),
                   L.ptr(P[n["norm"] + ".bias"]), L.ptr(n["x"]) if a is not None else None, L.ptr(n["y"]),
                   L.ptr(n["stats"]) if keep else None, R, C, LN_EPS, drop if a is not None else 0.0, rng, 8 * la + site, st)
            if n["sub"] is None:
                continue
            kind, mod, l, ly = n["sub"]
            if kind == "attn":
                self._attn_forward(p, P, l, ly, mod, n["y"], keep, drop)
            elif kind == "conv":
                self._conv_inner_forward(p, P, l, ly, n["y"], keep, training, update_running_stats)
            elif kind == "ffn":
                self._ffn_fwd(g, P, mod, n["y"], ly["f"], ly["u"], keep, drop, 8 * l + 3, R, C, D)
            else:
                self._ffn_fwd(g, P, mod, n["y"], ly["mf"], ly["mu"], keep, drop, 8 * l + 5, R, C, D)
        if drop:
            self.drop_state[2:3].add_(1)                     # the next training forward draws new masks (captured with the step)
        return g["h"]

    def _backward_pre(self, p, P, G, dfeat, done, drop, ks, ws):
        """The chain in reverse.  gs: the running gradient of the residual stream (None while nothing has arrived on the current
        stream); gy: the gradient of the current node's LayerNorm output.  A node's launch adds its LayerNorm's input gradient to gs
        in place (dxsum aliases dres_in) and leaves the gradient of the sub-layer output that was added in front of it (ga)."""
        c, eng, lib, st, g = self.cfg, self.eng, self.eng.lib, _stream(), p.sa
        C, R = self.eng.cfg[-1][0], p.sa["R"]
        rng = L.ptr(g["rng"]) if drop else None
        gy, gs, flip = g["dh"], None, 0
        for n in reversed(g["chain"]):
            if n["sub"] is not None:
                # the sub-layer behind this node: ga (the gradient of its output) -> its parameters' gradients and gy = g["dn"]
                kind, mod, l, ly = n["sub"]
                if kind == "attn":
                    self._attn_backward(p, P, G, l, ly, mod, ga, n["y"], g["dn"], drop, ks, ws, done)
                elif kind == "conv":
                    self._conv_inner_backward(p, P, G, l, ly, ga, n["y"], g["dn"], not p.trained, ks, ws, done)
                else:
                    u, hid = (ly["u"], 8 * l + 3) if kind == "ffn" else (ly["mu"], 8 * l + 5)
                    self._ffn_backward(p, P, G, mod, ga, n["y"], u, hid, g["dn"], drop, ks, ws, done)
                gy = g["dn"]
            else:
                # a closing norm: its output is a new stream, whose gradient is what has arrived on it (the head's for the last one)
                gy, gs = (gs if gs is not None else gy), None
            if gs is None:
                flip ^= 1
                dx = g["ds"][flip]                      # (never the buffer gy may be)
            else:
                dx = gs
            a, s, site, la = n["add"] if n["add"] is not None else (None, 1.0, 0, 0)
            # the gradient of a is dx itself where s m sd = 1
            da = g["da"] if a is not None and (drop or s != 1.0) else None
            eng._k("sed_resid_layernorm_bwd", lib.sed_resid_layernorm_bwd, L.ptr(gy), L.ptr(gs), L.ptr(n["x"]), L.ptr(P[n["norm"] + ".weight"]),
                   L.ptr(n["stats"]), s, L.ptr(dx), L.ptr(da), L.ptr(G[n["norm"] + ".weight"]), L.ptr(G[n["norm"] + ".bias"]),
                   L.ptr(g["ln_ws"]), R, C, drop if da is not None else 0.0, rng, 8 * la + site, st)
            done(n["norm"])
            gs = dx
            ga = da if da is not None else dx
        # back through the mel mean
        eng._k("sed_mel_mean_bwd", lib.sed_mel_mean_bwd, eng.dt, L.ptr(gs), L.ptr(dfeat), R, p.w_out, C, pad32(C), st)
