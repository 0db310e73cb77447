"""Drop-in counterparts of /root/reference/models/spectogram_models.py (ConvBlock :128-160,
Cnn_AvgPooling :163-230, interpolate :9-22, init_layer/init_bn :25-40) whose arithmetic runs in
libsed_hip.so on an MI355X.  Same constructor signatures, forward() shapes and state_dict keys
(`conv_blocks.{i}.conv{1,2}.weight`, `conv_blocks.{i}.bn{1,2}.{weight,bias,running_mean,
running_var,num_batches_tracked}`, `event_fc.{weight,bias}`; with attention=True also `att_fc.{weight,bias}`), so checkpoints interchange with the
reference's `train.py:123-128` / `main.py:37-39`.

There is no CPU path: calling forward() on a CPU module raises.
"""
from __future__ import annotations

import math
from typing import Dict

import torch
import torch.nn as nn

from .. import _lib as L
from ..engine import CnnEngine, SaConfig, num_pools_of, pad32, _stream

DEFAULT_CHANNEL_AND_POOL = [(64, 2), (128, 2), (256, 2), (512, 1)]   # spectogram_models.py:7
AUDIO_CHANNELS = 1      # dataset/common_config.py:6
MEL_BINS = 64           # dataset/spectogram/spectogram_configs.py:6

# arithmetic precision of newly built models: 'bf16' (bf16 storage + MFMA, fp32 accumulate) or
# 'fp32' (fp32 storage, exact-f32 MFMA: the mode the 1e-3 logit parity gate is judged in)
DEFAULT_PRECISION = "bf16"


def interpolate(x, ratio):
    """(batch, time_steps, classes) -> (batch, time_steps*ratio, classes), each step repeated."""
    if x.is_cuda and x.dtype == torch.float32:
        B, t, K = x.shape
        x = x.contiguous()
        out = torch.empty((B, t * ratio, K), dtype=torch.float32, device=x.device)
        L.check(L.lib().sed_interpolate(L.ptr(x), L.ptr(out), B, t, K, int(ratio), _stream()), "interpolate")
        return out
    return x.repeat_interleave(ratio, dim=1)     # shape utility for host-side tensors


def init_layer(layer, nonlinearity='leaky_relu'):
    nn.init.kaiming_uniform_(layer.weight, nonlinearity=nonlinearity)
    if hasattr(layer, 'bias') and layer.bias is not None:
        layer.bias.data.fill_(0.)


def init_bn(bn):
    bn.bias.data.fill_(0.)
    bn.running_mean.data.fill_(0.)
    bn.weight.data.fill_(1.)
    bn.running_var.data.fill_(1.)


class _Conv3x3Params(nn.Module):
    """Parameter holder with nn.Conv2d(3x3, bias=False)'s weight shape and default init draw."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 3, 3))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))   # same RNG draw as nn.Conv2d.__init__
        self.bias = None


class _BatchNormParams(nn.Module):
    """Parameter/buffer holder with nn.BatchNorm2d's names (eps 1e-5, momentum 0.1)."""

    def __init__(self, num_features):
        super().__init__()
        self.num_features = num_features
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class _LinearParams(nn.Module):
    def __init__(self, in_features, out_features):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))   # same RNG draws as nn.Linear.__init__
        bound = 1 / math.sqrt(in_features)
        nn.init.uniform_(self.bias, -bound, bound)


class _BlockFunction(torch.autograd.Function):
    """One ConvBlock (conv3x3-BN-ReLU twice, avg-pool) as an autograd node over the HIP kernels, NCHW fp32 at the
    boundary like the reference module (spectogram_models.py:153-160), including the input gradient."""

    @staticmethod
    def forward(ctx, block, keep, x, w1, w2, g1, b1, g2, b2):
        eng = block._engine()
        P = block._tensor_dict()
        training = block.training
        plan = eng.forward(x, P, training, keep_for_grad=keep)
        if training:
            block.bn1.num_batches_tracked += 1
            block.bn2.num_batches_tracked += 1
        block._fwd_serial += 1
        ctx.block, ctx.plan, ctx.serial, ctx.training = block, plan, block._fwd_serial, training
        yh = plan.y[0]
        B, Ho, Wo, Cp = yh.shape
        y = torch.empty((B, block.conv2.out_channels, Ho, Wo), dtype=torch.float32, device=x.device)
        L.check(L.lib().sed_nhwc_to_nchw(eng.dt, L.ptr(yh), L.ptr(y), B, block.conv2.out_channels, Ho, Wo, Cp, _stream()),
                "nhwc_to_nchw")
        return y

    @staticmethod
    def backward(ctx, dy):
        block, plan = ctx.block, ctx.plan
        if ctx.serial != block._fwd_serial:
            raise RuntimeError("the activations of this forward were overwritten by a later forward of the same shape")
        eng = block._engine()
        P = block._tensor_dict()
        dy = dy.contiguous().float()
        B, C, Ho, Wo = dy.shape
        L.check(L.lib().sed_nchw_to_nhwc(eng.dt, L.ptr(dy), L.ptr(plan.dy[0]), B, C, Ho, Wo, plan.dy[0].shape[3], _stream()),
                "nchw_to_nhwc")
        names = ["conv1.weight", "conv2.weight", "bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias"]
        G = {"conv_blocks.0." + n: torch.empty_like(P["conv_blocks.0." + n]) for n in names}
        eng.backward(plan, P, G)
        cin = block.conv1.in_channels
        dx = torch.empty((B, cin, plan.T, plan.F), dtype=torch.float32, device=dy.device)
        L.check(L.lib().sed_nhwc_to_nchw(eng.dt, L.ptr(plan.dx), L.ptr(dx), B, cin, plan.T, plan.F, plan.dx.shape[3], _stream()),
                "nhwc_to_nchw")
        return (None, None, dx) + tuple(G["conv_blocks.0." + n] for n in names)


class ConvBlock(nn.Module):
    def __init__(self, in_channels, out_channels, pool_size=2, precision=None):
        super().__init__()
        self.pool_size = pool_size
        self.precision = precision
        self.conv1 = _Conv3x3Params(in_channels, out_channels)
        self.conv2 = _Conv3x3Params(out_channels, out_channels)
        self.bn1 = _BatchNormParams(out_channels)
        self.bn2 = _BatchNormParams(out_channels)
        self.init_weights()
        self._eng = None
        self._fwd_serial = 0

    def init_weights(self):
        init_layer(self.conv1)
        init_layer(self.conv2)
        init_bn(self.bn1)
        init_bn(self.bn2)

    def _engine(self):
        prec = self.precision or DEFAULT_PRECISION
        if self._eng is None or self._eng.precision != prec:
            self._eng = CnnEngine(1, [(self.conv2.out_channels, int(self.pool_size))], self.conv1.in_channels, prec,
                                  head="none", generic_first=True)
        return self._eng

    def _tensor_dict(self) -> Dict[str, torch.Tensor]:
        d = {"conv_blocks.0." + n: p.data for n, p in self.named_parameters()}
        d.update({"conv_blocks.0." + n: b for n, b in self.named_buffers()})
        return d

    def forward(self, input):
        """(B, Cin, H, W) float32 on the GPU -> (B, Cout, H // pool, W // pool): spectogram_models.py:153-160 as ONE
        autograd node (inside Cnn_AvgPooling the blocks run fused, NHWC/bf16 end to end, without this NCHW round trip).
        W must be 8, 16, 32 or 64 (the mel axis of the network's four blocks)."""
        if not input.is_cuda or not self.conv1.weight.is_cuda:
            raise RuntimeError("ConvBlock runs on the MI355X only: move the module and the input to 'cuda' "
                               "(there is no CPU path)")
        x = input.float()
        # an eval forward under grad mode keeps what the eval-mode (running-statistics) backward needs; outputs are the same bits
        keep = torch.is_grad_enabled() and not self.training
        return _BlockFunction.apply(self, keep, x, self.conv1.weight, self.conv2.weight, self.bn1.weight, self.bn1.bias,
                                    self.bn2.weight, self.bn2.bias)


class _ModelFunction(torch.autograd.Function):
    """Whole-model forward/backward as ONE autograd node over the HIP pipeline."""

    @staticmethod
    def forward(ctx, model, keep, x, *params):
        P = model._tensor_dict()
        training = model.training
        plan = model.engine.forward(x, P, training, keep_for_grad=keep)
        if training:
            model._nbt_pending += 1
        model._fwd_serial += 1
        ctx.model, ctx.plan, ctx.serial = model, plan, model._fwd_serial
        ctx.training = training
        return model.engine.interpolate(plan)

    @staticmethod
    def backward(ctx, dlogits):
        model = ctx.model
        if ctx.serial != model._fwd_serial:
            raise RuntimeError("the activations of this forward were overwritten by a later forward of the "
                               "same shape; call backward() before the next forward()")
        P = model._tensor_dict()
        names = [n for n, _ in model._core_named_parameters()]
        G = {n: torch.empty_like(P[n]) for n in names}
        need_dx = bool(ctx.needs_input_grad[2])
        model.engine.backward(ctx.plan, P, G, dlogits=dlogits.contiguous().float(), need_dx=need_dx)
        return (None, None, ctx.plan.dx_in if need_dx else None) + tuple(G[n] for n in names)


class Cnn_AvgPooling(nn.Module):
    def __init__(self, classes_num, model_config=DEFAULT_CHANNEL_AND_POOL, precision=None, mel_bins=None, frontend=None,
                 attention=False):
        '''attention: True registers att_fc, a second linear layer beside event_fc that scores every frame per class (the
        attention pooling head, csrc/sed_attn.hip; pooling "att" of FusedTrainer / clip_probs).  forward() is unchanged: it
        returns the frame logits, and its autograd backward gives att_fc a zero gradient.  False draws no random number and adds
        no key to the state_dict.
        mel_bins: the declared input width (mel-bin count).  None: the specialised widths only (8 / 16 / 32 / 64 at every
        block), as before.  An integer F in [1, 256]: inputs of width F only; blocks at other widths run the width-general
        kernels.  The parameters do not depend on it: a checkpoint loads into a model of any declared width.
        frontend: None, or a models.frontend_layers.PCEN applied to the input before the first block (submodule `frontend`,
        first in parameter order; its width must be the model's, MEL_BINS when mel_bins is None).  None adds no key to the
        state_dict and launches nothing new.'''
        super().__init__()
        self.mel_bins = CnnEngine.check_mel_bins(mel_bins)
        self.attention = bool(attention)
        self.frontend = self._check_frontend(frontend, self.mel_bins)      # before conv_blocks: first in named_parameters()
        self.model_config = model_config
        self.classes_num = classes_num
        self.precision = precision or DEFAULT_PRECISION
        self.num_pools = num_pools_of(model_config)
        blocks = [ConvBlock(in_channels=AUDIO_CHANNELS, out_channels=model_config[0][0], pool_size=model_config[0][1])]
        for i in range(1, len(model_config)):
            blocks.append(ConvBlock(in_channels=model_config[i - 1][0], out_channels=model_config[i][0],
                                    pool_size=model_config[i][1]))
        self.conv_blocks = torch.nn.Sequential(*blocks)
        self._build_head(model_config[-1][0], classes_num)
        self.init_weights()
        if self.attention:          # after event_fc, and after its init: the other parameters draw what they always drew
            self.att_fc = _LinearParams(self.event_fc.in_features, classes_num)
            init_layer(self.att_fc)
        self.engine = self._make_engine(self.precision)
        self._fwd_serial = 0
        self._nbt_pending = 0     # training forwards not yet added to the num_batches_tracked buffers

    @staticmethod
    def _check_frontend(frontend, mel_bins):
        if frontend is None:
            return None
        from .frontend_layers import PCEN
        if not isinstance(frontend, PCEN):
            raise TypeError(f"frontend must be a PCEN layer or None (got {type(frontend).__name__})")
        width = MEL_BINS if mel_bins is None else mel_bins
        if frontend.mel_bins != width:
            raise ValueError(f"the front-end was built for {frontend.mel_bins} mel bins, the model takes {width}")
        return frontend

    def _core_named_parameters(self):
        """The parameters the engine owns: every one but the front-end layer's, which has an autograd node of its own."""
        return [(n, p) for n, p in self.named_parameters() if not n.startswith("frontend.")]

    def _flush_counters(self):
        """BatchNorm's num_batches_tracked buffers are bookkeeping only (momentum is fixed): training
        forwards are counted on the host and folded into the 8 buffers when somebody looks at them,
        instead of launching 8 one-element kernels per step."""
        if self._nbt_pending:
            n, self._nbt_pending = self._nbt_pending, 0
            for blk in self.conv_blocks:
                blk.bn1.num_batches_tracked += n
                blk.bn2.num_batches_tracked += n

    def state_dict(self, *args, **kwargs):
        self._flush_counters()
        return super().state_dict(*args, **kwargs)

    def init_weights(self):
        init_layer(self.event_fc)

    def _build_head(self, c_last, classes_num):
        self.event_fc = _LinearParams(c_last, classes_num)

    def _make_engine(self, precision):
        return CnnEngine(self.classes_num, self.model_config, AUDIO_CHANNELS, precision, mel_bins=self.mel_bins,
                         attention=self.attention)

    def set_precision(self, precision: str):
        self.precision = precision
        self.engine = self._make_engine(precision)
        return self

    def clone_without_engines(self):
        """A deep copy of the parameters, buffers and settings with an engine of its own (the mean teacher of FusedTrainer).  An
        engine holds the library handle and the plans' device buffers, neither of which is to be copied: deepcopy's memo maps
        an object's id to its copy, so entering the engines there as None makes the copy carry None in their place."""
        import copy
        memo = {id(self.engine): None}
        memo.update({id(blk._eng): None for blk in self.conv_blocks if blk._eng is not None})
        if self.frontend is not None:       # its workspace is a device buffer like the plans'
            memo[id(self.frontend._ws)] = None
        twin = copy.deepcopy(self, memo)
        twin.engine = twin._make_engine(twin.precision)
        return twin

    def _tensor_dict(self) -> Dict[str, torch.Tensor]:
        d = {n: p.data for n, p in self.named_parameters()}
        d.update({n: b for n, b in self.named_buffers()})
        return d

    def forward(self, x):
        '''Input: (batch_size, channels_num, times_steps, freq_bins) float32 on the GPU.
        Output: raw logits (batch_size, 8*floor(floor(floor(T/2)/2)/2), classes_num).'''
        if not x.is_cuda:
            raise RuntimeError("Cnn_AvgPooling runs on the MI355X only: move the model and the input to "
                               "'cuda' (there is no CPU path)")
        first = next(self.parameters())
        if not first.is_cuda:
            raise RuntimeError("model parameters are on the CPU; call model.to('cuda')")
        x = x.float()
        if self.frontend is not None:
            # the layer's own autograd node; a trainable one makes x require a gradient, so the keep / need_dx route below runs
            x = self.frontend(x if x.dim() == 4 else x.unsqueeze(1))
        params = [p for _, p in self._core_named_parameters()]
        # grad mode: an eval forward keeps what the eval-mode (frozen-BatchNorm) backward needs, a training forward whose input
        # needs a gradient keeps what the input gradient needs (C1 mode: conv1's ReLU mask).  Outputs are the same bits.
        keep = torch.is_grad_enabled() and (not self.training or x.requires_grad)
        return _ModelFunction.apply(self, keep, x, *params)

    def logits(self, x):
        return torch.sigmoid(self.forward(x))

    def model_description(self, working_sample_rate=48000, hop_size=15840):
        print("Model description")
        b, w = 'b', MEL_BINS if self.mel_bins is None else self.mel_bins
        h = 60 * working_sample_rate // hop_size
        c = AUDIO_CHANNELS
        print(f"\tInput: ({b}, {c}, {h}, {w})")
        for (c, k) in self.model_config:
            h, w = h // k, w // k
            print(f"\tconv_block -> ({b}, {c}, {h}, {w})")
        print(f"\tmean(dim=3) -> ({b}, {c}, {h})")
        print(f"\ttranspose(1,2) -> ({b}, {h}, {c})")
        print(f"\tFC + sigmoid -> ({b}, {h}, {self.classes_num})")
        num_outputs = h
        h *= 2 ** self.num_pools
        frame_duration = hop_size / working_sample_rate
        print(f"\tinterpolate({2 ** self.num_pools})-> ({b}, {h}, {self.classes_num})")
        print(f"\tModel has {num_outputs} outputs before interpolation, each stands for {2 ** self.num_pools} "
              f"frames or {2 ** self.num_pools * frame_duration:.2f}s")
        n = sum(p.numel() for p in self.parameters() if p.requires_grad)
        print(f"\tModel has {n} parameters")


class _GruParams(nn.Module):
    """Parameter holder with nn.GRU(input, hidden, batch_first=True, bidirectional=True)'s names, shapes
    and default init (U(+-1/sqrt(hidden)), same RNG draw order)."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        k = 1.0 / math.sqrt(hidden_size)
        for sfx in ("", "_reverse"):
            for name, shape in (("weight_ih_l0", (3 * hidden_size, input_size)), ("weight_hh_l0", (3 * hidden_size, hidden_size)),
                                ("bias_ih_l0", (3 * hidden_size,)), ("bias_hh_l0", (3 * hidden_size,))):
                prm = nn.Parameter(torch.empty(shape))
                nn.init.uniform_(prm, -k, k)
                setattr(self, name + sfx, prm)


class Crnn_AvgPooling(Cnn_AvgPooling):
    """BASELINE.json configs[3] (not in the reference repository): the Cnn_AvgPooling
    feature extractor, then mean(dim=3) -> transpose -> bidirectional GRU(C_last, 256) ->
    Linear(512, classes) -> interpolate.  state_dict: conv_blocks.*, gru.{weight_ih_l0,...,
    bias_hh_l0_reverse} (loadable into torch.nn.GRU), event_fc.{weight (classes, 2*hidden), bias}."""

    def __init__(self, classes_num, model_config=DEFAULT_CHANNEL_AND_POOL, precision=None, gru_hidden=256, mel_bins=None,
                 frontend=None, attention=False):
        self.gru_hidden = int(gru_hidden)
        super().__init__(classes_num, model_config, precision, mel_bins=mel_bins, frontend=frontend, attention=attention)

    def _build_head(self, c_last, classes_num):
        self.gru = _GruParams(c_last, self.gru_hidden)
        self.event_fc = _LinearParams(2 * self.gru_hidden, classes_num)

    def _make_engine(self, precision):
        return CnnEngine(self.classes_num, self.model_config, AUDIO_CHANNELS, precision, head="gru",
                         gru_hidden=self.gru_hidden, mel_bins=self.mel_bins, attention=self.attention)


class _MhaParams(nn.Module):
    """Parameter holder with torch.nn.MultiheadAttention(C, heads, batch_first=True)'s names, shapes and initialisation:
    in_proj_weight (3C, C) xavier-uniform, in_proj_bias (3C,) zeros, out_proj.weight (C, C) nn.Linear's default, out_proj.bias (C,)
    zeros.  RNG draw order, as that module's constructor: out_proj.weight, out_proj.bias (nn.Linear's draw, then overwritten
    with zeros), in_proj_weight."""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * embed_dim))
        self.out_proj = _LinearParams(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.in_proj_bias, 0.0)
        nn.init.constant_(self.out_proj.bias, 0.0)


class _LayerNormParams(nn.Module):
    """Parameter holder with torch.nn.LayerNorm(C)'s names (eps 1e-5): weight ones, bias zeros, no random draw."""

    def __init__(self, normalized_shape):
        super().__init__()
        self.normalized_shape = (normalized_shape,)
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))


class _FfnParams(nn.Module):
    """Parameter holder of an encoder layer's feed-forward sub-layer with torch.nn.TransformerEncoderLayer's names: linear1 (D, C) and
    linear2 (C, D), torch.nn.Linear's initial values, drawn in that order (weight, bias each)."""

    def __init__(self, channels, width):
        super().__init__()
        self.linear1 = _LinearParams(channels, width)
        self.linear2 = _LinearParams(width, channels)


class _Conv1dParams(nn.Module):
    """Parameter holder with torch.nn.Conv1d(in, out, k, groups=groups)'s names, shapes (weight (out, in / groups, k), bias (out,)) and
    initial values, drawn in that module's order (weight, then bias)."""

    def __init__(self, in_channels, out_channels, kernel_size, groups=1):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size, self.groups = in_channels, out_channels, kernel_size, groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))   # same RNG draws as nn.Conv1d.__init__
        bound = 1 / math.sqrt(in_channels // groups * kernel_size)
        nn.init.uniform_(self.bias, -bound, bound)


class _ConvModuleParams(nn.Module):
    """Parameter holder of an encoder layer's Conformer convolution module: pointwise1 Conv1d(C, 2C, 1), depthwise Conv1d(C, C, k,
    padding=(k-1)/2, groups=C), bn BatchNorm1d(C), pointwise2 Conv1d(C, C, 1), with torch's names and shapes; drawn in the order
    pointwise1, depthwise, pointwise2 (the BatchNorm draws nothing)."""

    def __init__(self, channels, kernel_size):
        super().__init__()
        self.pointwise1 = _Conv1dParams(channels, 2 * channels, 1)
        self.depthwise = _Conv1dParams(channels, channels, kernel_size, groups=channels)
        self.bn = _BatchNormParams(channels)
        self.pointwise2 = _Conv1dParams(channels, channels, 1)


class _RelPosParams(nn.Module):
    """Parameter holder of one layer's relative-position table: weight (heads, num_buckets) fp32, zeros (nothing is drawn)"""

    def __init__(self, heads, num_buckets):
        super().__init__()
        self.heads, self.num_buckets = heads, num_buckets
        self.weight = nn.Parameter(torch.zeros(heads, num_buckets))


class Csa_AvgPooling(Cnn_AvgPooling):
    """The Cnn_AvgPooling feature extractor with a self-attention encoder layer as the temporal head (the conv-Transformer family
    of the DCASE task-4 systems; csrc/sed_mhsa.hip).  With R = B*t rows and C the last block's channels:
        x   = mean over mel of the conv features                           [R][C]
        x'  = x + pe[i]   (pos_encoding; i = frame inside the clip, pe[i][2j] = sin(i / 10000^(2j/C)), pe[i][2j+1] = cos(the same),
                           built in float64, rounded once to fp32; not a parameter, not in the state_dict)
        qkv = x' . attn.in_proj_weight^T + attn.in_proj_bias               [R][3C]
        ctx = multi-head attention: sa_heads heads of dh = C / sa_heads, softmax over the t frames of the same clip, scores
              scaled by 1/sqrt(dh), no mask, no dropout
        a   = ctx . attn.out_proj.weight^T + attn.out_proj.bias
        h   = LayerNorm(x' + a) (attn_norm; eps 1e-5, affine)
        event_fc(h) (and att_fc(h) with attention=True) -> interpolate as before
    By default no feed-forward sub-layer and one layer.  sa_ffn = D > 0 adds the position-wise MLP of an encoder layer behind the
    attention (csrc/sed_ffn.hip), and sa_layers = N stacks N such layers, the positional table added once before layer 0:
        f   = act(h . ffn.linear1.weight^T + ffn.linear1.bias) . ffn.linear2.weight^T + ffn.linear2.bias     (act: relu or erf-form gelu)
        h2  = LayerNorm(h + f) (ffn_norm)                                  -> the next layer's x, or event_fc's input
    which is torch.nn.TransformerEncoderLayer(C, sa_heads, D, dropout=0.0, activation=act, batch_first=True, norm_first=False);
    encoder_layer_state(state_dict, l) maps a layer's keys onto that module's.  Layer 0 registers attn, attn_norm, ffn, ffn_norm,
    layer l >= 1 attn_l{l}, attn_norm_l{l}, ffn_l{l}, ffn_norm_l{l} (the ffn modules only with sa_ffn > 0), event_fc after them.
    The semantics are torch.nn.MultiheadAttention(C, sa_heads, batch_first=True)'s and
    torch.nn.LayerNorm(C)'s, and attn.* / attn_norm.* of the state_dict load into those modules.  The float64 buffer attn_config =
    (sa_heads, pos_encoding) makes the head rebuildable from a state_dict alone (from_state_dict); a second float64 buffer
    encoder_config = (sa_layers, sa_ffn, activation code: 0 relu, 1 gelu) exists only when sa_layers > 1 or sa_ffn > 0, so a
    default model's state_dict has the one-layer head's keys.
    RNG draw order: conv_blocks as always, then per layer attn.out_proj.weight, attn.out_proj.bias (drawn, then zeroed),
    attn.in_proj_weight (torch's constructor order), then with sa_ffn > 0 ffn.linear1.weight, ffn.linear1.bias, ffn.linear2.weight,
    ffn.linear2.bias (torch.nn.Linear's initial values; the LayerNorms draw nothing); after the layers event_fc's draws and its
    init_layer, then att_fc's with attention=True.
    sa_conv_kernel = k > 0 (odd, 3..31) puts the Conformer convolution module between the attention and the feed-forward sub-layer of
    every layer (csrc/sed_convmod.hip), post-LN like the other two, p = (k - 1) / 2:
        g   = h . convm.pointwise1.weight^T + convm.pointwise1.bias                 [R][2C]  (Conv1d(C, 2C, 1))
        v   = g[:, :C] * sigmoid(g[:, C:])                                          (F.glu over the channels)
        z[b,i,c] = convm.depthwise.bias[c] + sum_{j<k} convm.depthwise.weight[c][0][j] * v[b, i + j - p, c]
                                                    (Conv1d(C, C, k, padding=p, groups=C); frames outside the clip are zero)
        y   = convm.bn(z)     BatchNorm1d(C) over the R rows (eps 1e-5, momentum 0.1; batch statistics and the running update in
                              training, the running statistics in eval)
        o   = silu(y) . convm.pointwise2.weight^T + convm.pointwise2.bias           (Conv1d(C, C, 1))
        h_c = LayerNorm(h + o) (conv_norm)                     -> the FFN sub-layer's input, or the layer's output without an FFN
    Layer 0 registers convm and conv_norm, layer l >= 1 convm_l{l} and conv_norm_l{l}, between that layer's attn_norm* and ffn*;
    conv_module_state(state_dict, l) returns a layer's entries under the names above.  A third float64 buffer conv_config = (k,)
    exists only when k > 0.  Per layer the draws are: the attention's, then convm.pointwise1.{weight, bias}, convm.depthwise.{weight,
    bias}, convm.pointwise2.{weight, bias} (torch.nn.Conv1d's initial values; bn and conv_norm draw nothing), then the FFN's.  With
    k = 0 the draws, the state_dict keys and the launches are those of a model without the argument.
    sa_dropout = p in [0, 1) and sa_dropout_seed: torch.nn.TransformerEncoderLayer(dropout=p)'s placement with one probability for
    every site, in training mode only -- the attention probabilities (p~_ij = m_ij s p_ij, no renormalisation), each sub-layer's output
    before its residual add (attention, convolution module, FFN: LayerNorm(x + m s a)) and the FFN hidden activation (m s act(u)),
    s = 1 / (1 - p).  The masks are generated inside the kernels, forward and backward, from the engine's counter-based state
    engine.drop_state = (seed_lo, seed_hi, step, 0) (csrc/philox.h; tests/dropout_formula.py reproduces every cell); every training
    forward advances the step word by one.  The seed is sa_dropout_seed, or torch.initial_seed() when None: no random number is
    drawn, no parameter or buffer is added, and eval-mode forwards and backwards never drop.  p = 0 (the default) changes nothing.
    sa_window = None, an int w (left = right = w) or a pair (left, right) with None for an unbounded side: the local attention window
    of every head of every layer -- key j of the same clip takes part for query i iff i - left <= j <= i + right, which is
    torch.nn.TransformerEncoderLayer(src, src_mask=M) with M[i][j] = True where j < i - left or j > i + right; (left, 0) is causal
    attention with a look-back of left.  The softmax runs over the in-window keys only (the diagonal is always inside: no empty row)
    and the kernels skip the key tiles outside it (sed_mhsa_fwd_win / sed_mhsa_bwd_win, csrc/sed_mhsa.hip).  The window is
    architecture, not regularisation: it holds in training and eval forwards and in every backward, and dropout composes with it
    (the same cells dropped, p over the window).  Only the attention is windowed: the convolution module and the CNN keep their
    receptive fields.  A float64 buffer window_config = (left, right), -1 for an unbounded side, exists only when a window is set
    (window_config_from_state_dict returns None without it); with sa_window = None the draws, the state_dict keys, the launches and
    the output bits are those of a model without the argument.
    sa_rel_pos = None, an int L >= 1 or a pair (num_buckets, max_distance): a learned relative-position bias per layer, head and bucket,
    as T5 / WavLM / BEATs use it -- with d = j - i (key minus query, frames of the same clip)
        s_ij = scale q_i . k_j + rel_pos.weight[g][bucket(d)]
    which is torch's float attn_mask / src_mask (rel_pos_bias(state_dict, l, t) returns it, (H, t, t)); lse, p and ctx run over the
    in-window keys, dropout and the window compose as before.  L: bucket(d) = clamp(d, -L, L) + L, 2L + 1 buckets.  (nb, maxd): T5's
    bidirectional log buckets, nb even >= 4, maxd > nb / 4; n = nb / 2, a = |d|, m = n / 2: bucket = (n if d > 0 else 0) + (a if a < m
    else min(n - 1, m + floor(ln(a / m) / ln(maxd / m) (n - m)))), in float64 (heads.SaConfig.rel_pos_map).  Every layer has its own table:
    one module with a single fp32 parameter weight (sa_heads, num_buckets), initialised to zeros (no random number is drawn, every other
    parameter keeps its initial value), registered BETWEEN that layer's attn* and attn_norm* -- layer 0 rel_pos, layer l >= 1
    rel_pos_l{l} -- so the parameter order per layer is attn, rel_pos, attn_norm, convm, conv_norm, ffn, ffn_norm and the backward
    completes the groups in exactly the reverse order (the table's gradient is ready right after the attention core's backward, before
    in_proj's).  The kernels read a per-distance table built from the weights by one small launch per layer and forward
    (sed_relpos_expand, sed_mhsa_fwd_rel / _bwd_rel, sed_relpos_fold; csrc/sed_mhsa.hip); the t x t bias and its gradient never
    exist.  A float64 buffer rel_pos_config = (mode, a, b) -- (0, L, 0) or (1, nb, maxd) -- exists only when the option is set
    (rel_pos_config_from_state_dict returns None without it); encoder_layer_state still returns TransformerEncoderLayer's keys only.
    pos_encoding is an independent switch (the expected use is pos_encoding=False with sa_rel_pos).  With sa_rel_pos = None the
    draws, the state_dict keys, the launches and the output bits are those of a model without the argument.
    sa_norm_first = True makes every layer pre-LN: on the residual stream x [R][C] (the positional table added once before layer 0),
    layer l is
        [sa_macaron]      x <- x + 1/2 FFNm(LN(x))      ffn_mac_norm*, ffn_mac*
                          x <- x + MHSA(LN(x))          attn_norm*, attn*, [rel_pos*]
        [sa_conv_kernel]  x <- x + ConvModule(LN(x))    conv_norm*, convm*      (the module's inner arithmetic as above)
        [sa_ffn]          x <- x + s FFN(LN(x))         ffn_norm*, ffn*;  s = 1/2 with sa_macaron, else 1
        [closing norm]    x <- LN(x)                    out_norm*
    The closing norm exists on every layer with sa_macaron (the Conformer block of Gulati et al. 2020: two half-weighted FFNs around
    attention and convolution) and on the last layer only without it, which is torch.nn.TransformerEncoder(TransformerEncoderLayer(C,
    sa_heads, D, norm_first=True), N, norm=LayerNorm(C)); event_fc / att_fc read the last closing norm's output.  One launch forms a
    sub-layer's residual add and the next LayerNorm (sed_resid_layernorm_fwd / _bwd, csrc/sed_layernorm.hip); the attention core, the
    convolution module's inner arithmetic and the FFN kernel are the post-LN ones.  Names: layer 0 bare, layer l >= 1 with _l{l}.
    Registration order per layer: ffn_mac_norm, ffn_mac, attn_norm, attn, rel_pos, conv_norm, convm, ffn_norm, ffn, out_norm -- each
    norm before its sub-layer, because its gradient completes after the sub-layer's; the backward completes the groups in exactly the
    reverse order.  Draw order per layer: the macaron FFN (linear1.weight, linear1.bias, linear2.weight, linear2.bias), the attention,
    the convolution module, the FFN; the LayerNorms draw nothing.  Dropout sites (stream 8 l + site): 0 - 4 as above, 5 the macaron
    FFN's hidden activation, 6 the macaron FFN's output before its add.  A float64 buffer block_config = (norm_first, macaron) exists
    only with sa_norm_first (block_config_from_state_dict); encoder_layer_state keeps returning TransformerEncoderLayer's keys
    (norm1 = attn_norm, norm2 = ffn_norm), closing_norm_state(state_dict, l) returns the closing norm's entries and
    macaron_ffn_state(state_dict, l) the macaron FFN's.  With both False the draws, the state_dict keys, the launches and the output
    bits are those of a model without the arguments.  Refused before any draw: sa_macaron without sa_norm_first, sa_macaron with
    sa_ffn = 0.
    Refused: sa_rel_pos a non-integer or L < 1, num_buckets odd or < 4, max_distance <= num_buckets / 4, more than 4096 buckets,
    a negative or non-integer sa_window side, sa_dropout outside [0, 1), C % sa_heads != 0, a head width other than 32 or 64, C % 4 != 0, sa_layers < 1, sa_ffn not 0 or a multiple of 32 up to
    4096 (and C > 512 with it), an activation other than relu / gelu, sa_conv_kernel even, below 3 or above 31 (before any draw)."""

    ACTIVATIONS = ("relu", "gelu")

    def __init__(self, classes_num, model_config=DEFAULT_CHANNEL_AND_POOL, precision=None, sa_heads=4, pos_encoding=True,
                 mel_bins=None, frontend=None, attention=False, sa_layers=1, sa_ffn=0, sa_activation="relu", sa_conv_kernel=0,
                 sa_dropout=0.0, sa_dropout_seed=None, sa_window=None, sa_rel_pos=None, sa_norm_first=False, sa_macaron=False):
        self.sa_config = SaConfig(int(model_config[-1][0]), sa_heads, pos_encoding, sa_layers, sa_ffn, sa_activation, sa_conv_kernel,
                                  sa_dropout, sa_dropout_seed, sa_window, sa_rel_pos, sa_norm_first, sa_macaron)   # (checked before any draw)
        for kw, v in self.sa_config.keywords(every=True).items():
            setattr(self, kw, v)            # model.sa_heads, model.sa_dropout, ...: the checked options
        super().__init__(classes_num, model_config, precision, mel_bins=mel_bins, frontend=frontend, attention=attention)

    def _build_head(self, c_last, classes_num):
        if self.sa_norm_first:
            self._build_pre_ln_layers(c_last)
        for l in range(0 if self.sa_norm_first else self.sa_layers):
            an, nn_, fn, fnn = CnnEngine.sa_layer_names(l)
            setattr(self, an, _MhaParams(c_last, self.sa_heads))
            if self.sa_rel_pos is not None:
                setattr(self, CnnEngine.sa_rel_name(l), _RelPosParams(self.sa_heads, CnnEngine.rel_pos_buckets(self.sa_rel_pos)))
            setattr(self, nn_, _LayerNormParams(c_last))
            if l == 0:
                self.register_buffer("attn_config", torch.tensor([float(self.sa_heads), float(self.pos_encoding)], dtype=torch.float64))
            if self.sa_conv_kernel:
                cm, cn = CnnEngine.sa_conv_names(l)
                setattr(self, cm, _ConvModuleParams(c_last, self.sa_conv_kernel))
                setattr(self, cn, _LayerNormParams(c_last))
            if self.sa_ffn:
                setattr(self, fn, _FfnParams(c_last, self.sa_ffn))
                setattr(self, fnn, _LayerNormParams(c_last))
        if self.sa_conv_kernel:
            self.register_buffer("conv_config", torch.tensor([float(self.sa_conv_kernel)], dtype=torch.float64))
        if self.sa_layers > 1 or self.sa_ffn:
            self.register_buffer("encoder_config", torch.tensor([float(self.sa_layers), float(self.sa_ffn),
                                                                 float(self.ACTIVATIONS.index(self.sa_activation))], dtype=torch.float64))
        if self.sa_window is not None:
            self.register_buffer("window_config", torch.tensor([-1.0 if v is None else float(v) for v in self.sa_window], dtype=torch.float64))
        if self.sa_rel_pos is not None:
            mode = self.sa_rel_pos[0] == "log"
            self.register_buffer("rel_pos_config", torch.tensor([float(mode), float(self.sa_rel_pos[1]),
                                                                 float(self.sa_rel_pos[2]) if mode else 0.0], dtype=torch.float64))
        if self.sa_norm_first:
            self.register_buffer("block_config", torch.tensor([float(self.sa_norm_first), float(self.sa_macaron)], dtype=torch.float64))
        self.event_fc = _LinearParams(c_last, classes_num)

    def _build_pre_ln_layers(self, c_last):
        """sa_norm_first: per layer, every norm BEFORE its sub-layer (SaConfig.module_order); the draws in sub-layer order"""
        cfg = self.sa_config
        for l in range(self.sa_layers):
            for kind, mod, norm, _, _ in cfg.sublayers(l):
                setattr(self, norm, _LayerNormParams(c_last))
                if kind == "attn":
                    setattr(self, mod, _MhaParams(c_last, self.sa_heads))
                    if self.sa_rel_pos is not None:
                        setattr(self, CnnEngine.sa_rel_name(l), _RelPosParams(self.sa_heads, CnnEngine.rel_pos_buckets(self.sa_rel_pos)))
                    if l == 0:
                        self.register_buffer("attn_config", torch.tensor([float(self.sa_heads), float(self.pos_encoding)], dtype=torch.float64))
                elif kind == "conv":
                    setattr(self, mod, _ConvModuleParams(c_last, self.sa_conv_kernel))
                else:
                    setattr(self, mod, _FfnParams(c_last, self.sa_ffn))
            if cfg.has_out_norm(l):
                setattr(self, cfg.out_name(l), _LayerNormParams(c_last))

    @staticmethod
    def block_config_from_state_dict(weights):
        """(sa_norm_first, sa_macaron) from a state_dict's block_config; (False, False) when the buffer is absent"""
        if "block_config" not in weights:
            return False, False
        cfg = weights["block_config"].detach().cpu().double().tolist()
        return bool(round(cfg[0])), bool(round(cfg[1]))

    @staticmethod
    def closing_norm_state(weights, layer):
        """Layer `layer`'s closing LayerNorm entries (weight, bias) of a sa_norm_first state_dict without the module prefix: the last
        layer's load into torch.nn.TransformerEncoder(..., norm=LayerNorm(C)).norm; {} where the layer has no closing norm"""
        on = SaConfig.out_name(layer)
        return {k[len(on) + 1:]: v for k, v in weights.items() if k.startswith(on + ".")}

    @staticmethod
    def macaron_ffn_state(weights, layer):
        """Layer `layer`'s macaron FFN entries of a sa_macaron state_dict: linear1.*, linear2.* and, as norm.*, its LayerNorm's"""
        mn, mnn = SaConfig.macaron_names(layer)
        out = {}
        for k, v in weights.items():
            if k.startswith(mn + "."):
                out[k[len(mn) + 1:]] = v
            elif k.startswith(mnn + "."):
                out["norm." + k[len(mnn) + 1:]] = v
        return out

    def _make_engine(self, precision):
        return CnnEngine(self.classes_num, self.model_config, AUDIO_CHANNELS, precision, head="sa", mel_bins=self.mel_bins,
                         attention=self.attention, **self.sa_config.keywords())

    def _flush_counters(self):
        """The convolution modules' BatchNorm counters follow the conv blocks': counted on the host, folded in when looked at."""
        n = self._nbt_pending
        super()._flush_counters()
        if n and self.sa_conv_kernel:
            for l in range(self.sa_layers):
                getattr(self, CnnEngine.sa_conv_names(l)[0]).bn.num_batches_tracked += n

    @staticmethod
    def conv_config_from_state_dict(weights):
        """sa_conv_kernel from a state_dict's conv_config; 0 when the buffer is absent"""
        if "conv_config" not in weights:
            return 0
        return int(round(weights["conv_config"].detach().cpu().double().tolist()[0]))

    @staticmethod
    def window_config_from_state_dict(weights):
        """sa_window = (left, right), None for an unbounded side, from a state_dict's window_config; None when the buffer is absent"""
        if "window_config" not in weights:
            return None
        cfg = weights["window_config"].detach().cpu().double().tolist()
        return tuple(None if v < 0 else int(round(v)) for v in cfg[:2])

    @staticmethod
    def rel_pos_config_from_state_dict(weights):
        """sa_rel_pos = L or (num_buckets, max_distance) from a state_dict's rel_pos_config; None when the buffer is absent"""
        if "rel_pos_config" not in weights:
            return None
        mode, a, b = (int(round(v)) for v in weights["rel_pos_config"].detach().cpu().double().tolist()[:3])
        return (a, b) if mode else a

    @staticmethod
    def rel_pos_bias(weights, layer, t):
        """(H, t, t) float tensor: layer `layer`'s bias bias[g][i][j] = weight[g][bucket(j - i)] as torch's additive attn_mask / src_mask
        (repeat it over the clips for a 3-D mask), in the weight's dtype on the CPU"""
        cfg = CnnEngine.check_sa_rel_pos(Csa_AvgPooling.rel_pos_config_from_state_dict(weights))
        if cfg is None:
            raise ValueError("the state_dict has no rel_pos_config: the model was built without sa_rel_pos")
        w = weights[CnnEngine.sa_rel_name(layer) + ".weight"].detach().cpu()
        m = torch.from_numpy(CnnEngine.rel_pos_map(cfg, t).astype("int64"))
        i = torch.arange(t)
        return w[:, m[(i[None, :] - i[:, None]) + t - 1]]

    @staticmethod
    def conv_module_state(weights, layer):
        """Layer `layer`'s convolution-module entries of a state_dict without the module prefix: pointwise1.*, depthwise.*, bn.*,
        pointwise2.* (they load into torch.nn.Conv1d / BatchNorm1d modules of those names) and, as conv_norm.*, the LayerNorm's."""
        cm, cn = CnnEngine.sa_conv_names(layer)
        out = {}
        for k, v in weights.items():
            if k.startswith(cm + "."):
                out[k[len(cm) + 1:]] = v
            elif k.startswith(cn + "."):
                out["conv_norm." + k[len(cn) + 1:]] = v
        return out

    @staticmethod
    def encoder_config_from_state_dict(weights):
        """(sa_layers, sa_ffn, sa_activation) from a state_dict's encoder_config; (1, 0, 'relu') when the buffer is absent"""
        if "encoder_config" not in weights:
            return 1, 0, "relu"
        cfg = weights["encoder_config"].detach().cpu().double().tolist()
        return int(round(cfg[0])), int(round(cfg[1])), Csa_AvgPooling.ACTIVATIONS[int(round(cfg[2]))]

    @staticmethod
    def encoder_layer_state(weights, layer):
        """Layer `layer`'s entries of a state_dict under torch.nn.TransformerEncoderLayer's names (self_attn.*, linear1.*, linear2.*,
        norm1.*, norm2.*; the last three only for a model with an FFN): that torch module on the CPU loads them with load_state_dict (what the tests compare against)."""
        an, nn_, fn, fnn = CnnEngine.sa_layer_names(layer)
        out = {}
        for ours, theirs in ((an, "self_attn"), (nn_, "norm1"), (fn, None), (fnn, "norm2")):
            for k, v in weights.items():
                if k.startswith(ours + "."):
                    rest = k[len(ours) + 1:]
                    out[rest if theirs is None else theirs + "." + rest] = v
        return out

    @staticmethod
    def config_from_state_dict(weights):
        """(sa_heads, pos_encoding) from a state_dict's attn_config"""
        cfg = weights["attn_config"].detach().cpu().double().tolist()
        return int(round(cfg[0])), bool(round(cfg[1]))
