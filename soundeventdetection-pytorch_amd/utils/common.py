"""Counterpart of /root/reference/utils/common.py:11-30 (WeightedBCE); the arithmetic runs in
libsed_hip.so (sed_bce_fwd_bwd); WeakBCE (this build only) is its clip-level counterpart over sed_weak_bce_fwd_bwd."""
from __future__ import annotations

import torch

from .. import _lib as L
from ..engine import _stream, check_pooling


class _BCEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, target, recall_factor):
        B, To, K = output.shape
        dev = output.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dout = torch.empty_like(output)
        scratch = torch.empty(max(1, (B * To * K + 255) // 256), dtype=torch.float32, device=dev)
        L.check(L.lib().sed_bce_fwd_bwd(L.ptr(output), L.ptr(target), L.ptr(loss), L.ptr(dout), L.ptr(scratch), B, To,
                                        K, 1, target.shape[1], float(recall_factor), 1.0, _stream()), "bce_fwd_bwd")
        ctx.save_for_backward(dout)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dout,) = ctx.saved_tensors
        return dout * g, None, None


class WeightedBCE:
    def __init__(self, recall_factor, multi_frame):
        self.recall_factor = float(recall_factor)
        self.multi_frame = multi_frame

    def __call__(self, output, target):
        dev = output.device
        if not output.is_cuda:   # reference eval() hands CPU tensors (train.py:24-26): compute on the GPU anyway
            output = output.cuda()
        target = target.to(output.device)
        if self.multi_frame:
            # (batch, frames, classes); frame counts differ by the pooling floor: the kernel truncates
            # both to N = min(frames) (common.py:20-22)
            o = output.float().contiguous()
            t = target.float().contiguous()
            if o.dim() != 3 or t.dim() != 3 or o.shape[0] != t.shape[0] or o.shape[2] != t.shape[2]:
                raise ValueError(f"expected (B, T, K) output/target, got {tuple(o.shape)} / {tuple(t.shape)}")
        else:
            o = output.float().reshape(1, -1, 1).contiguous()
            t = target.float().reshape(1, -1, 1).contiguous()
            if o.shape != t.shape:
                raise ValueError("output and target sizes differ")
        loss = _BCEFunction.apply(o, t, self.recall_factor)
        return loss if dev == loss.device else loss.to(dev)


class _WeakBCEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, target, recall_factor, mode_id, ratio):
        B, To, K = output.shape
        dev = output.device
        # the model repeats each of its t = To / ratio logits `ratio` times: the kernel takes them once, with `ratio` frames each
        pre = output[:, ::ratio].contiguous()
        t = pre.shape[1]
        frames = target.shape[1] if target.dim() == 3 else 0
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dpre = torch.empty_like(pre)
        ws = torch.empty(max(1, L.lib().sed_weak_bce_ws_bytes(B, t, K) // 8), dtype=torch.float64, device=dev)
        L.check(L.lib().sed_weak_bce_fwd_bwd(L.ptr(pre), L.ptr(target), frames, None, L.ptr(loss), L.ptr(dpre), 0, B, t, K, ratio,
                                             frames if frames else To, mode_id, float(recall_factor), 1.0, 1.0, L.ptr(ws),
                                             _stream()), "weak_bce_fwd_bwd")
        ctx.save_for_backward(dpre)
        ctx.ratio, ctx.frames = ratio, To
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dpre,) = ctx.saved_tensors
        if ctx.ratio == 1:
            return dpre * g, None, None, None, None
        # the gradient of a repeated logit lands on its first copy: the model's backward sums the copies again
        dout = torch.zeros((dpre.shape[0], ctx.frames, dpre.shape[2]), dtype=dpre.dtype, device=dpre.device)
        dout[:, ::ctx.ratio] = dpre * g
        return dout, None, None, None, None


class WeakBCE:
    """Clip-level WeightedBCE (this build only): the (B, T, K) frame logits are turned into probabilities, pooled over time
    (pooling: max, mean, linear or exp) into one clip probability per class and compared with the clip label.  target: (B, K)
    clip labels, or a strong (B, Tt, K) tensor whose maximum over the frames is the clip label; both are truncated to
    min(T, Tt) frames as in WeightedBCE.  ratio: the model's interpolation ratio (Cnn_AvgPooling: 2 ** num_pools) when `output`
    is its x`ratio` repeated logits -- T must be a multiple of it -- so that every distinct logit is read once; the loss is the
    same with ratio=1."""

    def __init__(self, recall_factor, pooling, ratio=1):
        self.recall_factor = float(recall_factor)
        if pooling == "att":
            raise ValueError("unknown pooling 'att' for WeakBCE: the criterion sees only the frame logits, not the attention head's "
                             "(train with FusedTrainer(weak_pooling='att') on a model built with attention=True)")
        self.mode_id = check_pooling(pooling)
        self.pooling = pooling
        self.ratio = int(ratio)
        if self.ratio < 1:
            raise ValueError(f"ratio must be >= 1 (got {ratio!r})")

    def __call__(self, output, target):
        if output.dim() != 3 or target.dim() not in (2, 3):
            raise ValueError(f"expected (B, T, K) output and a (B, K) or (B, Tt, K) target, got {tuple(output.shape)} / "
                             f"{tuple(target.shape)}")
        if output.shape[0] != target.shape[0] or output.shape[2] != target.shape[-1]:
            raise ValueError(f"output {tuple(output.shape)} and target {tuple(target.shape)} differ in batch or classes")
        if output.shape[1] % self.ratio != 0:
            raise ValueError(f"output has {output.shape[1]} frames, not a multiple of ratio={self.ratio}")
        dev = output.device
        if not output.is_cuda:
            output = output.cuda()
        o = output.float()
        t = target.to(output.device).float().contiguous()
        loss = _WeakBCEFunction.apply(o, t, self.recall_factor, self.mode_id, self.ratio)
        return loss if dev == loss.device else loss.to(dev)
