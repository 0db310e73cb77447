"""Trainable front-end layers that sit between the log-mel features and Cnn_AvgPooling / Crnn_AvgPooling.

PCEN: per-channel energy normalisation (Wang et al., ICASSP 2017; for sound event detection Lostanlen et al. 2019), the usual
replacement for the logarithm in far-field and noisy detection.  Forward and backward run in libsed_hip.so (csrc/sed_pcen.hip;
include/sed_hip.h has the formulas).  There is no CPU path.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from .. import _lib as L

PCEN_INPUTS = {"db": 0, "power": 1}
PARAM_NAMES = ("log_alpha", "log_delta", "log_r", "logit_s")
MAX_MEL_BINS = 256


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class _PCENFunction(torch.autograd.Function):
    """The layer as ONE autograd node over sed_pcen_fwd / sed_pcen_bwd.  The backward rebuilds the smoother from x: nothing but
    x and the four parameter rows is saved."""

    @staticmethod
    def forward(ctx, layer, x, log_alpha, log_delta, log_r, logit_s):
        theta = torch.stack([log_alpha.detach(), log_delta.detach(), log_r.detach(), logit_s.detach()]).contiguous()
        y = layer.run_forward(x, theta)
        ctx.layer, ctx.theta = layer, theta
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        need_dx = bool(ctx.needs_input_grad[1])
        need_dtheta = any(ctx.needs_input_grad[2:6])
        if not (need_dx or need_dtheta):
            return (None,) * 6
        dx, dtheta = ctx.layer.run_backward(x, ctx.theta, gy, need_dx, need_dtheta)
        rows = tuple(dtheta[i] if ctx.needs_input_grad[2 + i] else None for i in range(4)) if need_dtheta else (None,) * 4
        return (None, dx) + rows


class PCEN(nn.Module):
    """y = (E / (eps + M)^alpha + delta)^r - delta^r per mel bin, M the first-order smoother of E along time with coefficient s
    (M_0 = E_0), E = gain * 10^((x * std + mean) / 10) for input='db' (log-mel in dB, z-scored by mean / std when given: what
    every dataset path of this package yields) or gain * max(x, 0) for input='power'.  alpha, delta, r and s are per-bin and
    trained through log_alpha, log_delta, log_r (their logarithms) and logit_s; trainable=False keeps the four as buffers of the
    same names.  (B, 1, T, F) or (B, T, F) float32 on the GPU gives the same shape."""

    def __init__(self, mel_bins: int, input: str = "db", mean=None, std=None, alpha: float = 0.98, delta: float = 2.0,
                 r: float = 0.5, s: float = 0.025, eps: float = 1e-6, gain: float = 1.0, trainable: bool = True):
        super().__init__()
        if isinstance(mel_bins, bool) or int(mel_bins) != mel_bins or not (1 <= int(mel_bins) <= MAX_MEL_BINS):
            raise ValueError(f"mel_bins must be an integer in [1, {MAX_MEL_BINS}] (got {mel_bins!r})")
        if input not in PCEN_INPUTS:
            raise ValueError(f"input must be 'db' (log-mel in dB) or 'power' (linear mel power), got {input!r}")
        if (mean is None) != (std is None):
            raise ValueError("mean and std come together")
        if mean is not None and input != "db":
            raise ValueError("mean / std un-normalise a z-scored dB input: they do not go with input='power'")
        for name, v in (("alpha", alpha), ("delta", delta), ("r", r), ("eps", eps), ("gain", gain)):
            if not (0.0 < float(v) < float("inf")):
                raise ValueError(f"{name} must be finite and > 0 (got {v!r})")
        if not (0.0 < float(s) < 1.0):
            raise ValueError(f"s must lie in (0, 1) (got {s!r})")
        F = self.mel_bins = int(mel_bins)
        self.trainable = bool(trainable)
        init = {"log_alpha": math.log(alpha), "log_delta": math.log(delta), "log_r": math.log(r),
                "logit_s": math.log(s) - math.log1p(-s)}
        for name in PARAM_NAMES:
            t = torch.full((F,), init[name], dtype=torch.float32)
            if self.trainable:
                setattr(self, name, nn.Parameter(t))
            else:
                self.register_buffer(name, t)
        if mean is None:
            self.register_buffer("feat_mean", None)
            self.register_buffer("feat_std", None)
        else:
            m = torch.as_tensor(mean, dtype=torch.float32).reshape(-1)
            sd = torch.as_tensor(std, dtype=torch.float32).reshape(-1)
            if m.numel() != F or sd.numel() != F:
                raise ValueError(f"mean and std must have mel_bins = {F} entries (got {m.numel()} and {sd.numel()})")
            self.register_buffer("feat_mean", m.clone())
            self.register_buffer("feat_std", sd.clone())
        # (input kind, eps, gain): with it a state_dict alone rebuilds the layer (from_state_dict)
        self.register_buffer("pcen_config", torch.tensor([float(PCEN_INPUTS[input]), float(eps), float(gain)], dtype=torch.float64))
        self._config = (PCEN_INPUTS[input], float(eps), float(gain))
        self._ws = None
        self.backward_calls = 0         # sed_pcen_bwd calls so far (tests: a fixed layer with a constant input makes none)

    # -- persistence ---------------------------------------------------------------------------
    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        c = self.pcen_config.detach().cpu()
        self._config = (int(c[0].item()), float(c[1].item()), float(c[2].item()))

    @classmethod
    def from_state_dict(cls, sd, prefix: str = "", trainable: bool = True) -> "PCEN":
        """The layer a state_dict describes: its width, input kind, eps, gain, mean / std and the four parameter rows."""
        cfg = sd[prefix + "pcen_config"].detach().cpu()
        kind = int(cfg[0].item())
        if kind not in (0, 1):
            raise ValueError(f"{prefix}pcen_config names input kind {kind}")
        mean, std = sd.get(prefix + "feat_mean"), sd.get(prefix + "feat_std")
        layer = cls(sd[prefix + "log_alpha"].numel(), input="db" if kind == 0 else "power", mean=mean, std=std,
                    eps=float(cfg[1].item()), gain=float(cfg[2].item()), trainable=trainable)
        own = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)} if prefix else dict(sd)
        layer.load_state_dict({k: own[k] for k in layer.state_dict().keys()})
        return layer

    def extra_repr(self) -> str:
        kind, eps, gain = self._config
        return (f"mel_bins={self.mel_bins}, input={'db' if kind == 0 else 'power'}, eps={eps:g}, gain={gain:g}, "
                f"trainable={self.trainable}, normalised={self.feat_mean is not None}")

    # -- the two calls -------------------------------------------------------------------------
    def theta(self) -> torch.Tensor:
        """(4, F) fp32: the four parameter rows as the kernels take them."""
        return torch.stack([getattr(self, n).detach() for n in PARAM_NAMES]).contiguous()

    def _check_input(self, x: torch.Tensor):
        if not x.is_cuda or not self.log_alpha.is_cuda:
            raise RuntimeError("PCEN runs on the MI355X only: move the module and the input to 'cuda' (there is no CPU path)")
        if x.dtype != torch.float32:
            raise ValueError("PCEN takes float32")
        if x.dim() == 4 and x.shape[1] == 1:
            B, _, T, F = x.shape
        elif x.dim() == 3:
            B, T, F = x.shape
        else:
            raise ValueError(f"PCEN takes (B, 1, T, F) or (B, T, F), got {tuple(x.shape)}")
        if F != self.mel_bins:
            raise ValueError(f"PCEN was built for {self.mel_bins} mel bins, the input has {F}")
        return int(B), int(T), int(F)

    def _workspace(self, B: int, T: int, F: int, device) -> torch.Tensor:
        n = (L.lib().sed_pcen_ws_bytes(B, T, F) + 7) // 8
        if self._ws is None or self._ws.numel() < n or self._ws.device != device:
            self._ws = torch.empty(n, dtype=torch.float64, device=device)
        return self._ws

    def run_forward(self, x: torch.Tensor, theta: Optional[torch.Tensor] = None, launch=None) -> torch.Tensor:
        """sed_pcen_fwd on x.  launch: None, or an engine's _k (so that the call shows in its launch list / timer)."""
        B, T, F = self._check_input(x)
        x = x.detach().contiguous()
        theta = self.theta() if theta is None else theta
        y = torch.empty_like(x)
        kind, eps, gain = self._config
        lib = L.lib()
        args = (L.ptr(x), L.ptr(self.feat_mean), L.ptr(self.feat_std), L.ptr(theta), kind, eps, gain, L.ptr(y),
                L.ptr(self._workspace(B, T, F, x.device)), B, T, F, _stream())
        if launch is not None:
            launch("sed_pcen_fwd", lib.sed_pcen_fwd, *args)
        else:
            L.check(lib.sed_pcen_fwd(*args), "sed_pcen_fwd")
        return y

    def run_backward(self, x: torch.Tensor, theta: Optional[torch.Tensor], gy: torch.Tensor, need_dx: bool = True,
                     need_dtheta: bool = True, dtheta_out: Optional[torch.Tensor] = None, launch=None):
        """sed_pcen_bwd: (dx or None, dtheta (4, F) or None).  dtheta_out: a contiguous (4, F) fp32 tensor to write into."""
        B, T, F = self._check_input(x)
        x = x.detach().contiguous()
        gy = gy.detach().float().contiguous()
        if gy.shape != x.shape:
            raise ValueError(f"the upstream gradient has shape {tuple(gy.shape)}, the input {tuple(x.shape)}")
        theta = self.theta() if theta is None else theta
        dx = torch.empty_like(x) if need_dx else None
        dtheta = None
        if need_dtheta:
            dtheta = dtheta_out if dtheta_out is not None else torch.empty((4, F), dtype=torch.float32, device=x.device)
        kind, eps, gain = self._config
        lib = L.lib()
        args = (L.ptr(x), L.ptr(self.feat_mean), L.ptr(self.feat_std), L.ptr(theta), kind, eps, gain, L.ptr(gy), L.ptr(dx),
                L.ptr(dtheta), L.ptr(self._workspace(B, T, F, x.device)), B, T, F, _stream())
        self.backward_calls += 1
        if launch is not None:
            launch("sed_pcen_bwd", lib.sed_pcen_bwd, *args)
        else:
            L.check(lib.sed_pcen_bwd(*args), "sed_pcen_bwd")
        return dx, dtheta

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._check_input(x)
        return _PCENFunction.apply(self, x, *(getattr(self, n) for n in PARAM_NAMES))
