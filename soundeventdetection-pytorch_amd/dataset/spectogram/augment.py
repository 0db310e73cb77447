"""Log-mel batch augmentation on the device (this build only; the reference augments in 'Complex' mode alone).

SpecAugment time / frequency masks, a circular time shift, mixup and FilterAugment-style band gains, applied by ONE launch
(`sed_logmel_augment`, csrc/sed_augment.hip) that also does the crop gather and the z-score, for features and labels.  Every random
decision is drawn here, on the host, from the global numpy RNG -- like `SpectogramDataset._draw` -- so `np.random.seed` reproduces a
run and `train.reseed_rank` separates the data-parallel ranks; the kernel only reads the resulting tables.

`draw()` call order, per batch (a call is skipped where its option is off, so the all-zero config draws nothing):
  1. for each sample b in order: `time_masks` x [w = randint(0, time_mask_frames + 1), clipped to T; t0 = randint(0, T - w + 1)],
     then `freq_masks` x [w = randint(0, freq_mask_bins + 1), clipped to F; f0 = randint(0, F - w + 1)],
     then shift = randint(0, T) with `time_shift`;
  2. with mixup_prob > 0: perm = permutation(B); for each b: rand() < mixup_prob -> l = beta(alpha, alpha), lam = max(l, 1 - l),
     partner = perm[b] (a sample that draws itself stays unmixed);
  3. with filter_prob > 0, for each b: rand() < filter_prob -> n = randint(lo, hi + 1) bands; n - 1 distinct interior knots
     (choice without replacement, sorted) between the end bins; n + 1 knot gains uniform(db_lo, db_hi); np.interp over the bins."""
from __future__ import annotations

import dataclasses
from typing import Optional, Tuple

import numpy as np
import torch

from ... import _lib as L

MAX_MASKS = 8            # SED_AUG_MAX_MASKS of csrc/sed_augment.hip


@dataclasses.dataclass
class SpecAugmentConfig:
    """Everything at zero (the defaults) is valid and is the identity.  mask_value 0.0 is the bank mean after the z-score."""
    time_masks: int = 0
    time_mask_frames: int = 0          # a mask is 0 .. time_mask_frames frames wide
    freq_masks: int = 0
    freq_mask_bins: int = 0
    time_shift: bool = False
    mixup_prob: float = 0.0
    mixup_alpha: float = 0.2
    label_mix: str = "max"             # "max": the rule of the complex-mode mix; "soft": lam * y + (1 - lam) * y_partner
    filter_prob: float = 0.0
    filter_bands: Tuple[int, int] = (3, 6)
    filter_db: Tuple[float, float] = (-6.0, 6.0)
    mask_value: float = 0.0

    def __post_init__(self):
        for name in ("time_masks", "time_mask_frames", "freq_masks", "freq_mask_bins"):
            v = getattr(self, name)
            if int(v) != v or v < 0:
                raise ValueError(f"{name} must be an integer >= 0 ({v!r} given)")
            setattr(self, name, int(v))
        if self.time_masks > MAX_MASKS or self.freq_masks > MAX_MASKS:
            raise ValueError(f"at most {MAX_MASKS} time masks and {MAX_MASKS} frequency masks per sample")
        for name in ("mixup_prob", "filter_prob"):
            v = float(getattr(self, name))
            if not 0.0 <= v <= 1.0:
                raise ValueError(f"{name} must lie in [0, 1] ({v!r} given)")
            setattr(self, name, v)
        if not float(self.mixup_alpha) > 0.0:
            raise ValueError(f"mixup_alpha must be > 0 ({self.mixup_alpha!r} given)")
        if self.label_mix not in ("max", "soft"):
            raise ValueError(f"label_mix is 'max' or 'soft' ({self.label_mix!r} given)")
        lo, hi = (int(v) for v in self.filter_bands)
        if not 1 <= lo <= hi:
            raise ValueError(f"filter_bands must be (lo, hi) with 1 <= lo <= hi ({self.filter_bands!r} given)")
        self.filter_bands = (lo, hi)
        dlo, dhi = (float(v) for v in self.filter_db)
        if not (np.isfinite(dlo) and np.isfinite(dhi) and dlo <= dhi):
            raise ValueError(f"filter_db must be a finite (lo, hi) with lo <= hi ({self.filter_db!r} given)")
        self.filter_db = (dlo, dhi)
        if not np.isfinite(self.mask_value):
            raise ValueError("mask_value must be finite")

    @property
    def label_mix_code(self) -> int:
        return 1 if self.label_mix == "soft" else 0


def row_ints(cfg: SpecAugmentConfig) -> int:
    return 4 + 2 * (cfg.time_masks + cfg.freq_masks)


def _band_gain(cfg: SpecAugmentConfig, F: int) -> np.ndarray:
    """One FilterAugment-style gain curve over F bins, float64 (dB)."""
    n = int(np.random.randint(cfg.filter_bands[0], cfg.filter_bands[1] + 1))
    n = max(1, min(n, F - 1))                       # n - 1 distinct interior knots need F - 2 >= n - 1
    if F == 1:
        return np.array([np.random.uniform(*cfg.filter_db)], dtype=np.float64)
    inner = np.sort(np.random.choice(np.arange(1, F - 1), n - 1, replace=False)) if n > 1 else np.zeros(0, dtype=np.int64)
    knots = np.concatenate(([0], inner, [F - 1])).astype(np.float64)
    gains = np.random.uniform(cfg.filter_db[0], cfg.filter_db[1], n + 1)
    return np.interp(np.arange(F, dtype=np.float64), knots, gains)


def draw(cfg: SpecAugmentConfig, starts, T: int, F: int, std_mel=None):
    """The tables of one batch: (tab int32 (B, row_ints), gain float32 (B, F) or None).  starts: the crop start of every sample
    in the feature bank; T, F: crop frames and mel bins.  std_mel (F,): the z-score's std where the features are z-scored --
    adding g dB before the z-score is adding g / std after it.  Call order: the module docstring."""
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    B, T, F = len(starts), int(T), int(F)
    nt, nf = cfg.time_masks, cfg.freq_masks
    tab = np.zeros((B, row_ints(cfg)), dtype=np.int32)
    tab[:, 0] = starts
    tab[:, 2] = np.arange(B)
    lam = np.ones(B, dtype=np.float32)
    for b in range(B):
        for count, width, axis, base in ((nt, cfg.time_mask_frames, T, 4), (nf, cfg.freq_mask_bins, F, 4 + 2 * nt)):
            for m in range(count):
                w = min(int(np.random.randint(0, width + 1)), axis)
                tab[b, base + 2 * m] = int(np.random.randint(0, axis - w + 1))
                tab[b, base + 2 * m + 1] = w
        if cfg.time_shift:
            tab[b, 1] = int(np.random.randint(0, T))
    if cfg.mixup_prob > 0.0:
        perm = np.random.permutation(B)
        for b in range(B):
            if np.random.rand() < cfg.mixup_prob:
                l = float(np.random.beta(cfg.mixup_alpha, cfg.mixup_alpha))
                if int(perm[b]) != b:
                    tab[b, 2] = int(perm[b])
                    lam[b] = np.float32(max(l, 1.0 - l))          # the sample keeps its identity
    tab[:, 3] = lam.view(np.int32)
    gain = None
    if cfg.filter_prob > 0.0:
        g64 = np.zeros((B, F), dtype=np.float64)
        for b in range(B):
            if np.random.rand() < cfg.filter_prob:
                g64[b] = _band_gain(cfg, F)
        if std_mel is not None:
            g64 = g64 / np.broadcast_to(np.asarray(std_mel, dtype=np.float64), (F,))[None, :]
        gain = g64.astype(np.float32)
    return tab, gain


def launch(bank, bank_frames, events, K, mean, std, tab_h, gain_h, cfg: SpecAugmentConfig, B, T, F, stream):
    """Upload the tables, allocate the outputs and run sed_logmel_augment.  bank (bank_frames, F) fp32 and events
    (bank_frames, K) float64 (or None) are device tensors; `stream` is the current stream (the table uploads are ordered on
    it).  Returns (out (B, T, F) fp32, ev_out (B, T, K) float64 or None)."""
    dev = bank.device
    tab_h = np.ascontiguousarray(tab_h, dtype=np.int32)
    tab_d = torch.from_numpy(tab_h).to(dev)
    gain_d = None if gain_h is None else torch.from_numpy(np.ascontiguousarray(gain_h, dtype=np.float32)).to(dev)
    out = torch.empty((B, T, F), dtype=torch.float32, device=dev)
    ev_out = None if events is None else torch.empty((B, T, K), dtype=torch.float64, device=dev)
    L.check(L.lib().sed_logmel_augment(L.ptr(bank), int(bank_frames), L.ptr(events), int(K), L.ptr(mean), L.ptr(std),
                                       tab_h.ctypes.data, L.ptr(tab_d), L.ptr(gain_d), float(cfg.mask_value),
                                       cfg.label_mix_code, L.ptr(out), L.ptr(ev_out), B, T, F, cfg.time_masks, cfg.freq_masks,
                                       stream), "logmel_augment")
    return out, ev_out


class LogMelAugment:
    """Callable (x (B, 1, T, F) fp32 cuda, y (B, T, K) any float dtype) -> (x', y'): new tensors, the inputs are untouched, y'
    comes out in y's dtype.  One launch per call; `last_tab` / `last_gain` are the host tables of the last call."""

    def __init__(self, cfg: Optional[SpecAugmentConfig] = None):
        self.cfg = cfg if cfg is not None else SpecAugmentConfig()
        self.last_tab: Optional[np.ndarray] = None
        self.last_gain: Optional[np.ndarray] = None

    def __call__(self, x: torch.Tensor, y: torch.Tensor):
        if not (x.is_cuda and y.is_cuda):
            raise RuntimeError("LogMelAugment runs on the MI355X (cuda tensors); there is no CPU path")
        if x.dim() != 4 or x.shape[1] != 1 or x.dtype != torch.float32:
            raise ValueError(f"features must be (B, 1, T, F) float32, got {tuple(x.shape)} {x.dtype}")
        B, _, T, F = x.shape
        if y.dim() != 3 or y.shape[0] != B or y.shape[1] != T or not y.is_floating_point():
            raise ValueError(f"labels must be a float (B, T, K) = ({B}, {T}, K) tensor, got {tuple(y.shape)} {y.dtype}")
        K = int(y.shape[2])
        xb = x.contiguous().view(B * T, F)
        yb = y.contiguous().to(torch.float64).view(B * T, K)
        tab, gain = draw(self.cfg, np.arange(B, dtype=np.int64) * T, T, F)
        self.last_tab, self.last_gain = tab, gain
        out, ev = launch(xb, B * T, yb, K, None, None, tab, gain, self.cfg, B, T, F,
                         torch.cuda.current_stream().cuda_stream)
        return out.view(B, 1, T, F), ev.to(y.dtype)
