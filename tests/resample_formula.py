"""Float64 restatement of the audio ingest (decode, channel rule, polyphase resampler) shared by tests/test_resample_host.py and
tests/test_gpu_resample.py.  torch, on whichever device the operands live; nothing of the library is called here.

    y[m] = sum_k h[m*down + half - k*up] * x[k],   m = 0 .. ceil(n_in*up/down) - 1,   half = 10*max(up, down)

with terms whose index falls outside h (2*half + 1 taps) or outside x absent."""
import numpy as np
import torch

SCALE = {np.dtype(np.int16): 2.0 ** -15, np.dtype(np.int32): 2.0 ** -31, np.dtype(np.float32): 1.0}


def n_out_of(n_in, up, down):
    return -((-n_in * up) // down)


def term_indices(up, down, n_in, device="cpu"):
    """(j, k, valid), each (n_out, T): output m's i-th candidate term is h[j[m, i]] * x[k[m, i]], present where valid"""
    half = 10 * max(up, down)
    T = 2 * half // up + 1
    m = torch.arange(n_out_of(n_in, up, down), dtype=torch.int64, device=device)
    t = m * down + half
    q = torch.div(t, up, rounding_mode="floor")
    p = t - q * up
    i = torch.arange(T, dtype=torch.int64, device=device)
    j = p[:, None] + i[None, :] * up
    k = q[:, None] - i[None, :]
    valid = (j <= 2 * half) & (k >= 0) & (k < n_in)
    return j.clamp(max=2 * half), k.clamp(0, n_in - 1), valid


def resample_formula(x, h, up, down, idx=None):
    """x float64 (..., n_in), h float64 (2*half + 1,) -> (y, S, taps): the sum, the sum of the terms' magnitudes (both (..., n_out))
    and the number of terms present per output (n_out,)"""
    j, k, valid = term_indices(up, down, x.shape[-1], x.device) if idx is None else idx
    hm = h[j] * valid
    xg = x[..., k]
    return (hm * xg).sum(-1), (hm.abs() * xg.abs()).sum(-1), valid.sum(-1)


def downmix(pcm, ch_out):
    """pcm numpy (..., n, ch_in) int16 / int32 / float32 -> float64 (..., ch_out, n): soundfile's scaling, then the channel rule of
    read_multichannel_audio (fewer channels than wanted: the mean, duplicated; one wanted: the mean; more: the first ch_out)"""
    a = pcm.astype(np.float64) * SCALE[pcm.dtype]
    ch_in = a.shape[-1]
    if ch_in < ch_out:
        a = np.repeat(a.mean(-1, keepdims=True), ch_out, axis=-1)
    elif ch_out == 1:
        a = a.mean(-1, keepdims=True)
    elif ch_in > ch_out:
        a = a[..., :ch_out]
    return np.ascontiguousarray(np.swapaxes(a, -1, -2))
