"""Counterpart of /root/reference/dataset/dataset_utils.py:13-91 (collecting audio paths + labels,
reading audio).  Host-side file handling, plus the host half of the device audio ingest (filter design, AudioIngest).

Audio decoding: the reference uses `soundfile` + `librosa.resample` (neither is in this image);
this module reads PCM/float WAV with scipy.io.wavfile and resamples with a polyphase filter
(scipy.signal.resample_poly).  The resampler is NOT librosa's (kaiser_best / soxr): features of
audio that needs resampling differ from the reference's at the filter-design level (documented
deviation; audio already at the working sample rate is bit-identical after decoding).

read_multichannel_audio(..., device=...) runs the channel rule and the same polyphase filter on the MI355X
(sed_resample_poly, float32): audio at the working rate is float32(host path) bit for bit for integer PCM; audio that
needs resampling differs from the host path by the fp32 rounding of the taps and of the FIR sum only (a few 1e-7 of the
signal's level) -- a second, far smaller deviation on top of the filter-design one."""
from __future__ import annotations

import ctypes as C
import json
import os
from collections import defaultdict
from fractions import Fraction
from math import gcd

import numpy as np

from .. import _lib
from .spectogram.spectogram_configs import REF_NATIVE


def get_film_clap_paths_and_labels(data_root, time_margin=0.1):
    """(:13-41) [(audio_path, start_times, end_times, name)] from paths_and_labels_fixed_Meron.txt."""
    result, num_claps = [], 0
    files_per_film = defaultdict(int)
    path_to_label = json.load(open(os.path.join(data_root, "paths_and_labels_fixed_Meron.txt")))
    print("Collecting Film-clap dataset")
    for sound_path, centers in path_to_label.items():
        film_name = os.path.basename(os.path.dirname(sound_path))
        name = f"{film_name}_{os.path.splitext(os.path.basename(sound_path))[0]}"
        assert os.path.exists(sound_path), sound_path
        result.append((sound_path, [e - time_margin for e in centers], [e + time_margin for e in centers], name))
        num_claps += len(centers)
        files_per_film[film_name] += 1
    for film_name, n in files_per_film.items():
        print(f"\t- {film_name} has {n}")
    print(f"\tFilm clap dataset contains {len(result)} audio files with {num_claps} clap incidents")
    return result


def get_tau_sed_paths_and_labels(audio_dir, labels_data_dir, labels=("doorslam",)):
    """(:44-62) one csv per recording; keep the rows whose sound_event_recording is in `labels`."""
    import pandas as pd
    results = []
    for audio_fname in os.listdir(audio_dir):
        bare_name = os.path.splitext(audio_fname)[0]
        df = pd.read_csv(os.path.join(labels_data_dir, bare_name + ".csv"), sep=",")
        keep = [i for i, v in enumerate(df["sound_event_recording"].values) if v in labels]
        results.append((os.path.join(audio_dir, audio_fname), df["start_time"].values[keep],
                        df["end_time"].values[keep], bare_name))
    return results


def tau_audio_and_meta_dirs(root, fold_name="eval"):
    """Where download_tau_sed_2019.ensure_tau_data leaves the extracted data; no download here."""
    audio_dir = os.path.join(root, "raw", f"foa_{fold_name}")                 # download_tau_sed_2019.py:58-60
    meta_dir = os.path.join(root, "raw", f"metadata_{fold_name}")
    for d in (audio_dir, meta_dir):
        if not os.path.isdir(d):
            raise FileNotFoundError(f"{d} is missing: TAU-SED-2019 has to be placed there by hand "
                                    "(this build never downloads; there is no network on the GPU boxes)")
    return audio_dir, meta_dir


def _decode_pcm(data):
    if data.dtype == np.uint8:
        return (data.astype(np.float64) - 128.0) / 128.0
    if np.issubdtype(data.dtype, np.integer):
        return data.astype(np.float64) / float(2 ** (8 * data.dtype.itemsize - 1))   # soundfile's float64 scaling
    return data.astype(np.float64)


def _decode_wav(path):
    from scipy.io import wavfile
    sample_rate, data = wavfile.read(path)
    return _decode_pcm(data), int(sample_rate)


# ---- resampler design (host, float64) and the device ingest --------------------------------------
# max(up, down) of sed_resample_poly: every pair among 8, 11.025, 16, 22.05, 24, 32, 44.1, 48 and 96 kHz but 11.025 <-> 32 / 96 kHz
MAX_RESAMPLE_RATIO = 640
DEVICE_PCM = (np.dtype(np.int16), np.dtype(np.int32), np.dtype(np.float32))    # what the ingest kernel decodes


def resample_ratio(src_rate, dst_rate):
    """(up, down): dst_rate / src_rate as a reduced fraction."""
    if int(src_rate) != src_rate or int(dst_rate) != dst_rate or src_rate <= 0 or dst_rate <= 0:
        raise ValueError(f"sample rates must be positive integers, got {src_rate} -> {dst_rate}")
    fr = Fraction(int(dst_rate), int(src_rate))
    return fr.numerator, fr.denominator


def _check_ratio(up, down):
    if int(up) != up or int(down) != down or up < 1 or down < 1 or gcd(int(up), int(down)) != 1:
        raise ValueError(f"up / down must be a reduced fraction of positive integers, got {up} / {down}")
    if max(up, down) > MAX_RESAMPLE_RATIO:
        raise ValueError(f"resampling by {up} / {down} is outside the supported range max(up, down) <= {MAX_RESAMPLE_RATIO}")


def resample_filter(up, down):
    """The FIR scipy.signal.resample_poly(x, up, down) designs by default, float64, 2 * half + 1 taps with half = 10 * max(up, down):
    up * firwin(2 * half + 1, 1 / max(up, down), window=('kaiser', 5.0)), restated with numpy alone."""
    _check_ratio(up, down)
    fc = 1.0 / max(up, down)
    half = 10 * max(up, down)
    h = fc * np.sinc(fc * (np.arange(2 * half + 1) - half)) * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * up


def resample_phases(up, down):
    """resample_filter in the order sed_resample_poly reads it: (up, Tp) float32, [p][i] = h[p + i * up], zero past the end of h."""
    h = resample_filter(up, down)
    tp = C.c_int(0)
    _lib.check(_lib.lib().sed_resample_plan(int(up), int(down), C.byref(tp), None), "resample_plan")
    padded = np.zeros(up * tp.value, dtype=np.float64)
    padded[:h.size] = h
    return np.ascontiguousarray(padded.reshape(tp.value, up).T.astype(np.float32))


def resampled_length(n_in, up, down):
    return -((-int(n_in) * int(up)) // int(down))


class AudioIngest:
    """PCM frames -> float32 waveform at the working rate on the MI355X (sed_resample_poly): decode, the channel rule of
    read_multichannel_audio and the polyphase resampler in one launch on the current stream.  Keeps the device filter of every
    (up, down) it has met and owns its output buffer: a result is valid until the next call."""

    def __init__(self, device="cuda", ch_out=1):
        import torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the audio ingest runs on the MI355X only (device='cuda')")
        self.ch_out = int(ch_out)
        self._taps = {}
        self._out = None

    def taps(self, up, down):
        import torch
        key = (int(up), int(down))
        if key not in self._taps:
            self._taps[key] = torch.from_numpy(resample_phases(*key)).to(self.device)
        return self._taps[key]

    def __call__(self, pcm, src_rate, dst_rate):
        """pcm: numpy array or tensor (n, ch) or (B, n, ch) of int16, int32 or float32 -> (ch_out, n_out) or (B, ch_out, n_out)."""
        import torch
        x = torch.from_numpy(np.ascontiguousarray(pcm)) if isinstance(pcm, np.ndarray) else pcm
        if x.dim() not in (2, 3):
            raise ValueError("expected PCM frames (n, channels) or (B, n, channels)")
        code = {torch.int16: _lib.PCM_I16, torch.int32: _lib.PCM_I32, torch.float32: _lib.PCM_F32}.get(x.dtype)
        if code is None:
            raise TypeError(f"PCM must be int16, int32 or float32 (got {x.dtype}): other formats decode on the host")
        up, down = resample_ratio(src_rate, dst_rate)
        _check_ratio(up, down)
        x = x.to(self.device).contiguous()
        batched = x.dim() == 3
        B, n_in, ch_in = x.shape if batched else (1,) + tuple(x.shape)
        if n_in < 1:
            raise ValueError("empty audio")
        n_out = resampled_length(n_in, up, down)
        numel = B * self.ch_out * n_out
        if self._out is None or self._out.numel() < numel:
            self._out = torch.empty(numel, dtype=torch.float32, device=self.device)
        out = self._out[:numel].view((B, self.ch_out, n_out) if batched else (self.ch_out, n_out))
        taps = None if up == down == 1 else self.taps(up, down)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().sed_resample_poly(code, _lib.ptr(x), _lib.ptr(taps), _lib.ptr(out), B, n_in, n_out, ch_in,
                                                    self.ch_out, up, down, torch.cuda.current_stream().cuda_stream),
                       "resample_poly")
        return out


_ingests = {}


def read_multichannel_audio(audio_path, target_fs=None, cfg=REF_NATIVE, device=None):
    """(:65-91) (samples, channels) float64 at target_fs with cfg.audio_channels channels.

    With `device`: the file is decoded on the host, its raw int16 / int32 / float32 PCM goes to the MI355X, and AudioIngest applies
    the same channel rule and resampler there; the result is a float32 DEVICE tensor (channels, samples).  At the file's own rate that
    tensor is float32(host result) bit for bit for integer PCM; audio that needs resampling differs from the host result by the fp32
    rounding of the taps and of the FIR sum (the filter design is the same, so the deviation from librosa recorded above is
    unchanged).  uint8 and float64 files take the host path and are copied."""
    if device is not None:
        import torch
        from scipy.io import wavfile
        if not torch.cuda.is_available():
            raise RuntimeError("no MI355X visible: the device audio ingest has no CPU form (device=None / host_resample give the host path)")
        sample_rate, data = wavfile.read(audio_path)
        if data.dtype in DEVICE_PCM:
            key = (str(torch.device(device)), int(cfg.audio_channels))
            if key not in _ingests:
                _ingests[key] = AudioIngest(device, cfg.audio_channels)
            dst = int(sample_rate) if target_fs is None else int(target_fs)
            return _ingests[key](data.reshape(data.shape[0], -1), int(sample_rate), dst).clone()
        host = read_multichannel_audio(audio_path, target_fs, cfg)
        return torch.from_numpy(np.ascontiguousarray(host.T.astype(np.float32))).to(device)
    audio, sample_rate = _decode_wav(audio_path)
    if audio.ndim == 1:
        audio = audio.reshape(-1, 1)
    if audio.shape[1] < cfg.audio_channels:
        audio = np.repeat(audio.mean(1).reshape(-1, 1), cfg.audio_channels, axis=1)
    elif cfg.audio_channels == 1:
        audio = audio.mean(1).reshape(-1, 1)
    elif audio.shape[1] > cfg.audio_channels:
        audio = audio[:, :cfg.audio_channels]
    if target_fs is not None and sample_rate != target_fs:
        from scipy.signal import resample_poly
        fr = Fraction(int(target_fs), int(sample_rate))
        audio = np.stack([resample_poly(audio[:, i], fr.numerator, fr.denominator) for i in range(audio.shape[1])],
                         axis=1)
    return audio
