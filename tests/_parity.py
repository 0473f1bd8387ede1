"""Shared parity checks of the GPU path against the reference's outputs (fixtures or the oracle).

Waveform parity is asserted unconditionally.  When every code matches, the end-to-end waveform is
compared with the reference's.  When a non-decisive code differs (allowed: the fp64 top-2 gap is
below 1e-4 relative, where the CPU reference itself flips codes between thread counts), the
REFERENCE's codes are decoded on the GPU (vq_decode + generator, distil_codec.py:581-594) and that
waveform is held to the same SNR, so a code flip can never turn the waveform check into a pass.
"""
from __future__ import annotations

import numpy as np
import torch


def snr_db(x, ref) -> float:
    x = np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, np.float64).reshape(-1)
    ref = np.asarray(ref.detach().cpu() if torch.is_tensor(ref) else ref, np.float64).reshape(-1)
    return float(10 * np.log10((ref ** 2).sum() / max(((x - ref) ** 2).sum(), 1e-300)))


def _f64(x):
    return np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, np.float64)


def rel_per_clip(y, ref) -> np.ndarray:
    """max|y_b - ref_b| / max|ref_b| for every clip b (axis 0): shape (B,).  A batch-wide
    max|err| / max|ref| is carried by the loudest clip: a quiet clip that is entirely wrong beside
    it changes nothing there, and reads 1.0 here."""
    y, ref = _f64(y), _f64(ref)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    B = ref.shape[0]
    err = np.abs(y - ref).reshape(B, -1).max(axis=1)
    return err / (np.abs(ref).reshape(B, -1).max(axis=1) + 1e-300)


def rel_per_row(y, ref, channel_axis: int = 1) -> np.ndarray:
    """The same per (clip, row) of a (B, C, L) tensor (channels_first as the oracle lays it out;
    channel_axis=2 for channels-last), the maxima taken over the channels: shape (B, L)."""
    y, ref = _f64(y), _f64(ref)
    assert y.shape == ref.shape and y.ndim == 3, (y.shape, ref.shape)
    return np.abs(y - ref).max(axis=channel_axis) / (np.abs(ref).max(axis=channel_axis) + 1e-300)


def snr_per_clip(y, ref) -> np.ndarray:
    """SNR in dB of every clip (axis 0) against its own reference: shape (B,)."""
    y, ref = _f64(y), _f64(ref)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    B = ref.shape[0]
    sig = (ref ** 2).reshape(B, -1).sum(axis=1)
    noise = ((y - ref) ** 2).reshape(B, -1).sum(axis=1)
    return 10 * (np.log10(np.maximum(sig, 1e-300)) - np.log10(np.maximum(noise, 1e-300)))


def check_codes(gpu_codes, ref_codes, decisive, min_match: float = 0.97) -> float:
    """Exact on decisive frames, >= min_match exact overall; returns the exact-match rate."""
    gc = np.asarray(gpu_codes.cpu() if torch.is_tensor(gpu_codes) else gpu_codes).astype(np.int64)
    rc = np.asarray(ref_codes.cpu() if torch.is_tensor(ref_codes) else ref_codes).astype(np.int64)
    assert gc.shape == rc.shape, (gc.shape, rc.shape)
    assert np.array_equal(gc[decisive], rc[decisive]), "codes differ on decisive frames"
    match = float((gc == rc).mean()) if gc.size else 1.0
    assert match >= min_match, match
    return match


def check_wave(eng, gpu_codes, ref_codes, gpu_wav, ref_wav, min_db: float) -> float:
    """SNR of the GPU waveform against the reference's, unconditionally (see module docstring).
    Returns the SNR that was asserted."""
    gc = np.asarray(gpu_codes.cpu() if torch.is_tensor(gpu_codes) else gpu_codes).astype(np.int64)
    rc = np.asarray(ref_codes.cpu() if torch.is_tensor(ref_codes) else ref_codes).astype(np.int64)
    ref_wav = np.asarray(ref_wav, np.float64).reshape(gc.shape[0], -1)
    if np.array_equal(gc, rc):
        wav = gpu_wav
    else:
        wav = eng.generate(eng.vq_decode(torch.from_numpy(rc).to(torch.int32)))
    wav = np.asarray(wav.detach().cpu(), np.float64).reshape(ref_wav.shape)
    snr = snr_db(wav, ref_wav)
    assert snr >= min_db, f"waveform SNR {snr:.1f} dB < {min_db} dB (codes identical: {np.array_equal(gc, rc)})"
    return snr
