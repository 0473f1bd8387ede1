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


# ---------------------------------------------------------------------------------------------
# The ragged batches of tests/test_gpu_ragged_scale.py and tests/test_ragged_plan.py: one pool of
# 19 short clips and a 10 s filler, repeated and shuffled so that every dwconv_ln form of
# launch_dwconv_ln_ragged is selected once.
# ---------------------------------------------------------------------------------------------
# Frame counts below the 7-row window and the ring's prefetch distance, then just below, at and just
# above the 4-, 8-, 16- and 32-row widths: 376 frames, 33 16-row tiles.
RAGGED_SHORT_T = [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 15, 16, 17, 31, 32, 33, 47, 64, 65]
RAGGED_LONG_N, RAGGED_LONG_T = 240000, 937
# case -> (copies of the short set, copies of the long clip, total frames, form); form 0: 16-row tiles
# (>= 512 of them below 8192 rows), else the register ring's run width (8192 * {1, 2, 4, 8} rows)
RAGGED_CASES = {
    "t16": (20, 0, 7520, 0),
    "rw4": (22, 0, 8272, 4),
    "rw8": (22, 9, 16705, 8),
    "rw16": (22, 27, 33571, 16),
    "rw32": (22, 62, 66366, 32),
}


def ragged_pool_lengths() -> list[int]:
    """Raw sample counts of the pool, the long clip last.  A clip of n samples has 1 + (n + 1 - 256) // 256
    frames (n + 1 >= 385), so T frames come from 256 T - 1 .. 256 T + 254 samples: even short clips
    take the low end (384 at T = 1, the shortest the reflect pad accepts), odd ones the high end."""
    n = [max(384, 256 * t - 1) if i % 2 == 0 else 256 * t + 254 for i, t in enumerate(RAGGED_SHORT_T)]
    return n + [RAGGED_LONG_N]


def ragged_case_order(case: str) -> np.ndarray:
    """Pool indices of a case's clips in batch order: the pool repeated, then shuffled with a fixed
    seed, so long and short clips alternate and a workgroup's four runs fall in different clips."""
    k_short, k_long, _, _ = RAGGED_CASES[case]
    ns = len(RAGGED_SHORT_T)
    idx = np.concatenate([np.tile(np.arange(ns), k_short), np.full(k_long, ns, dtype=np.int64)])
    return np.random.default_rng(7000 + k_long).permutation(idx)
