"""Host-side helpers of the ragged decode (NativeCodec.generate_ragged / decode_ragged,
DistilCodec.decode_from_codes_batch(ragged=True)): padding and validation of code lists and
per-clip lengths.  numpy only, so they run (and are tested) without a GPU or the native library."""
from __future__ import annotations

import numpy as np

PAD_CODE = -1  # the reference's masked code; the ragged kernels never read a padded entry


def check_lengths(lengths, batch: int, frames_max: int) -> np.ndarray:
    """Per-clip frame counts as a contiguous int32 array [batch].  ValueError for an empty batch, a
    count that does not match `batch`, a non-integer value, or a length outside [0, frames_max]
    (the kernels would clamp it silently)."""
    a = np.asarray(lengths)
    if a.ndim != 1 or a.shape[0] == 0:
        raise ValueError("lengths must be a non-empty 1-D sequence")
    if a.shape[0] != batch:
        raise ValueError(f"{a.shape[0]} lengths for a batch of {batch} clips")
    if a.dtype.kind not in "iu":
        if a.dtype.kind != "f" or not np.all(a == np.floor(a)):
            raise ValueError("lengths must be integers")
    if frames_max < 1:
        raise ValueError("frames_max must be >= 1")
    a64 = a.astype(np.int64)
    bad = np.nonzero((a64 < 0) | (a64 > frames_max))[0]
    if bad.size:
        b = int(bad[0])
        raise ValueError(f"clip {b} has length {int(a64[b])}, outside [0, {frames_max}]")
    return np.ascontiguousarray(a64.astype(np.int32))


def pad_code_lists(codes_list, pad: int = PAD_CODE, n_residual: int = 1) -> tuple[np.ndarray, np.ndarray]:
    """Code lists of different lengths -> (codes int32 [B, T_max] filled with `pad` beyond each
    list, lengths int32 [B]).  T_max is at least 1, so a batch of empty lists is still a valid
    (all-zero output) call.  ValueError for an empty batch or a code that does not fit int32.
    `n_residual` = R > 1: the lists are flat and frame-major, R codes per frame (as `encode` yields
    them); codes is [B, T_max, R], lengths count frames, and a list whose length is not a multiple
    of R is a ValueError."""
    if len(codes_list) == 0:
        raise ValueError("ragged decode needs at least one clip")
    R = int(n_residual)
    if R < 1:
        raise ValueError("n_residual must be >= 1")
    rows = [np.asarray(c, dtype=np.int64).reshape(-1) for c in codes_list]
    for b, r in enumerate(rows):
        if r.shape[0] % R:
            raise ValueError(f"clip {b}: a code list of {r.shape[0]} entries is not a multiple of the {R} codebooks per frame")
    lengths = np.array([r.shape[0] // R for r in rows], dtype=np.int32)
    t_max = max(1, int(lengths.max()))
    out = np.full((len(rows), t_max * R), pad, dtype=np.int64)
    for b, r in enumerate(rows):
        out[b, : r.shape[0]] = r
    if R > 1:
        out = out.reshape(len(rows), t_max, R)
    if out.min() < np.iinfo(np.int32).min or out.max() > np.iinfo(np.int32).max:
        raise ValueError("audio code does not fit 32 bits")
    return np.ascontiguousarray(out.astype(np.int32)), check_lengths(lengths, len(rows), t_max)


def check_codes_in_lengths(codes: np.ndarray, lengths: np.ndarray, codebook_size: int) -> None:
    """IndexError, like torch indexing, for a code outside [-codebook_size, codebook_size) among a
    clip's own entries; what lies beyond a clip's length is not looked at.  codes: [B, T] or, for R
    codebooks per frame, [B, T, R] (every layer's entry is checked)."""
    t = np.arange(codes.shape[1])[None, :]
    live = t < np.asarray(lengths)[:, None]
    if codes.ndim == 3:
        live = live[:, :, None]
    bad = live & ((codes >= codebook_size) | (codes < -codebook_size))
    if bad.any():
        at = tuple(int(v[0]) for v in np.nonzero(bad))
        where = f"clip {at[0]}, frame {at[1]}" + (f", layer {at[2]}" if codes.ndim == 3 else "")
        raise IndexError(f"audio code {int(codes[at])} ({where}) out of range for a codebook of "
                         f"{codebook_size} entries")
