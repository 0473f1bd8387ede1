#!/usr/bin/env python3
"""Ragged against padded decode (codes -> waveform) on batches of code lists of different lengths, one process.

    python tools/bench_ragged_decode.py [--reps 10] [--warmup 2] [--out profiles/ragged_decode_ab.json]

Padded side: vq_decode + generate on the lists padded to the longest, (B, T_max), what
decode_from_codes_batch runs.  Ragged side: NativeCodec.decode_ragged on the same padded codes with
the per-clip lengths resident in HBM.  Three batches (24 kHz, 93.75 frames per second):
  * c4_like: 32 clips of 9-10 s (C4's distribution, about 5 % padding);
  * tts_like: one 10 s clip beside 31 of 1-3 s (mostly padding);
  * uniform_32x10s: every length equal to T_max (nothing to skip: what the lengths cost).
The two sides alternate inside every repetition; each is timed with HIP events; the record holds the
median and the spread, the same pair for the generator alone (generate / generate_ragged on one z),
real samples per second, and the share of the padded frames' time recovered:
(padded - ragged) / (padded * padding share), where the padded call's time is taken as proportional to
its frames.  Empty workgroups and the tail rounds of partly filled launches keep that share below 1.
Seeded random codes, seeded synthetic weights.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distilcodec_nabeel_amd import config, weights  # noqa: E402
from distilcodec_nabeel_amd.engine import NativeCodec  # noqa: E402

FPS = 24000 / 256


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def _profiled(eng, fn):
    eng.profile(True)
    eng.profile_reset()
    fn()
    kern = eng.profile_read()
    eng.profile(False)
    eng.profile_reset()
    return kern


def run_batch(eng, lens, seed, reps, warmup):
    B, t_max = len(lens), max(lens)
    rng = np.random.default_rng(seed)
    codes = torch.from_numpy(rng.integers(0, eng.NC, size=(B, t_max)).astype(np.int32)).cuda()
    for b, n in enumerate(lens):
        codes[b, n:] = 0  # the padded call's pad code (decode_from_codes_batch)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device="cuda")
    wav = torch.empty(B, eng.hop * t_max, device="cuda")

    def pad_step():
        return eng.generate(eng.vq_decode(codes))

    def rag_step():
        return eng.decode_ragged(codes, lens_dev, wav=wav)

    for _ in range(warmup):
        pad_step()
        rag_step()
    torch.cuda.synchronize()
    z = eng.vq_decode(codes).clone()
    t_pad, t_rag, t_gen, t_genr = [], [], [], []
    for _ in range(reps):
        t_pad.append(_timed(pad_step)[0])
        t_rag.append(_timed(rag_step)[0])
        t_gen.append(_timed(lambda: eng.generate(z))[0])  # the generator alone, on the same z
        t_genr.append(_timed(lambda: eng.generate_ragged(z, lens_dev, wav=wav))[0])
    k_pad, k_rag = _profiled(eng, pad_step), _profiled(eng, rag_step)
    med = lambda v: float(np.median(v))  # noqa: E731
    frames, padded = sum(lens), B * t_max
    pad_share = 1.0 - frames / padded
    saved = med(t_pad) - med(t_rag)
    return {
        "clips": B, "frames_max": t_max, "frames_real": frames, "frames_padded": padded, "padding_share": round(pad_share, 4),
        "padded_ms": round(med(t_pad), 3), "ragged_ms": round(med(t_rag), 3),
        "padded_ms_min_max": [round(min(t_pad), 3), round(max(t_pad), 3)],
        "ragged_ms_min_max": [round(min(t_rag), 3), round(max(t_rag), 3)],
        "ragged_over_padded": round(med(t_rag) / med(t_pad), 4),
        "generate_ms": round(med(t_gen), 3), "generate_ragged_ms": round(med(t_genr), 3),
        "generate_ragged_over_generate": round(med(t_genr) / med(t_gen), 4),
        "real_samples_per_s_padded": round(frames * eng.hop / (med(t_pad) * 1e-3)),
        "real_samples_per_s_ragged": round(frames * eng.hop / (med(t_rag) * 1e-3)),
        "padding_time_recovered": round(saved / (med(t_pad) * pad_share), 4) if pad_share > 0 else None,
        "reps": reps, "warmup": warmup, "kernels_padded": k_pad, "kernels_ragged": k_rag,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None, help="write the record to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ragged_decode.py needs the GPU: nothing is measured without one")
    cfg = config.default_config()
    eng = NativeCodec(cfg, weights.synthetic_state_dict(cfg, seed=1234), "cuda:0", gemm="x6")
    r = np.random.Generator(np.random.PCG64(a.seed))
    sec = lambda lo, hi, n: [int(round(s * FPS)) for s in r.uniform(lo, hi, size=n)]  # noqa: E731
    batches = {
        "c4_like": sec(9.0, 10.0, 32),
        "tts_like": [int(round(10 * FPS))] + sec(1.0, 3.0, 31),
        "uniform_32x10s": [int(round(10 * FPS))] * 32,
    }
    record = {"data": "seeded random codes, seeded synthetic weights; lengths in frames of 256 samples at 24 kHz",
              "timing": "HIP events around each call, sides alternating, median of reps", "batches": {}}
    for name, lens in batches.items():
        rec = run_batch(eng, lens, a.seed, a.reps, a.warmup)
        record["batches"][name] = rec
        print(json.dumps({"batch": name, **{k: v for k, v in rec.items() if not k.startswith("kernels_")}}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
