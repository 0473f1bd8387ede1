#!/usr/bin/env python3
"""Ragged against padded token extraction on one batch of clips of different lengths, one process.

    python tools/bench_ragged.py [--clips 64] [--min-s 2] [--max-s 10] [--reps 20] [--warmup 3]
                                 [--gemm x6,bf16] [--out profiles/ragged_ab.json]

Padded side: the existing codes-only staged path (mel -> encode -> vq_encode, every want_* false) on
the batch right-padded to its longest clip, (B, T_max).  Ragged side: NativeCodec.tokenize_ragged on the
same clips resident in HBM (the call packs them and uploads its plan table, which is timed with it).
The two sides alternate inside every repetition; each is timed with HIP events; the record holds the
median and the spread, both row counts, launch counts and the per-kernel tables of one profiled call
each.  A second, ungated record repeats this on 32 equal-length 10 s clips (per-row cost with nothing
to skip).  Synthetic clips with seeded lengths, seeded synthetic weights.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distilcodec_nabeel_amd import config, synth, weights  # noqa: E402
from distilcodec_nabeel_amd.engine import NativeCodec  # noqa: E402


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


def run_batch(eng, lengths, seed, reps, warmup):
    clips = [torch.from_numpy(synth.batch_clips(lengths, i, i + 1, seed=seed)[0]).cuda() for i in range(len(lengths))]
    B, n_max = len(clips), max(lengths)
    padded = torch.zeros(B, n_max + 1, device="cuda")
    for i, c in enumerate(clips):
        padded[i, 1: 1 + c.numel()] = c
    t_max = eng.num_frames(n_max + 1)
    rows_ragged = sum(eng.num_frames(n + 1) for n in lengths)

    def pad_step():
        return eng.vq_encode(eng.encode(eng.mel(padded)), want_pjt_in=False, want_fup=False, want_quantized=False)[0]

    def rag_step():
        return eng.tokenize_ragged(clips)

    for _ in range(warmup):
        pad_step()
        rag_step()
    torch.cuda.synchronize()
    t_pad, t_rag = [], []
    for _ in range(reps):
        ms, pc = _timed(pad_step)
        t_pad.append(ms)
        ms, (rc, off, _, _) = _timed(rag_step)
        t_rag.append(ms)
    # how far the padded batch's codes are from each clip's own (ragged) codes, on the clips' own frames
    off = off.tolist()
    same = sum(int((pc[b, : off[b + 1] - off[b]] == rc[off[b]: off[b + 1]]).sum()) for b in range(B))
    k_pad, k_rag = _profiled(eng, pad_step), _profiled(eng, rag_step)
    med = lambda v: float(np.median(v))  # noqa: E731
    return {
        "clips": B, "seconds_min": min(lengths) / 24000, "seconds_max": n_max / 24000,
        "rows_padded": B * t_max, "rows_ragged": rows_ragged, "row_share": round(rows_ragged / (B * t_max), 4),
        "padded_ms": round(med(t_pad), 3), "ragged_ms": round(med(t_rag), 3),
        "padded_ms_min_max": [round(min(t_pad), 3), round(max(t_pad), 3)],
        "ragged_ms_min_max": [round(min(t_rag), 3), round(max(t_rag), 3)],
        "ragged_over_padded": round(med(t_rag) / med(t_pad), 4),
        "us_per_row_padded": round(1e3 * med(t_pad) / (B * t_max), 4),
        "us_per_row_ragged": round(1e3 * med(t_rag) / rows_ragged, 4),
        "launches_padded": sum(v["launches"] for v in k_pad.values()),
        "launches_ragged": sum(v["launches"] for v in k_rag.values()),
        "codes_equal_on_own_frames": round(same / rows_ragged, 5),
        "reps": reps, "warmup": warmup, "kernels_padded": k_pad, "kernels_ragged": k_rag,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=2.0)
    ap.add_argument("--max-s", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gemm", default="x6,bf16")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None, help="write the record to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ragged.py needs the GPU: nothing is measured without one")
    cfg = config.default_config()
    state = weights.synthetic_state_dict(cfg, seed=1234, with_generator=False)
    eng = NativeCodec(cfg, state, "cuda:0", with_generator=False)
    r = np.random.Generator(np.random.PCG64(a.seed))
    lengths = [int(x) for x in r.integers(int(a.min_s * 24000), int(a.max_s * 24000) + 1, size=a.clips)]
    record = {"data": "synthetic speech/music-like clips, seeded lengths uniform in [min, max] s, seeded synthetic weights",
              "timing": "HIP events around each call, sides alternating, median of reps", "modes": {}}
    for mode in a.gemm.split(","):
        eng.set_gemm(mode)
        rec = {"ragged_batch": run_batch(eng, lengths, a.seed, a.reps, a.warmup),
               "equal_length_32x10s": run_batch(eng, [240000] * 32, a.seed + 1000, a.reps, a.warmup)}
        record["modes"][mode] = rec
        for name, v in rec.items():
            print(json.dumps({"gemm": mode, "batch": name, **{k: v[k] for k in v if not k.startswith("kernels_")}}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
