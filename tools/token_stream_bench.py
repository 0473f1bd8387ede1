#!/usr/bin/env python
"""Step latency of the batched token stream (streaming.TokenStream) on the published geometry with
synthetic weights: sessions in {1, 8, 32} x push_frames in {8, 24, 93}, every slot pushing push_frames
frames per step.  Three ways to run the same step alternate inside one process:

  graph   the step replayed from its one captured HIP graph (TokenStream(graph=True));
  eager   the same step launched eagerly;
  loop    what the package offered before: per session, one eager generate(vq_decode(window [1][W])),
          the call HaloStream._generate_window makes, the windows assembled with torch ops.

Every timed step starts from an idle device (a synchronise), is bracketed by HIP events and includes
its host-side work (upload, launches, the copy of the emitted samples).  p50 / p99 over `--steps` steps
after `--warmup` untimed ones, and the audio seconds produced per wall second at p50.  Writes
profiles/token_stream.json and prints the table of DESIGN.md §5 "Token streams".
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SESSIONS = (1, 8, 32)
PUSHES = (8, 24, 93)


class LoopBaseline:
    """Per session: the codes still needed as a device tensor, the window cut with torch ops, one eager
    vq_decode + generate per session and step (HaloStream's generator half, without its encoder)."""

    def __init__(self, eng, sessions: int, halo: int):
        self.eng, self.halo = eng, halo
        self.codes = [torch.empty(0, dtype=torch.int32, device=eng.device) for _ in range(sessions)]
        self.c_off = [0] * sessions
        self.emitted = [0] * sessions

    def push(self, codes_per_slot):
        eng, h, outs = self.eng, self.halo, []
        for b, c in enumerate(codes_per_slot):
            self.codes[b] = torch.cat([self.codes[b], torch.as_tensor(c, dtype=torch.int32).to(eng.device)])
            T = self.c_off[b] + self.codes[b].shape[0]
            E = self.emitted[b]
            f_new = max(E, T - h)
            g0 = max(0, E - h)
            if f_new > E:
                wav = eng.generate(eng.vq_decode(self.codes[b][g0 - self.c_off[b]:][None]))[0]
                outs.append(wav[eng.hop * (E - g0):eng.hop * (f_new - g0)].clone())
            else:
                outs.append(torch.empty(0, device=eng.device))
            self.emitted[b] = f_new
            drop = max(0, f_new - h) - self.c_off[b]
            self.codes[b], self.c_off[b] = self.codes[b][drop:], self.c_off[b] + drop
        return outs


def _timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def run_case(eng, sessions: int, push: int, steps: int, warmup: int, seed: int = 0) -> dict:
    from distilcodec_nabeel_amd.streaming import TokenStream

    ways = {"graph": TokenStream(eng, sessions, push, graph=True), "eager": TokenStream(eng, sessions, push)}
    halo = ways["graph"].halo_frames
    ways["loop"] = LoopBaseline(eng, sessions, halo)
    rng = np.random.default_rng(seed)
    ms = {k: [] for k in ways}
    frames = 0
    for i in range(warmup + steps):
        codes = [rng.integers(0, eng.NC, size=push).astype(np.int32) for _ in range(sessions)]
        outs = {}
        for k, w in ways.items():  # alternating: the three ways see the same step back to back
            t, outs[k] = _timed(lambda w=w: w.push(codes))
            if i >= warmup:
                ms[k].append(t)
        n = [o.numel() for o in outs["graph"]]
        assert n == [o.numel() for o in outs["eager"]] == [o.numel() for o in outs["loop"]]
        assert all(torch.equal(a, b) for a, b in zip(outs["graph"], outs["eager"]))
        if i >= warmup:
            frames += sum(n) // eng.hop
    row = {"sessions": sessions, "push_frames": push, "halo_frames": halo, "window_frames": push + 2 * halo,
           "steps": steps, "warmup": warmup, "frames_per_step": frames / steps}
    rate = eng.cfg["spec_transform"]["sampling_rate"]
    for k, v in ms.items():
        p50, p99 = float(np.percentile(v, 50)), float(np.percentile(v, 99))
        row[k] = {"p50_ms": p50, "p99_ms": p99, "audio_s_per_wall_s": frames / steps * eng.hop / rate / (p50 * 1e-3)}
    return row


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "token_stream.json"))
    args = ap.parse_args()
    from distilcodec_nabeel_amd import config, weights
    from distilcodec_nabeel_amd.engine import NativeCodec

    cfg = config.default_config()
    eng = NativeCodec(cfg, weights.synthetic_state_dict(cfg, seed=1234), "cuda:0", gemm="x6")
    rows = []
    print("| sessions | push | W | graph p50 / p99 ms | eager p50 / p99 ms | loop p50 / p99 ms | loop / graph | audio s per s (graph) |")
    print("|---|---|---|---|---|---|---|---|")
    for sessions in SESSIONS:
        for push in PUSHES:
            r = run_case(eng, sessions, push, args.steps, args.warmup)
            rows.append(r)
            g, e, l = r["graph"], r["eager"], r["loop"]
            print(f"| {sessions} | {push} | {r['window_frames']} | {g['p50_ms']:.2f} / {g['p99_ms']:.2f} | "
                  f"{e['p50_ms']:.2f} / {e['p99_ms']:.2f} | {l['p50_ms']:.2f} / {l['p99_ms']:.2f} | "
                  f"{l['p50_ms'] / g['p50_ms']:.1f}x | {g['audio_s_per_wall_s']:.0f} |", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "gemm": "x6", "weights": "synthetic (seed 1234)",
                   "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
