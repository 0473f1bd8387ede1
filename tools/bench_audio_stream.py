#!/usr/bin/env python
"""Push latency of the batched audio stream (streaming.AudioStream) on the published geometry with
synthetic weights, every slot pushing push_samples samples per step.  The ways to run the same step
alternate inside one process:

  graph     the step replayed from its one captured HIP graph (AudioStream(graph=True));
  eager     the same step launched eagerly;
  halo      what the package offered before: `sessions` HaloStream(push_samples=..., graph=True) objects
            pushed in turn (each cuts its windows with torch ops on the host path, keeps its state in
            Python, and also decodes: its push returns audio, so it includes the generator half);
  halo_enc  only the encoder-window graph of each of those HaloStreams replayed in turn: the
            tokenizing share of `halo` without its host work, a lower bound of it.

Every timed step starts from an idle device (a synchronise), is bracketed by HIP events and includes
its host-side work (staging, upload, launches, the copy of the emitted codes).  The median (and p99)
over `--steps` steps after `--warmup` untimed ones.  Writes profiles/audio_stream.json and prints the
table of DESIGN.md §5 "Audio streams".
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

CASES = ((1, 2048), (8, 2048), (32, 2048), (8, 8192))


def _timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def run_case(eng, sessions: int, push: int, steps: int, warmup: int, seed: int = 0) -> dict:
    from distilcodec_nabeel_amd.streaming import AudioStream, HaloStream

    graph, eager = AudioStream(eng, sessions, push, graph=True), AudioStream(eng, sessions, push)
    halos = [HaloStream(eng, push_samples=push, graph=True) for _ in range(sessions)]

    def halo_push(chunks):
        return [h.push(c) for h, c in zip(halos, chunks)]

    def halo_enc(_):
        for h in halos:
            h.graphs[0].replay()

    ways = {"graph": graph.push, "eager": eager.push, "halo": halo_push, "halo_enc": halo_enc}
    rng = np.random.default_rng(seed)
    ms = {k: [] for k in ways}
    frames = 0
    for i in range(warmup + steps):
        chunks = [(0.1 * rng.standard_normal(push)).astype(np.float32) for _ in range(sessions)]
        outs = {}
        for k, fn in ways.items():  # alternating: the ways see the same step back to back
            t, outs[k] = _timed(lambda fn=fn: fn(chunks))
            if i >= warmup:
                ms[k].append(t)
        assert all(torch.equal(a, b) for a, b in zip(outs["graph"], outs["eager"]))
        if i >= warmup:
            frames += sum(o.shape[0] for o in outs["graph"])
    row = {"sessions": sessions, "push_samples": push, "halo_frames": graph.halo_frames,
           "window_frames": graph.window_frames, "steps": steps, "warmup": warmup, "frames_per_step": frames / steps}
    rate = eng.cfg["spec_transform"]["sampling_rate"]
    for k, v in ms.items():
        p50, p99 = float(np.percentile(v, 50)), float(np.percentile(v, 99))
        row[k] = {"p50_ms": p50, "p99_ms": p99}
    row["audio_s_per_wall_s_graph"] = sessions * push / rate / (row["graph"]["p50_ms"] * 1e-3)
    return row


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "audio_stream.json"))
    args = ap.parse_args()
    from distilcodec_nabeel_amd import config, weights
    from distilcodec_nabeel_amd.engine import NativeCodec

    cfg = config.default_config()
    eng = NativeCodec(cfg, weights.synthetic_state_dict(cfg, seed=1234), "cuda:0", gemm="x6")
    rows = []
    print("| sessions | push samples | Wf | graph p50 / p99 ms | eager p50 / p99 ms | halo p50 / p99 ms | halo_enc p50 ms | halo / graph | audio s per s (graph) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for sessions, push in CASES:
        r = run_case(eng, sessions, push, args.steps, args.warmup)
        rows.append(r)
        g, e, l, le = r["graph"], r["eager"], r["halo"], r["halo_enc"]
        print(f"| {sessions} | {push} | {r['window_frames']} | {g['p50_ms']:.2f} / {g['p99_ms']:.2f} | "
              f"{e['p50_ms']:.2f} / {e['p99_ms']:.2f} | {l['p50_ms']:.2f} / {l['p99_ms']:.2f} | {le['p50_ms']:.2f} | "
              f"{l['p50_ms'] / g['p50_ms']:.1f}x | {r['audio_s_per_wall_s_graph']:.0f} |", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "gemm": "x6", "weights": "synthetic (seed 1234)",
                   "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
