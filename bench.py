#!/usr/bin/env python3
"""Throughput benchmark of the MI355X DistilCodec encode -> VQ -> decode path.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c2|c4] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N [--full]

A plain run does only what the headline figure needs: it builds the engine and the resident batch,
runs W untimed and K timed steps, writes the last step's outputs when --dump-outputs is given, and
prints the result line (`value`, `ms_per_step`; the sub-records below are null).  Everything else
the benchmark measures or checks runs only with --full.

Workloads (BASELINE.json configs):
  c2 (default; configs[1]): 32 synthetic 10 s 24 kHz clips PER GPU (speech-like / music-like),
     fp32, the full path mel -> ConvNeXt encoder -> GRFVQ search -> decode(codes) -> HiFiGAN
     generator, i.e. `DistilCodec.encode` followed by `decode_from_codes`.
  c4 (configs[3]): 128 ragged universal-audio clips (9-10 s, speech+music) per GPU, global batch
     128 N (1024 on 8 GPUs), every shard padded to the GLOBAL maximum.
Both run through the shipped multi-GPU path (`sharding.ShardedEncodeDecode`): rank r holds its
contiguous shard of the global clip list, resident in HBM; a step = `dcx_encode_decode` over the
shard plus the all_gather of every rank's codes (RCCL over xGMI).  Clips are independent, so there
is no collective on the data path (weak scaling); the gather is the only exchange.  With --full and
the default c2 workload the same line carries sub-records (each skippable by a flag):
  "c4"             a C4 pass (128 ragged clips per GPU, padded to the global max), at every N;
  "c3"             (N = 1) configs[2]: encoder + GRFVQ token extraction, 256 x 10 s, bf16;
  "c5"             (N = 1) configs[4]: 1 s hops through one captured hipGraph (split-K latency mode);
  "codes_vs_oracle" (N = 1) the first, middle and last clip of the timed C2 batch against the CPU oracle: decisive codes
                   exact, the raw code match rate and the waveform SNR (the metric's "code-index
                   bit-exact vs CPU" clause, measured on the benchmarked workload).

Rank 0 prints one JSON line.  `value` counts real (unpadded) clip samples of all ranks per second.
--dump-outputs DIR writes what the last timed step returned to its caller, DIR/codes.npy (the
gathered codes) and DIR/wav.npy (this rank's waveforms), as float32, at most 64 MB in all (a fixed,
seeded sample of the rows of a larger array).  Clips and weights are seeded, so two builds run with
the same arguments can be compared output for output.
With --full, `roofline` reports the dominant kernel (largest summed device time, HIP events around
each launch on its stream during the timed steps) as algorithmic FLOP/s against its MFMA ceiling;
`cpu_baseline` times the CPU oracle (the reference's algorithm on PyTorch-CPU,
oracle/reference_cpu.py) on a bounded sample on this host, all cores and 1 thread, median of 3.
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import statistics
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from distilcodec_nabeel_amd import config as dconfig  # noqa: E402
from distilcodec_nabeel_amd import sharding, synth, weights  # noqa: E402
from distilcodec_nabeel_amd.engine import NativeCodec  # noqa: E402

FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 (= fp32 vector peak)
BF16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA
# x6 mode executes 6 exact bf16 products per fp32 product: its ceiling in fp32-algorithmic FLOP/s
X6_PEAK_TFLOPS = BF16_MFMA_PEAK_TFLOPS / 6
# h3 (the wide convs since round 5): 3 exact fp16 products per fp32 product, fp16 MFMA at the bf16 rate
H3_PEAK_TFLOPS = BF16_MFMA_PEAK_TFLOPS / 3
HBM_PEAK_GBS = 8000.0
SR = 24000
MFLOP_PER_FRAME = 2045.08  # encode -> decode algorithmic work per 256-sample frame
C3_MFLOP_PER_FRAME = 415.36  # encode-only (mel excluded) per frame

WORKLOADS = {
    # clips per GPU, longest clip, shortest clip
    "c2": (32, 240000, 240000),
    "c4": (128, 240000, 216000),
}


def traffic_for(kernel: str):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC pass (profiles/pmc_latest.json:
    2*FETCH_SIZE + WRITE_SIZE, gfx950 correction), or None when that kernel was not profiled."""
    path = os.path.join(HERE, "profiles", "pmc_latest.json")
    try:
        with open(path) as f:
            d = json.load(f)
        return d["kernels"][kernel]["hbm_bytes_per_launch"]
    except (OSError, KeyError, ValueError):
        return None


def _cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def _host_threads() -> int:
    """The CPU share this process may use: the affinity mask, capped by OMP_NUM_THREADS when set
    (16 on the GPU box, whose os.cpu_count() shows the whole machine)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    omp = os.environ.get("OMP_NUM_THREADS")
    return max(1, min(n, int(omp))) if omp and omp.isdigit() else n


def cpu_baseline(cfg, state):
    """Oracle (PyTorch-CPU restatement of the reference) on bounded samples of the
    C2 workload: 1 warm-up then the median of 3 runs, with all host threads and with 1 thread."""
    from oracle import reference_cpu as R

    def timed(batch, n, threads, seed):
        torch.set_num_threads(threads)
        R.encode_decode(R.pad_batch(synth.clips(1, SR // 4, seed=999))[0], state, cfg)  # warm-up
        audio, _ = R.pad_batch(synth.clips(batch, n, seed=seed, kind="mix"))
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            R.encode_decode(audio, state, cfg)
            runs.append(time.perf_counter() - t0)
        return batch * n / statistics.median(runs), runs

    threads = _host_threads()
    v_all, runs_all = timed(2, 5 * SR, threads, 0)
    v_one, runs_one = timed(1, SR, 1, 0)
    torch.set_num_threads(threads)
    return {"value": round(v_all, 1), "unit": "samples/s", "cores": threads, "kind": "port",
            "cpu_model": _cpu_model(), "host_cpu_count": os.cpu_count(),
            "value_1thread": round(v_one, 1),
            "sample": (f"full encode->VQ->decode, fp32, oracle/reference_cpu.py, 1 warm-up + median of 3: "
                       f"{threads} threads on 2 x 5 s clips (runs {', '.join(f'{r:.2f}' for r in runs_all)} s); "
                       f"1 thread on 1 x 1 s clip (runs {', '.join(f'{r:.2f}' for r in runs_one)} s)")}


def c3_record(cfg, state, dev, steps: int = 3, batch: int = 256):
    """BASELINE configs[2] (C3): mel -> encoder -> GRFVQ codes of 256 x 10 s clips in bf16 (the
    reference's enable_bfloat16), inputs resident in HBM, codes only; one warm-up step, `steps`
    timed with HIP events; the dominant kernel (HIP events per launch, one more step) against the
    dense bf16 MFMA peak and against its own product-count ceiling."""
    n = 10 * SR
    audio = torch.zeros(batch, n + 1)
    for i, c in enumerate(synth.clips(batch, n, seed=0, kind="mix")):
        audio[i, 1:] = torch.from_numpy(c)
    audio = audio.to(dev)
    eng = NativeCodec(cfg, state, dev, with_generator=False, gemm="bf16")
    T = eng.num_frames(n + 1)

    def step():
        return eng.vq_encode(eng.encode(eng.mel(audio)), want_pjt_in=False, want_fup=False, want_quantized=False)[0]

    codes = step()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        codes = step()
    e1.record()
    torch.cuda.synchronize(dev)
    ms = e0.elapsed_time(e1) / steps
    assert int(codes.min()) >= 0 and int(codes.max()) < cfg["quantizer"]["codebook_size"]
    # per-launch timing on one stream (DCX_ENC_STREAMS=0): the timed steps run the encoder's two
    # half-batches on two streams, where a launch's HIP-event span includes the other
    # half's concurrent work; same kernels, same bits
    with eng.knobs(DCX_ENC_STREAMS=0):
        eng.profile(True)
        eng.profile_reset()
        step()
        kern = eng.profile_read()
        eng.profile(False)
    name, rec = max(kern.items(), key=lambda kv: kv[1]["ms"])
    prods = 1 if "prefilter_b1" in name else 2 if "prefilter_b" in name else 1
    ach = rec["flops"] / (rec["ms"] * 1e-3) / 1e12
    flops = C3_MFLOP_PER_FRAME * 1e6 * batch * T
    out = {"workload": f"C3: encoder + GRFVQ token extraction, {batch} x 10 s, bf16 (enable_bfloat16), codes only",
           "value": round(batch * n / (ms * 1e-3), 1), "unit": "samples/s", "ms_per_step": round(ms, 3),
           "steps": steps, "warmup": 1, "tflops_algorithmic": round(flops / (ms * 1e-3) / 1e12, 1),
           "frac_of_bf16_dense": round(flops / (ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS, 4),
           "dominant_kernel": {"kernel": name, "achieved": round(ach, 1), "unit": "TFLOP/s",
                               "frac_of_bf16_dense": round(ach / BF16_MFMA_PEAK_TFLOPS, 4),
                               "products_per_flop": prods,
                               "frac_of_product_ceiling": round(ach * prods / BF16_MFMA_PEAK_TFLOPS, 4),
                               "avg_launch_ms": round(rec["ms"] / rec["launches"], 4),
                               "share_of_device_time": round(rec["ms"] / sum(v["ms"] for v in kern.values()), 4),
                               "timing": "HIP events per launch over one more step on one stream (DCX_ENC_STREAMS=0)"}}
    del eng
    torch.cuda.empty_cache()
    return out


def c5_record(eng, hops: int = 100, warmup: int = 10, split_k: int = 16):
    """BASELINE configs[4] (C5): B = 1, 1 s hops, each hop's encode -> decode one hipGraph replay
    (streaming.GraphedHop) in the split-K latency mode; HIP events around each replay."""
    from distilcodec_nabeel_amd.streaming import GraphedHop

    n = SR
    stream = np.concatenate(synth.clips(1, n * (hops + warmup), seed=3, kind="speech"))
    chunks = torch.from_numpy(stream.reshape(-1, 1, n).astype(np.float32)).to(eng.device)
    eng.set_split_k(split_k)
    try:
        hop = GraphedHop(eng, n)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(hops)]
        for i in range(warmup):
            hop(chunks[i])
        torch.cuda.synchronize(eng.device)
        for i in range(hops):
            ev[i][0].record()
            hop(chunks[warmup + i])
            ev[i][1].record()
        torch.cuda.synchronize(eng.device)
        ms = np.array([a.elapsed_time(b) for a, b in ev])
        del hop
    finally:
        eng.set_split_k(0)
    return {"workload": "C5: streaming encode->decode, 1 s hops (24000 samples, B = 1), one hipGraph replay per hop, "
                        f"split-K latency mode (<= {split_k} slices)",
            "hops": hops, "warmup": warmup, "p50_ms": round(float(np.percentile(ms, 50)), 4),
            "p99_ms": round(float(np.percentile(ms, 99)), 4), "mean_ms": round(float(ms.mean()), 4),
            "real_time_factor_p99": round(float(np.percentile(ms, 99)) / 1000.0, 5)}


def codes_vs_oracle(eng, runner, cfg, state):
    """The first, middle and last clip of the timed C2 batch (full 10 s each) against the CPU oracle
    (oracle/reference_cpu.py, the reference's algorithm on PyTorch-CPU): codes exact on every decisive
    frame (fp64 relative top-2 gap > 1e-4, computed with torch fp64 on the GPU), the raw exact-match
    rate, and the waveform SNR (of the reference's codes decoded on the GPU when a non-decisive code
    differs).  Equal-length clips: each clip alone is the batch's clip (tests/test_gpu_api.py)."""
    from oracle import reference_cpu as R

    torch.set_num_threads(_host_threads())
    nb = runner.audio.shape[0]
    clips = sorted({0, nb // 2, nb - 1})
    E = R.codebook(state["quantizer"]).to(eng.device, torch.float64)
    e2 = (E ** 2).sum(1)
    frames = dec_frames = matches = 0
    decisive_exact, snrs, t_ref, of = True, [], 0.0, []
    for c in clips:
        audio = runner.audio[c:c + 1].cpu()
        t0 = time.perf_counter()
        ref = R.encode_decode(audio, state, cfg)
        t_ref += time.perf_counter() - t0
        rc = ref["codes"][0, :, :, 0].numpy()
        gc = runner.codes[c:c + 1].cpu().numpy().astype(np.int64)
        x = ref["x_pjt_in"].reshape(-1, ref["x_pjt_in"].shape[-1]).to(eng.device, torch.float64)
        d = (x ** 2).sum(1)[:, None] + e2[None, :] - 2.0 * x @ E.T
        v, _ = torch.topk(d, 2, dim=1, largest=False)
        decisive = (((v[:, 1] - v[:, 0]) / v[:, 0]) > 1e-4).cpu().numpy().reshape(rc.shape)
        del x, d
        same = np.array_equal(gc, rc)
        wav = runner.wav[c:c + 1] if same else eng.generate(eng.vq_decode(torch.from_numpy(rc).to(torch.int32)))
        w, r = wav.double().cpu().numpy().reshape(-1), ref["wav"][:, 0].double().numpy().reshape(-1)
        snrs.append(round(float(10 * np.log10((r ** 2).sum() / max(((w - r) ** 2).sum(), 1e-300))), 2))
        of.append("own codes" if same else "reference's codes")
        frames += gc.size
        dec_frames += int(decisive.sum())
        matches += int((gc == rc).sum())
        decisive_exact = decisive_exact and bool(np.array_equal(gc[decisive], rc[decisive]))
    return {"clips": f"clips {clips} of the timed C2 batch (10 s each), oracle/reference_cpu.py fp32 on the host CPU",
            "frames": int(frames), "decisive_frames": int(dec_frames), "decisive_exact": decisive_exact,
            "match_rate": round(matches / frames, 6), "waveform_snr_db": snrs,
            "waveform_of": of, "oracle_seconds": round(t_ref, 2)}


DUMP_BUDGET_BYTES = 64 * 1000 * 1000


def dump_outputs(path: str, arrays: dict, budget: int = DUMP_BUDGET_BYTES, seed: int = 0) -> dict:
    """Write each array as `path`/<name>.npy in float32 (float64 stays float64), `budget` bytes at
    most in all.  An array over its share of the budget (split in proportion to the sizes) is cut
    to a sample of its rows: sorted indices drawn without replacement from PCG64(seed), the same
    for every run of the same shapes.  Returns name -> the saved shape."""
    os.makedirs(path, exist_ok=True)
    out = {n: np.asarray(a) for n, a in arrays.items()}
    out = {n: a if a.dtype == np.float64 else a.astype(np.float32) for n, a in out.items()}
    total = sum(a.nbytes for a in out.values())
    shapes = {}
    for i, (name, a) in enumerate(out.items()):
        share = budget if total <= budget else budget * a.nbytes // total
        if a.nbytes > share:
            row_bytes = max(1, a.nbytes // a.shape[0])
            keep = share // row_bytes
            if keep < 1:
                raise ValueError(f"one row of {name} ({row_bytes} bytes) is over its share of the {budget}-byte budget")
            rows = np.sort(np.random.Generator(np.random.PCG64(seed + i)).choice(a.shape[0], size=keep, replace=False))
            a = a[rows]
        np.save(os.path.join(path, f"{name}.npy"), np.ascontiguousarray(a))
        shapes[name] = tuple(a.shape)
    return shapes


def make_runner(eng, workload: str, rank: int, world: int, seed: int = 0):
    per_gpu, longest, shortest = WORKLOADS[workload]
    n_total = per_gpu * world
    lengths = synth.ragged_lengths(n_total, seed + 7, longest, shortest)
    s, e = sharding.shard_bounds(n_total, rank, world)
    clips = synth.batch_clips(lengths, s, e, seed=seed)
    runner = sharding.ShardedEncodeDecode(eng, clips, max(lengths), n_total, rank, world)
    return runner, sum(lengths), n_total


def run_timed(runner, steps: int, warmup: int, world: int, dev, profile_eng=None):
    """W untimed steps, then K steps between barrier + synchronize; max over ranks.  Returns the
    seconds, the per-kernel profile and what the last timed step returned (all codes, local wav)."""
    for _ in range(warmup):
        runner.step()
    torch.cuda.synchronize(dev)
    codes = runner.codes
    if codes.numel():
        assert int(codes.min()) >= 0 and int(codes.max()) < 32768
        assert bool(torch.isfinite(runner.wav).all())
    if profile_eng is not None:
        profile_eng.profile(True)
        profile_eng.profile_reset()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        all_codes, wav = runner.step()
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    prof = {}
    if profile_eng is not None:
        prof = profile_eng.profile_read()
        profile_eng.profile(False)
    if world > 1:
        t = torch.tensor([dt], device=dev if dist.get_backend() != "gloo" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        assert all_codes.shape[0] == runner.n_total
    return dt, prof, (all_codes, wav)


def roofline(prof: dict, steps: int):
    if not prof:
        return None
    name, rec = max(prof.items(), key=lambda kv: kv[1]["ms"])
    avg_ms = rec["ms"] / rec["launches"]
    achieved = rec["flops"] / (rec["ms"] * 1e-3) / 1e12
    peak = H3_PEAK_TFLOPS if "x3" in name else X6_PEAK_TFLOPS if "x6" in name else FP32_MFMA_PEAK_TFLOPS
    return {"bound": "mfma", "kernel": name, "achieved": round(achieved, 2), "peak": round(peak, 1),
            "unit": "TFLOP/s", "frac": round(achieved / peak, 4), "traffic": traffic_for(name),
            "traffic_source": "committed PMC figure (profiles/pmc_latest.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE "
                              "passes over bench.py, 2*FETCH + WRITE per launch), not measured in this run",
            "peak_basis": ("dense fp16 MFMA 2500 TF / 3 fp16 products per fp32 product (h3)" if "x3" in name
                           else "bf16 dense MFMA 2500 TF / 6 bf16 products per fp32 product" if "x6" in name
                           else "fp32 MFMA v_mfma_f32_32x32x2_f32"),
            "launches_per_step": rec["launches"] // steps, "avg_launch_ms": round(avg_ms, 4),
            "flops_per_launch": rec["flops"] / rec["launches"],
            "share_of_device_time": round(rec["ms"] / sum(r["ms"] for r in prof.values()), 4)}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5, help="timed steps (>= 1)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", choices=sorted(WORKLOADS), default="c2")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's codes and waveforms to DIR/<name>.npy (float32, <= 64 MB)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline figure: the per-launch roofline timing, the "
                         "codes_vs_oracle check, the C4 / C5 / f32_ieee / C3 sub-records and the CPU baseline "
                         "(each skippable by its --no-* flag, which has no effect without --full)")
    ap.add_argument("--no-c4", action="store_true", help="skip the extra C4 pass")
    ap.add_argument("--no-c3", action="store_true", help="skip the C3 token-extraction sub-record (N = 1)")
    ap.add_argument("--no-c5", action="store_true", help="skip the C5 streaming-hop sub-record (N = 1)")
    ap.add_argument("--no-oracle-codes", action="store_true", help="skip the codes_vs_oracle check (N = 1)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-f32", action="store_true", help="skip the IEEE fp32-MFMA comparison pass at N = 1")
    ap.add_argument("--no-profile", action="store_true", help="skip the per-launch HIP-event roofline timing")
    ap.add_argument("--gemm", choices=["x6", "f32"], default="x6",
                    help="x6 (DCX_GEMM_X6): fp32-tolerance emulation, h3 (2 fp16 values, 3 products) for the wide "
                         "generator convs and the ConvNeXt 1x1 convs, x6 (3 bf16 planes, 6 products) elsewhere, fp32 "
                         "accumulation; f32: IEEE fp32 MFMA")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    return args


def main():
    args = parse_args()
    full = args.full

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # DCX_BENCH_ONE_DEVICE=1 (tests/test_gpu_bench_dist.py): rehearse the N > 1 path on a one-GPU box,
    # every rank on cuda:0 and gloo for the collectives (RCCL refuses two ranks on one device); the
    # driver's multi-GPU runs use one GPU per rank and RCCL ("nccl")
    one_dev = os.environ.get("DCX_BENCH_ONE_DEVICE") == "1"
    if one_dev:
        local = 0
    if world > 1:
        torch.cuda.set_device(local)
        if one_dev:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    dev = torch.device("cuda", local)

    cfg = dconfig.default_config()
    state = weights.synthetic_state_dict(cfg, seed=1234)
    eng = NativeCodec(cfg, state, dev, gemm=args.gemm)

    runner, samples, n_total = make_runner(eng, args.config, rank, world)
    dt, prof, last = run_timed(runner, args.steps, args.warmup, world, dev, eng if full and not args.no_profile else None)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"codes": last[0].cpu().numpy(), "wav": last[1].cpu().numpy()})
    del last
    ms_step = dt / args.steps * 1e3
    value = samples / (dt / args.steps)
    padded = n_total * (runner.audio.shape[1] - 1)
    frames = runner.frames
    roof = roofline(prof, args.steps)
    if roof and rank == 0 and os.environ.get("DCX_BENCH_KERNELS"):
        with open(os.environ["DCX_BENCH_KERNELS"], "w") as f:
            json.dump({"steps": args.steps, "kernels": prof}, f, indent=1)

    oracle_codes = None
    if full and world == 1 and args.config == "c2" and not args.no_oracle_codes:
        oracle_codes = codes_vs_oracle(eng, runner, cfg, state)

    c4 = None
    if full and args.config == "c2" and not args.no_c4:
        r4, s4, n4 = make_runner(eng, "c4", rank, world)
        k4 = min(args.steps, 3 if world > 1 else 2)
        dt4, _, _ = run_timed(r4, k4, 1, world, dev)
        c4 = {"workload": f"C4: {n4} ragged clips (9-10 s, speech+music), {n4 // world} per GPU, padded to the global max",
              "value": round(s4 / (dt4 / k4), 1), "unit": "samples/s (real, unpadded)",
              "ms_per_step": round(dt4 / k4 * 1e3, 3), "steps": k4, "warmup": 1, "global_batch": n4,
              "n_gpus": world}
        del r4
        torch.cuda.empty_cache()

    c5 = None
    if full and world == 1 and args.config == "c2" and args.gemm == "x6" and not args.no_c5:
        c5 = c5_record(eng)

    f32 = None
    if full and world == 1 and args.gemm == "x6" and not args.no_f32:
        eng.set_gemm("f32")
        kf = min(args.steps, 2)
        dtf, _, _ = run_timed(runner, kf, 1, world, dev)
        eng.set_gemm("x6")
        f32 = {"value": round(samples / (dtf / kf), 1), "unit": "samples/s", "ms_per_step": round(dtf / kf * 1e3, 3),
               "steps": kf, "arith": "IEEE fp32 MFMA (v_mfma_f32_32x32x2_f32), same workload",
               "tflops": round(samples / 256 * MFLOP_PER_FRAME * 1e6 / (dtf / kf) / 1e12, 1)}

    c3 = None
    if full and world == 1 and args.config == "c2" and not args.no_c3:
        del runner
        eng._ws = None  # the C2 / C4 workspace is not needed by the token-extraction handle
        torch.cuda.empty_cache()
        c3 = c3_record(cfg, state, dev)

    cpu = None
    if full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(cfg, state)

    if rank == 0:
        per_gpu, longest, shortest = WORKLOADS[args.config]
        workload = (f"C2: {per_gpu} x 10 s clips per GPU, full mel->encoder->VQ->decode->generator, fp32"
                    if args.config == "c2" else
                    f"C4: {n_total} ragged clips (9-10 s, speech+music), {per_gpu} per GPU, padded to the global max, "
                    f"full path, fp32")
        out = {
            "metric": "24 kHz samples/s encode+decode at 1/8 GPU; code-index bit-exact vs CPU",
            "value": round(value, 1),
            "unit": "samples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "arith": ("fp32-tolerance emulation (h3 / x6), not IEEE fp32: the wide generator convs and the ConvNeXt "
                      "1x1 convs as 2 fp16 values per operand (h, l; 22 significant bits, each operand tensor scaled "
                      "per clip or row by a power of two from a rigorous bound of its range), 3 exact fp16 products "
                      "per fp32 product (v_mfma_f32_16x16x32_f16, 'h3'); the rest as 3 bf16 planes (24 bits, the "
                      "fp32 exponent range), 6 exact bf16 products (v_mfma_f32_16x16x32_bf16 / 32x32x16_bf16, 'x6'); "
                      "fp32 accumulation; held to the fp32 tolerance of the contract (codes exact on decisive frames, "
                      ">= 80 dB); the IEEE fp32-MFMA figure is f32_ieee"
                      if args.gemm == "x6" else "IEEE fp32 MFMA (v_mfma_f32_32x32x2_f32)"),
            "data": "synthetic (speech/music-like 24 kHz clips; seeded synthetic weights, no checkpoint offline)",
            "config": {"workload": workload, "global_batch": n_total, "clip_samples_max": longest,
                       "frames_per_clip": frames, "parallelism": f"clip-sharded x{world}, codes all_gather",
                       "streams": ("per GPU, two half-batches on two HIP streams up to the generator, the generator "
                                   "on the whole shard (DCX_ENC_STREAMS=%d; same bits as one stream)"
                                   % eng.get_knob("DCX_ENC_STREAMS")),
                       "padded_samples_per_s": round(padded / (dt / args.steps), 1)},
            "tflops_algorithmic": round(padded / 256 * MFLOP_PER_FRAME * 1e6 / (dt / args.steps) / 1e12, 1),
            "roofline": roof,
            "f32_ieee": f32,
            "codes_vs_oracle": oracle_codes,
            "c4": c4,
            "c3": c3,
            "c5": c5,
            "cpu_baseline": cpu,
        }
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
