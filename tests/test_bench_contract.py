"""bench.py's output contract without a GPU: the roofline record computed from per-kernel HIP-event
timings (the dominant kernel, its achieved FLOP/s against the x6 or fp32 MFMA ceiling, the PMC
traffic committed in profiles/pmc_latest.json), the workload table (BASELINE.json configs[1] and
configs[3]), the CPU-baseline record (the oracle timed with all host threads and one), the
command line (a plain run against --full) and the --dump-outputs writer."""
import json
import os

import numpy as np
import pytest

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_roofline_picks_the_dominant_kernel():
    dom = "conv_gemm_x3dw_group<256,256,halo>"
    prof = {
        dom: {"launches": 20, "ms": 200.0, "flops": 20 * 2.6e12, "bytes": 0.0},
        "conv_gemm_f32<128,128>": {"launches": 4, "ms": 10.0, "flops": 1e12, "bytes": 0.0},
    }
    r = bench.roofline(prof, steps=2)
    assert r["kernel"] == dom
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s"
    assert abs(r["achieved"] - 20 * 2.6e12 / 0.2 / 1e12) < 0.01
    assert r["peak"] == round(bench.BF16_MFMA_PEAK_TFLOPS / 3, 1)  # h3: 3 fp16 products per fp32 product
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["launches_per_step"] == 10 and abs(r["avg_launch_ms"] - 10.0) < 1e-9
    assert abs(r["share_of_device_time"] - 200 / 210) < 1e-3
    # traffic: HBM bytes per launch of that kernel from the committed PMC pass, or None
    pmc = json.load(open(os.path.join(REPO, "profiles", "pmc_latest.json")))
    assert r["traffic"] == pmc["kernels"][dom]["hbm_bytes_per_launch"]
    assert bench.traffic_for("no_such_kernel") is None
    x6 = bench.roofline({"conv_gemm_x6dq<256,256,halo>": {"launches": 1, "ms": 1.0, "flops": 1e11, "bytes": 0}}, 1)
    assert x6["peak"] == round(bench.BF16_MFMA_PEAK_TFLOPS / 6, 1)
    f = bench.roofline({"conv_gemm_f32<128,128>": {"launches": 1, "ms": 1.0, "flops": 1e11, "bytes": 0}}, 1)
    assert f["peak"] == bench.FP32_MFMA_PEAK_TFLOPS
    assert bench.roofline({}, 1) is None


def test_workloads_are_the_baseline_configs():
    base = json.load(open(os.path.join(REPO, "BASELINE.json")))
    assert "batch=32 × 10 s" in base["configs"][1].replace("x", "×")
    assert bench.WORKLOADS["c2"] == (32, 240000, 240000)
    per_gpu, longest, shortest = bench.WORKLOADS["c4"]
    assert per_gpu * 8 == 1024 and longest == 240000 and shortest < longest


def test_cpu_baseline_record(cfg, state):
    rec = bench.cpu_baseline(cfg, state)
    assert rec["kind"] == "port" and rec["unit"] == "samples/s"
    assert rec["value"] > 0 and rec["value_1thread"] > 0
    assert rec["cores"] >= 1 and rec["cpu_model"]
    assert "median of 3" in rec["sample"]


def test_full_is_off_by_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    b = bench.parse_args(["--full", "--dump-outputs", "somewhere", "--no-c3"])
    assert b.full is True and b.dump_outputs == "somewhere" and b.no_c3
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_outputs_small_arrays_whole(tmp_path):
    codes = np.arange(3 * 5, dtype=np.int32).reshape(3, 5) * 2047
    wav = np.linspace(-1, 1, 3 * 40, dtype=np.float32).reshape(3, 40)
    d = str(tmp_path / "out")
    shapes = bench.dump_outputs(d, {"codes": codes, "wav": wav})
    assert shapes == {"codes": (3, 5), "wav": (3, 40)}
    assert sorted(os.listdir(d)) == ["codes.npy", "wav.npy"]
    c, w = np.load(os.path.join(d, "codes.npy")), np.load(os.path.join(d, "wav.npy"))
    assert c.dtype == np.float32 and np.array_equal(c, codes)  # code indices < 2^24: exact in float32
    assert w.dtype == np.float32 and np.array_equal(w, wav)
    bench.dump_outputs(d, {"x": np.ones((2, 2), dtype=np.float64)})
    assert np.load(os.path.join(d, "x.npy")).dtype == np.float64


def test_dump_outputs_samples_rows_within_the_budget(tmp_path):
    big = np.arange(100 * 256, dtype=np.float32).reshape(100, 256)  # 102400 bytes
    small = np.arange(100 * 4, dtype=np.int32).reshape(100, 4)      # 1600 bytes
    budget = 20000
    s1 = bench.dump_outputs(str(tmp_path / "a"), {"small": small, "big": big}, budget=budget)
    s2 = bench.dump_outputs(str(tmp_path / "b"), {"small": small, "big": big}, budget=budget)
    assert s1 == s2
    total = 0
    for n, full in (("small", small), ("big", big)):
        a, b = np.load(str(tmp_path / "a" / f"{n}.npy")), np.load(str(tmp_path / "b" / f"{n}.npy"))
        assert np.array_equal(a, b)  # the same sample from run to run
        assert 1 <= a.shape[0] < 100 and a.shape[1:] == full.shape[1:]
        rows = (a[:, 0] // full.shape[1]).astype(int)  # row r of either array starts at r * width
        assert np.all(np.diff(rows) > 0) and np.array_equal(a, full[rows].astype(np.float32))
        total += a.nbytes
    assert total <= budget
    assert bench.DUMP_BUDGET_BYTES <= 64 * 1000 * 1000
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "c"), {"big": big}, budget=100)
