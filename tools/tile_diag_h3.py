#!/usr/bin/env python3
"""Per-tile stamps of the conv_gemm_x3dw forms as the stages launch them (needs a library built with
-DDCX_TILE_DIAG, which exports dcx_diag_tiles; select it with DCX_LIB=...).

    bash tools/build_variant.sh libdcx_tile -DDCX_TILE_DIAG
    DCX_LIB=$PWD/distilcodec_nabeel_amd/libdcx_tile.so python tools/tile_diag_h3.py [--batch 32] [--frames 937]

Each workgroup stamps s_memrealtime (100 MHz) at entry, main-loop start, main-loop end and exit, with
its CU's hardware ids and its step count.  The tiles of one module call are cut into launches at the
gaps of the entry stamps (the launches of a stream run one after the other) and each launch's tiles
grouped by step count (the members of a grouped launch differ in taps).  Printed per launch and member:
tiles, median prologue / loop / epilogue in us, the median gap between consecutive tiles on a CU, and
the share of the launch's CU time outside main loops.

Launch order of a ParallelBlock (dcx_generator.cpp): c1 group, c2 group, c1 group, c2 group, c1 group,
then the three convs of the mean chain (MEAN_FIRST, MEAN_MID, MEAN_LAST); of a ConvNeXt block: pwconv1
(EPI_GELU), pwconv2 (EPI_GAMMA_RES).
"""
import argparse
import ctypes
import os
import sys
from collections import defaultdict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distilcodec_nabeel_amd import _native, config, weights  # noqa: E402
from distilcodec_nabeel_amd.engine import NativeCodec  # noqa: E402

PBLOCK = ["c1 group (silu h2)", "c2 group (EPI_RES, fp32 + h2)", "c1 group", "c2 group (in place)", "c1 group",
          "MEAN_FIRST", "MEAN_MID", "MEAN_LAST"]
BLOCK = ["pwconv1 (EPI_GELU, h2 rows)", "pwconv2 (EPI_GAMMA_RES)"]


def launches(t):
    """Tiles (rows of 6 words, any order) -> lists of rows, one per launch, in time order."""
    t = t[np.argsort(t[:, 0])]
    out, cur, end = [], [t[0]], t[0][3]
    for row in t[1:]:
        if row[0] > end:  # entered after every earlier tile had left: a new launch
            out.append(np.array(cur))
            cur = []
        cur.append(row)
        end = max(end, row[3])
    out.append(np.array(cur))
    return out


def report(label, t):
    us = lambda v: float(v) / 100.0  # noqa: E731
    steps = t[:, 5] >> 16
    cus = defaultdict(list)
    for row in t:
        cus[(int(row[5]) & 0xFFFF, (int(row[4]) >> 8) & 0xFF)].append(row)
    gaps = []
    for rows in cus.values():
        rows.sort(key=lambda z: z[0])
        gaps += [rows[i + 1][0] - rows[i][3] for i in range(len(rows) - 1)]
    span = t[:, 3].max() - t[:, 0].min()
    outside = 1.0 - (t[:, 2] - t[:, 1]).sum() / (len(cus) * span)
    print(f"  {label:32s} span {us(span):8.1f} us  {len(t):5d} tiles on {len(cus):3d} CUs  gap {us(np.median(gaps)) if gaps else 0:6.1f} us  "
          f"outside loops {outside:.3f}")
    for s in sorted(set(steps.tolist())):
        m = t[steps == s]
        pro, loop, epi = m[:, 1] - m[:, 0], m[:, 2] - m[:, 1], m[:, 3] - m[:, 2]
        print(f"      steps {s:4d}: {len(m):5d} tiles  prologue {us(np.median(pro)):6.1f}  loop {us(np.median(loop)):7.1f}  "
              f"epilogue {us(np.median(epi)):6.1f} us (p90 {us(np.percentile(epi, 90)):6.1f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=937)
    a = ap.parse_args()
    cfg = config.default_config()
    eng = NativeCodec(cfg, weights.synthetic_state_dict(cfg, seed=1234), "cuda:0", gemm="x6")
    f = _native.lib().dcx_diag_tiles
    f.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
    nmax = 16384
    buf = (ctypes.c_ulonglong * (6 * nmax))()
    g = torch.Generator().manual_seed(0)
    rates = np.cumprod(cfg["decoder"]["upsample_rates"])
    cases = [(f"generator.resblocks.{i}", cfg["decoder"]["upsample_initial_channel"] >> (i + 1), a.frames * int(rates[i]), PBLOCK)
             for i in range(3)]
    cases += [("encoder.stages.1.0", cfg["encoder"]["dims"][1], a.frames, BLOCK)]
    for name, C, L, labels in cases:
        B = a.batch
        bm, bn = (256, 256) if C % 256 == 0 else (384, 128)
        convs = 18 if labels is PBLOCK else 5  # (pwconv1 has 4 C columns, pwconv2 C)
        while B * -(-L // bm) * (C // bn) * convs > nmax and B > 1:
            B //= 2  # keep the whole call's tiles inside the stamp buffer
        x = torch.randn(B, L, C, generator=g).to("cuda:0")
        for _ in range(2):
            eng.module(name, x)
        torch.cuda.synchronize()
        f(buf, nmax, 1)
        eng.module(name, x)
        torch.cuda.synchronize()
        n = f(buf, nmax, 1)
        print(f"{name}  B {B}  rows {L}  C {C}: {n} tiles", flush=True)
        if n <= 0:
            continue
        t = np.ctypeslib.as_array(buf)[: 6 * n].reshape(n, 6).astype(np.int64)
        ls = launches(t)
        for i, lt in enumerate(ls):
            report(labels[i] if len(ls) == len(labels) else f"launch {i}", lt)


if __name__ == "__main__":
    main()
