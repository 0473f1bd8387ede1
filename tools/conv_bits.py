"""Bits of every conv kernel, for comparing two trees: run in each and diff the listings.

Walks the KERNELS table of tests/test_gpu_conv.py with its fixed seeds and prints `kernel name,
sha256(output)` per row and length; then generate, encode and the split-K generate of
tests/test_gpu_splitk.py::test_grouped_split_launches (T = 24) on the golden e2e_batch input, with the
default knobs and with DCX_H3 = DCX_H3_1X1 = DCX_H3_PAIRS = 0.  Usage: python tools/conv_bits.py > bits.txt
"""
import contextlib
import hashlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import test_gpu_conv as T  # noqa: E402
from distilcodec_nabeel_amd import config, weights  # noqa: E402
from distilcodec_nabeel_amd.engine import NativeCodec  # noqa: E402


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()[:32]


for shape, mode, kern, Ls in T.KERNELS:
    conv = T._conv(shape, mode)
    for L in Ls:
        x, res = T._data(shape, L)
        if mode == "bf16":
            out = (conv(x.cuda(), gemm="bf16"),)
        else:
            out = conv(x.cuda(), gemm="f32" if mode == "f32" else "x6", epi=3, res=res.cuda(), want_silu=True)
        print(f"{conv.last_kernel} {T._sid(shape)} {mode} L={L}, {sha(*out)}")

cfg = config.default_config()
state = weights.synthetic_state_dict(cfg, seed=1234)
g = dict(np.load(os.path.join(REPO, "tests", "golden", "e2e_batch.npz")))
eng = NativeCodec(cfg, state, "cuda:0", gemm="x6")
split = NativeCodec(cfg, state, "cuda:0", gemm="x6")
split.set_split_k(16)
z = torch.from_numpy(g["quantized"]).transpose(1, 2)
mel = torch.from_numpy(g["mel"]).transpose(1, 2)
z24 = torch.randn(1, 24, 1024, generator=torch.Generator().manual_seed(124)) * 0.5
for label, knobs in (("defaults", {}), ("h3 off", {"DCX_H3": 0, "DCX_H3_1X1": 0, "DCX_H3_PAIRS": 0})):
    with contextlib.ExitStack() as st:
        for e in (eng, split):
            st.enter_context(e.knobs(**knobs))
        print(f"generate [{label}], {sha(eng.generate(z))}")
        print(f"encode [{label}], {sha(eng.encode(mel))}")
        print(f"split-K generate T=24 [{label}], {sha(split.generate(z24))}")
