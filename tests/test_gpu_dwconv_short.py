"""The padded path's register-ring dwconv_ln (dwconv_ln_run_kernel, launches of B * L >= 8192 rows) on
clips shorter than its run, its 7-row window and its prefetch distance, through one ConvNeXt block
(`encoder.stages.<s>.0` of dcx_module_forward).  tests/test_gpu_modules.py runs that kernel only at
L = 937 and at run widths 4, 8 and 32; here L is 1, 3, 5, 7, 9 and 33, all four channel widths and all
four run widths appear, and every workgroup's four runs belong to different clips.

x is B copies of 16 distinct N(0, 1) clips in shuffled order.  Checks: DCX_DWCONV_TILED=1 (the tiled
kernel, 16-row tiles) gives the same bits and every copy of a clip gives the same bits (x6 and bf16);
in x6 each distinct clip is within 2e-4 (rel_per_clip, the module tolerance of DESIGN.md §4) of the
fp64 oracle's ConvNeXt block on the 16 distinct clips.  The row class is asserted from B * L before
anything is launched.  dcx_module_forward takes every one of these batch sizes; measured on the MI355X,
the worst clip against the oracle reads 2.2e-7 .. 4.9e-7 over the six cases.
"""
import numpy as np
import pytest
import torch
from _parity import rel_per_clip

pytestmark = pytest.mark.gpu

# (stage, B, L, run width): B * L is 8192, 8193, 16387, 32769, 65538 and 32770 rows, each at or just
# above the first row count of its run width (8192 * {1, 2, 4, 8})
CASES = [(0, 8192, 1, 4), (1, 2731, 3, 4), (2, 2341, 7, 8), (3, 3641, 9, 16), (0, 1986, 33, 32), (3, 6554, 5, 16)]
DISTINCT = 16


@pytest.fixture(scope="module")
def engines(cfg, state):
    from distilcodec_nabeel_amd.engine import NativeCodec

    sd = {"encoder": state["encoder"], "quantizer": state["quantizer"]}
    return {m: NativeCodec(cfg, sd, "cuda:0", with_generator=False, gemm=m) for m in ("x6", "bf16")}


def _run_width(rows):
    assert rows >= 8192  # the register ring, not the tiles
    return 32 if rows >= 65536 else 16 if rows >= 32768 else 8 if rows >= 16384 else 4


def _input(cfg, s, B, L):
    C = cfg["encoder"]["dims"][s]
    rng = np.random.default_rng(1000 * s + L)
    base = rng.standard_normal((DISTINCT, L, C)).astype(np.float32)  # channels-last
    which = rng.permutation(np.arange(B) % DISTINCT)
    assert len(set(which[:4].tolist())) > 1  # a workgroup's runs are not all one clip
    return base, which


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"s{c[0]}-B{c[1]}-L{c[2]}-rw{c[3]}")
def runs(request, engines, cfg):
    s, B, L, rw = request.param
    assert _run_width(B * L) == rw, (B, L)  # before anything is launched
    base, which = _input(cfg, s, B, L)
    x = torch.from_numpy(base).cuda()[torch.from_numpy(which).cuda()].contiguous()
    out = {"stage": s, "base": base, "which": torch.from_numpy(which).cuda()}
    name = f"encoder.stages.{s}.0"
    for mode, eng in engines.items():
        out[mode] = eng.module(name, x).clone()
        with eng.knobs(DCX_DWCONV_TILED=1):
            out[mode + "_tiled"] = eng.module(name, x).clone()
            torch.cuda.synchronize()
    out["flags"] = engines["x6"].range_flags(reset=True)
    yield out
    out.clear()


def _first_copy(y, which):
    """y's rows of the first copy of each distinct clip, [DISTINCT][L][C], and y against its copies."""
    first = torch.stack([(which == d).nonzero()[0, 0] for d in range(DISTINCT)])
    return y[first]


@pytest.mark.parametrize("mode", ["x6", "bf16"])
def test_tiled_knob_same_bits(runs, mode):
    assert bool(torch.isfinite(runs[mode]).all())
    assert torch.equal(runs[mode], runs[mode + "_tiled"])


@pytest.mark.parametrize("mode", ["x6", "bf16"])
def test_copies_agree(runs, mode):
    y, which = runs[mode], runs["which"]
    ref = _first_copy(y, which)[which]
    bad = (y != ref).flatten(1).any(1).nonzero().reshape(-1)
    assert bad.numel() == 0, ("copies differ at batch positions", bad[:8].tolist())


def test_x6_against_fp64_oracle(runs, state):
    from oracle import reference_cpu as R

    s = runs["stage"]
    x = torch.from_numpy(runs["base"]).double().transpose(1, 2)  # (16, C, L)
    with torch.no_grad():
        ref = R.convnext_block(x, state["encoder"], f"stages.{s}.0", torch.float64).transpose(1, 2)
    y = _first_copy(runs["x6"], runs["which"])
    rel = rel_per_clip(y, ref)
    print(f"\nstages.{s}.0 {tuple(runs['x6'].shape)}: x6 against the fp64 oracle, worst clip {rel.max():.3e}")
    assert rel.max() < 2e-4, rel
    assert runs["flags"] == 0
