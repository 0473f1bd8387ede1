"""The h3 weight layout (csrc/dcx_w3_layout.h) through the kernels that read it.

h2_pack writes the weights in the order of the kernels' LDS images (each 64-column block piece-major
for the conv kernels, each ring piece in lane order for the pair kernels), and every kernel takes its
source offsets from the same header.  The host side of that is tests/test_w3_layout_host.py; here the
kernels run:

  * NativeConv(..., h3=True) on shapes that reach every term of the index: one chunk with two
    64-column blocks (the 384 x 128 tile), the chunk stride, a second column tile (co0 = 256), the
    phase base with two taps, eight phases, and the one-tap convs; at lengths 1, 257 and 385.  Each
    case against the fp64 conv at the element-wise h3 bound of tests/test_gpu_conv.py (imported, not
    restated), and bit-equal under DCX_H3_BN = 128 / 256 and DCX_H3_SPLIT = 0 (other tiles and DMA
    issue orders over the same weights);
  * one ParallelBlock at C = 64 and at C = 32 on the pair kernel's smallest tile height, 2 clips:
    the per-wave weight loads (DCX_RP_RING=0) bit-equal to the LDS ring, and the output within the
    bound tests/test_gpu_h3.py holds the pair kernels to against the fp64 oracle (2e-4 of the maximum).
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_conv import _check_h3_elementwise, _conv64

pytestmark = pytest.mark.gpu

B = 2

# (cin, cout, k, dilation, transposed, stride)
SHAPES = [
    (32, 128, 3, 1, False, 1),    # one chunk, two 64-column blocks, the 384 x 128 tile
    (64, 256, 3, 2, False, 1),    # the chunk stride
    (64, 512, 11, 5, False, 1),   # a second column tile, co0 = 256
    (64, 128, 4, 1, True, 2),     # the phase base, two taps
    (64, 512, 16, 1, True, 8),    # eight phases, two taps
    (32, 256, 1, 1, False, 1),    # the one-tap convs
    (256, 512, 1, 1, False, 1),
]
LENGTHS = [1, 257, 385]


def _sid(shape):
    cin, cout, k, d, tr, s = shape
    return f"{cin}x{cout}k{k}" + (f"T{s}" if tr else f"d{d}")


@functools.lru_cache(maxsize=None)
def _weights(shape):
    cin, cout, k, d, tr, s = shape
    r = np.random.default_rng([7, cin, cout, k, d, int(tr), s])
    w = (r.standard_normal((cin, cout, k) if tr else (cout, cin, k)) / np.sqrt(cin * k)).astype(np.float32)
    b = (r.standard_normal(cout) * 0.1).astype(np.float32)
    return w, b


@functools.lru_cache(maxsize=None)
def _conv(shape):
    from distilcodec_nabeel_amd.engine import NativeConv

    cin, cout, k, d, tr, s = shape
    w, b = _weights(shape)
    return NativeConv(w, b, dilation=d, transposed=tr, stride=s, h3=True)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_conv_reads_the_packed_layout(shape, L):
    cin, cout, k, d, tr, s = shape
    w, b = _weights(shape)
    r = np.random.default_rng([cin, cout, k, L])
    x = torch.from_numpy(r.standard_normal((B, L, cin)).astype(np.float32))
    res = torch.from_numpy(r.standard_normal((B, L * (s if tr else 1), cout)).astype(np.float32))
    w64, b64 = torch.from_numpy(w).double(), torch.from_numpy(b).double()
    ref = _conv64(shape, x, w64, None) + b64 + res.double()
    mag = _conv64(shape, x.abs(), w64.abs(), None) + b64.abs() + res.double().abs()
    conv = _conv(shape)
    xd, rd = x.cuda(), res.cuda()
    y0 = conv(xd, gemm="x6", epi=3, res=rd)
    default = conv.last_kernel
    assert default.startswith("conv_gemm_x3d"), default
    ex = _check_h3_elementwise(y0, ref, mag, shape)
    print(f"\n{default} {_sid(shape)} L={L}: |err| / elementwise bound {ex:.3f}", end="")
    try:
        for knob, value in (("DCX_H3_BN", 128), ("DCX_H3_BN", 256), ("DCX_H3_SPLIT", 0)):
            conv.set_knob("DCX_H3_SPLIT", 1)
            conv.set_knob("DCX_H3_BN", 0)
            conv.set_knob(knob, value)
            y = conv(xd, gemm="x6", epi=3, res=rd)
            assert conv.last_kernel.startswith("conv_gemm_x3d"), conv.last_kernel
            assert torch.equal(y, y0), (knob, value, conv.last_kernel)
    finally:
        conv.set_knob("DCX_H3_SPLIT", 1)
        conv.set_knob("DCX_H3_BN", 0)


@pytest.fixture(scope="module")
def eng(cfg, state):
    from distilcodec_nabeel_amd.engine import NativeCodec

    return NativeCodec(cfg, state, "cuda:0", gemm="x6")


# (stage, smallest tile height of conv_res_pair_h3, rows: three tiles, the last ragged)
@pytest.mark.parametrize("stage,rows,L", [(3, 48, 130), (4, 112, 300)], ids=["C64", "C32"])
def test_pair_kernels_read_the_packed_layout(eng, state, cfg, stage, rows, L):
    from oracle import reference_cpu as R

    C = cfg["decoder"]["upsample_initial_channel"] >> (stage + 1)
    x = torch.from_numpy(np.random.default_rng(40 + stage).standard_normal((B, C, L)).astype(np.float32))
    ref = torch.nn.functional.silu(R.parallel_block(x.double(), state["generator"], stage, cfg["decoder"], torch.float64))
    xd = x.transpose(1, 2).contiguous().to("cuda:0")
    with eng.knobs(DCX_RP_R=rows):
        ring = eng.module(f"generator.resblocks.{stage}", xd)
    with eng.knobs(DCX_RP_R=rows, DCX_RP_RING=0):
        loads = eng.module(f"generator.resblocks.{stage}", xd)
    torch.cuda.synchronize()
    assert torch.equal(ring, loads)
    y = ring.cpu().double().transpose(1, 2)
    err = ((y - ref).abs().max() / ref.abs().max()).item()
    print(f"\nstage {stage} (C = {C}), {rows}-row tiles: rel err {err:.3g}", end="")
    assert err < 2e-4, err
