"""conv_gemm_x3dw's activation image (csrc/dcx_a3_layout.h) through the kernels that fill and read it.

x3dw_tile fetches an input chunk as 8 rows x 128 B per LDS-DMA instruction into a row-major image whose
pieces are XOR-permuted by the row, and recomputes its fragment base per tap offset; conv_gemm_x3dq /
x3dm (the DCX_H3_BN tilings) keep the piece-major image and are the same-bits reference.  The host side
is tests/test_a3_image_host.py; here the kernels run, NativeConv(..., h3=True), B = 2 different clips:

  * shapes that reach one chunk, the chunk parity with tap offsets that are no multiples of 8, a third
    chunk back in buffer 0 with a reach of 50 of the 64 halo rows, the 384 x 128 tile, a negative input
    step with two polyphase taps, and the one-tap form (one and three chunks);
  * lengths 1, 7, 9, 263 and 385: clips shorter than an 8-row block, tiles whose last block is partly
    or wholly out of range, and a second tile.

Each case against the fp64 conv at the element-wise h3 bound of tests/test_gpu_conv.py (imported, not
restated), bit-equal under DCX_H3_BN = 128 (conv_gemm_x3dq / x3dm), DCX_H3_BN = 256 and
DCX_H3_SPLIT = 0, and clip 1 of the pair bit-equal to clip 1 alone.  A two-tap conv has no x3dq form
(x3dq_bn keeps it on the 256 x 256 tiles under the knob): there the knob runs are still held to the
same bits, and the kernel-name assertion says so.  conv_gemm_x3dw's own unsplit 256 x 256 halo form
keeps the piece-major image (ROWS in x3dw_tile), so for the 256-column halo shapes the DCX_H3_SPLIT = 0
leg compares against that image; the unsplit row-image forms reached here are the 384 x 128 tile, the
one-tap form and, in the ragged test, the length-aware ones the generator launches.  One ragged generate
whose clips end on, just past and inside a tile, each bit-equal to the clip alone and to the unsplit run.
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
    (32, 256, 3, 1, False, 1),    # one chunk
    (64, 256, 7, 3, False, 1),    # chunk parity, offsets 0, 3, ... 18
    (96, 256, 11, 5, False, 1),   # the third chunk reuses buffer 0; reach 50 of the 64 halo rows
    (64, 128, 3, 5, False, 1),    # the 384 x 128 tile
    (64, 256, 4, 1, True, 2),     # negative in_step, two polyphase taps
    (32, 256, 1, 1, False, 1),    # one tap
    (96, 512, 1, 1, False, 1),
]
LENGTHS = [1, 7, 9, 263, 385]


def _sid(shape):
    cin, cout, k, d, tr, s = shape
    return f"{cin}x{cout}k{k}" + (f"T{s}" if tr else f"d{d}")


def _taps(shape):
    cin, cout, k, d, tr, s = shape
    return k // s if tr else k


def _default_kernel(shape):
    cout = shape[1]
    if _taps(shape) == 1:
        return "conv_gemm_x3dw<256,256>"
    return "conv_gemm_x3dw<256,256,halo>" if cout % 256 == 0 else "conv_gemm_x3dw<384,128,halo>"


@functools.lru_cache(maxsize=None)
def _weights(shape):
    cin, cout, k, d, tr, s = shape
    r = np.random.default_rng([11, cin, cout, k, d, int(tr), s])
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
def test_conv_through_the_image(shape, L):
    cin, cout, k, d, tr, s = shape
    w, b = _weights(shape)
    r = np.random.default_rng([cin, cout, k, L, 3])
    x = torch.from_numpy(r.standard_normal((B, L, cin)).astype(np.float32))
    x[1] *= 3.0  # the clips differ in scale too
    res = torch.from_numpy(r.standard_normal((B, L * (s if tr else 1), cout)).astype(np.float32))
    w64, b64 = torch.from_numpy(w).double(), torch.from_numpy(b).double()
    ref = _conv64(shape, x, w64, None) + b64 + res.double()
    mag = _conv64(shape, x.abs(), w64.abs(), None) + b64.abs() + res.double().abs()
    conv = _conv(shape)
    xd, rd = x.cuda(), res.cuda()
    y0 = conv(xd, gemm="x6", epi=3, res=rd)
    assert conv.last_kernel == _default_kernel(shape), conv.last_kernel
    ex = _check_h3_elementwise(y0, ref, mag, shape)
    print(f"\n{conv.last_kernel} {_sid(shape)} L={L}: |err| / elementwise bound {ex:.3f}", end="")
    # clip 1 of the pair is what clip 1 gives alone
    y1 = conv(xd[1:2].contiguous(), gemm="x6", epi=3, res=rd[1:2].contiguous())
    assert conv.last_kernel == _default_kernel(shape), conv.last_kernel
    assert torch.equal(y1, y0[1:2])
    try:
        for knob, value in (("DCX_H3_BN", 128), ("DCX_H3_BN", 256), ("DCX_H3_SPLIT", 0)):
            conv.set_knob("DCX_H3_SPLIT", 1)
            conv.set_knob("DCX_H3_BN", 0)
            conv.set_knob(knob, value)
            y = conv(xd, gemm="x6", epi=3, res=rd)
            kern = conv.last_kernel
            if knob == "DCX_H3_SPLIT" or _taps(shape) == 2 or (value == 256 and cout % 256):
                assert kern == _default_kernel(shape), (knob, value, kern)  # the same tiling, or no x3dq form
            else:  # the piece-major image of the old tilings
                assert kern.startswith("conv_gemm_x3dm<" if _taps(shape) == 1 else "conv_gemm_x3dq<"), (knob, value, kern)
            assert torch.equal(y, y0), (knob, value, kern)
    finally:
        conv.set_knob("DCX_H3_SPLIT", 1)
        conv.set_knob("DCX_H3_BN", 0)


def test_ragged_clips_straddling_a_tile(cfg, state):
    """Lengths 32, 33 and 20 frames at T_max = 33 (8 rows per frame at stage 0, 256-row tiles): clip 0
    ends on a tile boundary at every stage and its second tile is wholly dead, clip 1 has 8 live rows in
    its second tile, clip 2 ends inside its first.  The z rows beyond each length are NaN, so only the
    length-aware instantiations (the kernel names do not tell them from the padded ones) can leave a
    finite waveform and zeros beyond each length; each clip is what it gives alone."""
    from distilcodec_nabeel_amd.engine import NativeCodec

    eng = NativeCodec(cfg, state, "cuda:0", gemm="x6")
    lens = [32, 33, 20]
    z = torch.from_numpy(np.random.default_rng(17).standard_normal((3, 33, eng.D)).astype(np.float32))
    for b, n in enumerate(lens):
        z[b, n:] = float("nan")
    eng.profile(True)
    try:
        eng.profile_reset()
        wav = eng.generate_ragged(z, lens).clone()
        prof = eng.profile_read()
    finally:
        eng.profile(False)
        eng.profile_reset()
    ran = sorted(k for k, v in prof.items() if v["launches"] > 0)
    print(f"\nragged generate: {ran}", end="")
    assert any(k.startswith("conv_gemm_x3dw") for k in ran), ran
    assert torch.isfinite(wav).all()
    for b, n in enumerate(lens):
        assert wav[b, : eng.hop * n].abs().max() > 0 and not wav[b, eng.hop * n:].any(), b
        assert torch.equal(eng.generate_ragged(z[b:b + 1], lens[b:b + 1]), wav[b:b + 1]), b
    with eng.knobs(DCX_H3_SPLIT=0):  # the unsplit length-aware instantiations: the same bits
        assert torch.equal(eng.generate_ragged(z, lens), wav)
