"""The conv kernel family in isolation, kernel by kernel, against an fp64 CPU reference of F.conv1d /
F.conv_transpose1d.

KERNELS is a table of (shape, mode, expected kernel name, lengths): every case asserts the name
launch_conv reported for the call (NativeConv.last_kernel) as well as the numbers, so a dispatch
change that moves a shape to another kernel fails here instead of shrinking the coverage.  Every
name launch_conv and the h3 launchers can report for the primitive is the expected name of a row
(test_every_primitive_kernel_has_a_row keeps the list); the grouped launches are reachable through
modules only (tests/test_gpu_h3.py).  The lengths sit at 1, at one row either side of the kernel's
tile height, and (tap convs) below the tap span.

Modes: "x6" and "f32" (the primitive's defaults), "bf16" (one product, the reference's autocast),
"h3" (NativeConv(h3=True): the generator's wide convs and the ConvNeXt 1x1 convs), "h3/128" and
"h3/256" (the same with DCX_H3_BN, the other h3 tilings).

Every case runs B = 3 clips of different random data:
  * length sweep: epi = 3 (residual) with the SiLU output;
  * at one length per row also epi = 0 without a bias, epi = 0 with one, epi = 1 (erf GELU in fp64);
  * batch independence: clip b of the B = 3 run equals the B = 1 run of that clip bit for bit (the
    project's contract; a tile's halo reaching into a neighbouring clip shows here exactly);
  * h3 tap kernels: one mixed-scale case, the clips scaled by 2^-10, 1 and 2^10, each clip's error
    judged against its own maximum.

Bounds
  * x6, f32: max |y - y64| <= 1e-5 max |y64| (fp32 level).
  * bf16: tests/test_gpu_bf16.py::test_conv_bf16's rule against the fp64 conv of the bf16-rounded
    operands: bf16-valued outputs, every element within one bf16 ulp (2^-7 |ref| + 1e-6 max |ref|) of
    the rounded reference, fewer than 1 % of the elements different.  The 1 % is a rate, so it is
    taken over all the lengths of a row together (at L = 1 a row has a few hundred elements).
  * h3: the header's contract, max |y - y64| <= 2e-4 max |y64| (per clip in the mixed-scale case), and
    an a-priori bound per element, from the fp64 reference alone:
        |y - y64| <= (3 * 2^-22 + K * 2^-24) * (conv(|x|, |w|) + |b| + |res|) + 2^-23 |y64|
    Each operand keeps 22 significant bits (h + l, two fp16 values, after a power-of-two range scale:
    relative error 2^-22 each) and the l * l' product is dropped (2^-22 of |x| |w|): 3 * 2^-22 per
    product.  The products are exact in fp32 and accumulated in fp32 over K = taps * Cin terms
    (ConvTranspose: k / stride taps per phase), each addition rounding by at most 2^-24 of a partial
    sum no larger than conv(|x|, |w|): K * 2^-24, pessimistic.  The bias and residual additions and the
    final value round once each: 2^-23 |y64| with the slack of the K term.  (An operand more than
    2^17 below its clip's maximum loses low bits of l to fp16's subnormal spacing; its absolute error,
    2^-39 of the clip's maximum, is far below the other terms for the data used here.)

Measured on the MI355X: MEASURED below (pytest -s prints every case's figures).  The h3 kernels sit at
3e-7 .. 5e-7 of the maximum, where the x6 kernels do (2e-7 .. 2.5e-6) and below conv_gemm_f32 at
large K (3.3e-6), and use at most 2.3 % of the elementwise bound, whose K * 2^-24 term is a worst case.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# Largest max |y - y64| / max |y64| per kernel over its rows' length sweeps (epi = 3), from one MI355X
# run: (fp32 output, SiLU output); bf16 rows: the fraction of elements that differ from the rounded
# reference (bound 0.01).  A record, not a bound: the tests assert the bounds of the docstring.
MEASURED = {
    "conv_gemm_f32<128,128>": (3.29e-06, 3.46e-06),
    "conv_gemm_f32<256,64>": (7.83e-07, 7.76e-07),
    "conv_gemm_f32<256,32>": (1.14e-06, 1.16e-06),
    "conv_gemm_x6dm<256,256>": (9.85e-07, 8.32e-07),
    "conv_gemm_x6dm<256,256,halo>": (5.80e-07, 6.00e-07),
    "conv_gemm_x6dm<512,128,halo>": (1.67e-07, 2.00e-07),
    "conv_gemm_x6dq<256,256,halo>": (5.56e-07, 7.15e-07),
    "conv_gemm_x6dq<512,128,halo>": (3.03e-07, 3.44e-07),
    "conv_gemm_x6lm<256,128>": (1.44e-06, 1.57e-06),
    "conv_gemm_x6pp<256,128,halo>": (2.54e-06, 2.83e-06),
    "conv_gemm_x6pf<512,64,halo>": (8.01e-07, 9.25e-07),
    "conv_gemm_x6w4f<256,32,halo>": (3.53e-07, 3.68e-07),
    "conv_gemm_x6w4<256,64>": (3.83e-07, 4.13e-07),
    "conv_gemm_x6w4<256,64,halo>": (9.56e-07, 1.20e-06),
    "conv_gemm_x6w4<256,32>": (3.54e-07, 4.01e-07),
    "conv_gemm_x6w4<256,32,halo>": (1.16e-06, 1.25e-06),
    "conv_gemm_x3dw<256,256,halo>": (4.82e-07, 5.31e-07),   # |err| / elementwise bound <= 0.023
    "conv_gemm_x3dw<256,256>": (3.22e-07, 3.11e-07),        # 0.012
    "conv_gemm_x3dw<384,128,halo>": (4.79e-07, 5.14e-07),   # 0.022
    "conv_gemm_x3dq<128,256,halo>": (4.60e-07, 5.32e-07),   # 0.004
    "conv_gemm_x3dq<256,128,halo>": (4.60e-07, 5.02e-07),   # 0.004
    "conv_gemm_x3dm<128,256>": (3.22e-07, 3.19e-07),        # 0.012
    "conv_gemm_x3dm<256,128>": (2.98e-07, 3.53e-07),        # 0.010
    "conv_gemm_bf16w8<256,128,halo>": 0.00030,
    "conv_gemm_bf16w4<128,128>": 0.00003,
    "conv_gemm_bf16dm<256,256>": 0.00003,
    "conv_gemm_bf16w4f<256,64,halo>": 0.00012,
    "conv_gemm_bf16w4f<256,32,halo>": 0.00003,
    "conv_gemm_bf16w4<256,64>": 0.00008,
    "conv_gemm_bf16w4<256,32>": 0.00006,
    "conv_gemm_bf16w4<256,64,halo>": 0.00019,
    "conv_gemm_bf16w4<256,32,halo>": 0.00012,
}

B = 3

# (cin, cout, k, dilation, transposed, stride)
S_512_K3 = (512, 512, 3, 1, False, 1)
S_512_K11 = (512, 512, 11, 5, False, 1)
S_256_K7 = (256, 256, 7, 3, False, 1)
S_128_K11 = (128, 128, 11, 5, False, 1)
S_64_K11 = (64, 64, 11, 5, False, 1)
S_32_K7 = (32, 32, 7, 3, False, 1)
S_32_K3 = (32, 32, 3, 1, False, 1)
S_1024_K13 = (1024, 1024, 13, 1, False, 1)
S_128_256_K7 = (128, 256, 7, 1, False, 1)
S_1024_4096 = (1024, 4096, 1, 1, False, 1)
S_3584_1024 = (3584, 1024, 1, 1, False, 1)
T_1024_512 = (1024, 512, 16, 1, True, 8)
T_512_256 = (512, 256, 12, 1, True, 4)
T_256_128 = (256, 128, 4, 1, True, 2)
T_64_32 = (64, 32, 4, 1, True, 2)
T_1024_K1 = (1024, 1024, 1, 1, True, 1)
S_32_128_K1 = (32, 128, 1, 1, False, 1)
S_32_256_K3 = (32, 256, 3, 1, False, 1)
T_16_256 = (16, 256, 4, 1, True, 2)
S_64_512_K3D2 = (64, 512, 3, 2, False, 1)
S_128_K3 = (128, 128, 3, 1, False, 1)
# the smallest shapes that reach the other branches of launch_conv
S_32_4096_K11 = (32, 4096, 11, 5, False, 1)   # 16 column tiles of 256: the big tiles pay at any length
S_64_1024_K3 = (64, 1024, 3, 1, False, 1)
S_32_2176_K3 = (32, 2176, 3, 1, False, 1)     # 17 x 128 columns, no multiple of 256
T_64_512 = (64, 512, 16, 1, True, 8)
T_64_384 = (64, 384, 16, 1, True, 8)
S_64_4096_K1 = (64, 4096, 1, 1, False, 1)
S_256_64_K1 = (256, 64, 1, 1, False, 1)
S_256_96_K1 = (256, 96, 1, 1, False, 1)
S_256_64_K7 = (256, 64, 7, 3, False, 1)
S_256_96_K7 = (256, 96, 7, 3, False, 1)
S_64_512_K11 = (64, 512, 11, 5, False, 1)
S_64_128_K11 = (64, 128, 11, 5, False, 1)
T_64_128 = (64, 128, 4, 1, True, 2)
# one-tap h3 convs split their input per row (launch_h2_rows: Cin 256, 512, 768 or 1024)
S_256_512_K1 = (256, 512, 1, 1, False, 1)
S_256_384_K1 = (256, 384, 1, 1, False, 1)

X6DM = "conv_gemm_x6dm<256,256>"
X6DM_H = "conv_gemm_x6dm<256,256,halo>"
X6DM512_H = "conv_gemm_x6dm<512,128,halo>"
X6DQ_H = "conv_gemm_x6dq<256,256,halo>"
X6DQ512_H = "conv_gemm_x6dq<512,128,halo>"
X6LM = "conv_gemm_x6lm<256,128>"
X6PP_H = "conv_gemm_x6pp<256,128,halo>"
X6PF_H = "conv_gemm_x6pf<512,64,halo>"
X6W4F32_H = "conv_gemm_x6w4f<256,32,halo>"
F32_128 = "conv_gemm_f32<128,128>"
F32_64 = "conv_gemm_f32<256,64>"
F32_32 = "conv_gemm_f32<256,32>"

# (shape, mode, expected kernel, lengths).  The first 21 shapes with their first length are the cases
# this file has always had (both modes); the kernel column records what they reach: by the rule of
# big_tiles_pay (ceil(L / BM) * (Cout / BN) * phases >= 16 per clip) only two of them run an LDS-DMA
# big-tile kernel, the others with Cout % 128 == 0 the 256 x 128 ping-pong kernels.
KERNELS = [
    (S_512_K3, "x6", X6PP_H, (300,)),
    (S_512_K11, "x6", X6PP_H, (257, 1, 49, 255, 256)),
    (S_256_K7, "x6", X6PP_H, (1000,)),
    (S_128_K11, "x6", X6PP_H, (515,)),
    (S_64_K11, "x6", X6PF_H, (700, 1, 511, 512, 513)),          # fp32 input, split while staging
    (S_32_K7, "x6", X6W4F32_H, (1333,)),
    (S_32_K3, "x6", X6W4F32_H, (64,)),
    (S_1024_K13, "x6", X6PP_H, (97,)),
    (S_128_256_K7, "x6", X6PP_H, (93,)),
    (S_1024_4096, "x6", X6DM, (190,)),                          # 16 column tiles
    (S_3584_1024, "x6", X6LM, (77,)),
    (T_1024_512, "x6", X6DM_H, (50,)),                          # 2 column tiles x 8 phases
    (T_512_256, "x6", X6PP_H, (61,)),
    (T_256_128, "x6", X6PP_H, (129,)),
    (T_64_32, "x6", X6W4F32_H, (333,)),
    (T_1024_K1, "x6", X6LM, (45,)),
    # 2 and 6 K16 steps, fewer than the ping-pong kernels prefetch
    (S_32_128_K1, "x6", X6LM, (300, 1, 255, 256, 257)),
    (S_32_256_K3, "x6", X6PP_H, (200,)),
    # 2 steps (ConvT phases) and 12 steps with dilation: one and two row tiles of 256 x 128
    (T_16_256, "x6", X6PP_H, (100,)),
    (S_64_512_K3D2, "x6", X6PP_H, (260,)),
    # five row tiles of 256 x 128, the last ragged (three 512-row tiles would not pay: 3 < 16)
    (S_128_K3, "x6", X6PP_H, (1100,)),
    # the LDS-DMA big-tile kernels
    (S_32_4096_K11, "x6", X6DQ_H, (1, 255, 256, 257)),
    (S_64_1024_K3, "x6", X6DQ_H, (1000,)),                      # 4 row tiles, the last ragged
    (S_32_2176_K3, "x6", X6DQ512_H, (1, 511, 512, 513)),
    (T_64_512, "x6", X6DM_H, (1, 255, 256, 257)),
    (T_64_384, "x6", X6DM512_H, (1, 511, 513)),
    (S_64_4096_K1, "x6", X6DM, (1, 256, 257)),
    # planes-input small-Cout kernels (Cin > 128, or one tap)
    (S_256_64_K1, "x6", "conv_gemm_x6w4<256,64>", (1, 255, 257)),
    (S_256_96_K1, "x6", "conv_gemm_x6w4<256,32>", (1, 255, 257)),
    (S_256_64_K7, "x6", "conv_gemm_x6w4<256,64,halo>", (1, 255, 257)),
    (S_256_96_K7, "x6", "conv_gemm_x6w4<256,32,halo>", (1, 255, 257)),
    # conv_gemm_f32: the old cases, then its three tilings at their tile edges
    (S_512_K3, "f32", F32_128, (300,)),
    (S_512_K11, "f32", F32_128, (257, 1, 49, 127, 128, 129)),
    (S_256_K7, "f32", F32_128, (1000,)),
    (S_128_K11, "f32", F32_128, (515,)),
    (S_64_K11, "f32", F32_64, (700, 1, 255, 256, 257)),
    (S_32_K7, "f32", F32_32, (1333,)),
    (S_32_K3, "f32", F32_32, (64, 1, 255, 256, 257)),
    (S_1024_K13, "f32", F32_128, (97,)),
    (S_128_256_K7, "f32", F32_128, (93,)),
    (S_1024_4096, "f32", F32_128, (190,)),
    (S_3584_1024, "f32", F32_128, (77,)),
    (T_1024_512, "f32", F32_128, (50,)),
    (T_512_256, "f32", F32_128, (61,)),
    (T_256_128, "f32", F32_128, (129,)),
    (T_64_32, "f32", F32_32, (333,)),
    (T_1024_K1, "f32", F32_128, (45,)),
    (S_32_128_K1, "f32", F32_128, (300,)),
    (S_32_256_K3, "f32", F32_128, (200,)),
    (T_16_256, "f32", F32_128, (100,)),
    (S_64_512_K3D2, "f32", F32_128, (260,)),
    (S_128_K3, "f32", F32_128, (1100,)),
    (T_64_384, "f32", F32_128, (1, 127, 129)),
    (S_256_64_K1, "f32", F32_64, (1, 255, 257)),
    (S_256_96_K7, "f32", F32_32, (1, 255, 257)),
    # the one-product (bf16) names of the same dispatch
    (S_512_K11, "bf16", "conv_gemm_bf16w8<256,128,halo>", (1, 49, 255, 256, 257)),
    (S_32_128_K1, "bf16", "conv_gemm_bf16w4<128,128>", (1, 127, 128, 129)),
    (S_64_4096_K1, "bf16", "conv_gemm_bf16dm<256,256>", (1, 256, 257)),
    (S_64_K11, "bf16", "conv_gemm_bf16w4f<256,64,halo>", (1, 255, 256, 257)),
    (S_32_K7, "bf16", "conv_gemm_bf16w4f<256,32,halo>", (1, 255, 256, 257)),
    (S_256_64_K1, "bf16", "conv_gemm_bf16w4<256,64>", (1, 255, 257)),
    (S_256_96_K1, "bf16", "conv_gemm_bf16w4<256,32>", (1, 255, 257)),
    (S_256_64_K7, "bf16", "conv_gemm_bf16w4<256,64,halo>", (1, 255, 257)),
    (S_256_96_K7, "bf16", "conv_gemm_bf16w4<256,32,halo>", (1, 255, 257)),
    # h3 (k 11 with dilation 5 spans 50 rows: L = 49 is shorter than the span)
    (S_64_512_K11, "h3", "conv_gemm_x3dw<256,256,halo>", (1, 49, 255, 256, 257)),
    (T_64_512, "h3", "conv_gemm_x3dw<256,256,halo>", (1, 49, 255, 256, 257)),
    (S_256_512_K1, "h3", "conv_gemm_x3dw<256,256>", (1, 255, 257)),
    (S_64_128_K11, "h3", "conv_gemm_x3dw<384,128,halo>", (1, 383, 384, 385)),
    (T_64_128, "h3", "conv_gemm_x3dw<384,128,halo>", (1, 383, 384, 385)),
    (S_256_384_K1, "h3", "conv_gemm_x3dm<256,128>", (1, 255, 257)),
    (S_64_512_K11, "h3/256", "conv_gemm_x3dq<128,256,halo>", (1, 127, 129, 255, 257)),
    (S_64_512_K11, "h3/128", "conv_gemm_x3dq<256,128,halo>", (1, 255, 257)),
    (S_256_512_K1, "h3/256", "conv_gemm_x3dm<128,256>", (1, 127, 129, 255, 257)),
]

# every name launch_conv / launch_x3dw / launch_x3dq can report for a dcx_conv_forward call (fp32
# outputs only: the register-epilogue and persistent bf16 1x1 kernels need a compact bf16 output,
# the split-K and grouped launches a stage)
PRIMITIVE_KERNELS = {
    "conv_gemm_f32<128,128>", "conv_gemm_f32<256,64>", "conv_gemm_f32<256,32>",
    "conv_gemm_x6pf<512,64,halo>", "conv_gemm_x6w4f<256,32,halo>",
    "conv_gemm_x6dm<256,256>", "conv_gemm_x6dm<256,256,halo>", "conv_gemm_x6dm<512,128,halo>",
    "conv_gemm_x6dq<256,256,halo>", "conv_gemm_x6dq<512,128,halo>",
    "conv_gemm_x6lm<256,128>", "conv_gemm_x6pp<256,128,halo>",
    "conv_gemm_x6w4<256,64>", "conv_gemm_x6w4<256,64,halo>", "conv_gemm_x6w4<256,32>", "conv_gemm_x6w4<256,32,halo>",
    "conv_gemm_bf16w4f<256,64,halo>", "conv_gemm_bf16w4f<256,32,halo>", "conv_gemm_bf16dm<256,256>",
    "conv_gemm_bf16w4<128,128>", "conv_gemm_bf16w8<256,128,halo>",
    "conv_gemm_bf16w4<256,64>", "conv_gemm_bf16w4<256,64,halo>", "conv_gemm_bf16w4<256,32>", "conv_gemm_bf16w4<256,32,halo>",
    "conv_gemm_x3dw<256,256,halo>", "conv_gemm_x3dw<256,256>", "conv_gemm_x3dw<384,128,halo>",
    "conv_gemm_x3dq<128,256,halo>", "conv_gemm_x3dq<256,128,halo>", "conv_gemm_x3dm<128,256>", "conv_gemm_x3dm<256,128>",
}


# cin, cout, k, dil, transposed, stride, L: the cases of test_conv_matches_fp64 (the first length of the
# first 21 shapes of KERNELS in both modes)
CASES = [shape + (Ls[0],) for shape, mode, _, Ls in KERNELS[:21]]
_OLD = {(c[:6], g, c[6]) for c in CASES for g in ("x6", "f32")}


def _row_kernel(shape, mode, L):
    (kern,) = {k for sh, m, k, Ls in KERNELS if sh == shape and m == mode and L in Ls}
    return kern


def _sid(shape):
    cin, cout, k, d, tr, s = shape
    return f"{cin}x{cout}k{k}" + (f"T{s}" if tr else f"d{d}")


def _sweep(modes):
    return [pytest.param(shape, mode, kern, L, id=f"{kern}-{_sid(shape)}-{mode}-L{L}")
            for shape, mode, kern, Ls in KERNELS if mode.split("/")[0] in modes for L in Ls
            if (shape, mode, L) not in _OLD]


def _one_length(modes):
    """Per row one length that has a full tile and a ragged one where the row has such a length."""
    return [pytest.param(shape, mode, kern, max(Ls), id=f"{kern}-{_sid(shape)}-{mode}-L{max(Ls)}")
            for shape, mode, kern, Ls in KERNELS if mode.split("/")[0] in modes]


@functools.lru_cache(maxsize=None)
def _weights(shape):
    cin, cout, k, d, tr, s = shape
    r = np.random.default_rng([cin, cout, k, d, int(tr), s])
    w = (r.standard_normal((cin, cout, k) if tr else (cout, cin, k)) / np.sqrt(cin * k)).astype(np.float32)
    b = (r.standard_normal(cout) * 0.1).astype(np.float32)
    return w, b


@functools.lru_cache(maxsize=None)
def _conv_obj(shape, h3, bn, bias):
    from distilcodec_nabeel_amd.engine import NativeConv

    cin, cout, k, d, tr, s = shape
    w, b = _weights(shape)
    conv = NativeConv(w, b if bias else None, dilation=d, transposed=tr, stride=s, h3=h3)
    if bn:
        conv.set_knob("DCX_H3_BN", bn)
    return conv


def _conv(shape, mode, bias=True):
    """The row's conv object (x6, f32 and bf16 rows of a shape share one: the mode is per call)."""
    return _conv_obj(shape, mode.startswith("h3"), int(mode.split("/")[1]) if "/" in mode else 0, bias)


@functools.lru_cache(maxsize=64)
def _data(shape, L):
    """x [B][L][cin], res [B][Lout][cout] (fp32, shared and never modified)."""
    cin, cout, k, d, tr, s = shape
    r = np.random.default_rng([cin, cout, k, d, int(tr), s, L])
    x = torch.from_numpy(r.standard_normal((B, L, cin)).astype(np.float32))
    res = torch.from_numpy(r.standard_normal((B, L * (s if tr else 1), cout)).astype(np.float32))
    return x, res


def _conv64(shape, x, w, b):
    """fp64 conv of channels-last x [B][L][cin] -> [B][Lout][cout]."""
    cin, cout, k, d, tr, s = shape
    xt = x.double().transpose(1, 2)
    if tr:
        y = F.conv_transpose1d(xt, w, b, stride=s, padding=(k - s) // 2)
    else:
        y = F.conv1d(xt, w, b, dilation=d, padding=d * (k - 1) // 2)
    return y.transpose(1, 2)


@functools.lru_cache(maxsize=64)
def _ref(shape, L):
    """The conv of _data(shape, L) without its bias, in fp64."""
    return _conv64(shape, _data(shape, L)[0], torch.from_numpy(_weights(shape)[0]).double(), None)


@functools.lru_cache(maxsize=64)
def _mag(shape, L):
    """conv(|x|, |w|) in fp64: the magnitude the h3 elementwise bound scales with."""
    return _conv64(shape, _data(shape, L)[0].abs(), torch.from_numpy(_weights(shape)[0]).double().abs(), None)


def _k_terms(shape):
    cin, cout, k, d, tr, s = shape
    return (k // s if tr else k) * cin


def _maxrel(y, ref):
    return ((y.cpu().double() - ref).abs().max() / ref.abs().max()).item()


def _check_h3_elementwise(y, ref, mag, shape):
    """The a-priori h3 bound of the module docstring; mag = conv(|x|, |w|) + |b| + |res|."""
    bound = (3 * 2.0 ** -22 + _k_terms(shape) * 2.0 ** -24) * mag + 2.0 ** -23 * ref.abs()
    excess = ((y.cpu().double() - ref).abs() / bound).max().item()
    assert excess <= 1.0, f"elementwise h3 bound exceeded: |err| / bound = {excess:.3f}"
    return excess


def _gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / np.sqrt(2.0)))


def test_every_primitive_kernel_has_a_row():
    assert {kern for _, _, kern, _ in KERNELS} == PRIMITIVE_KERNELS == set(MEASURED)


def _check_sweep_case(shape, mode, kern, L):
    """Residual epilogue and the SiLU output at one length; the B = 3 run's clips equal their B = 1 runs."""
    w, b = _weights(shape)
    x, res = _data(shape, L)
    conv = _conv(shape, mode)
    gemm = "f32" if mode == "f32" else "x6"
    xd, rd = x.cuda(), res.cuda()
    y, ys = conv(xd, gemm=gemm, epi=3, res=rd, want_silu=True)
    assert conv.last_kernel == kern
    v = _ref(shape, L)
    b64 = torch.from_numpy(b).double()
    ref = v + b64 + res.double()
    sref = ref * torch.sigmoid(ref)
    err, serr = _maxrel(y, ref), _maxrel(ys, sref)
    print(f"\n{kern} {_sid(shape)} {mode} L={L}: err {err:.3g}, silu err {serr:.3g}", end="")
    tol = 2e-4 if mode.startswith("h3") else 1e-5
    assert err < tol, err
    assert serr < tol, serr
    if mode.startswith("h3"):
        ex = _check_h3_elementwise(y, ref, _mag(shape, L) + b64.abs() + res.double().abs(), shape)
        print(f", |err| / elementwise bound {ex:.3f}", end="")
    for c in range(B):
        y1, ys1 = conv(xd[c:c + 1].contiguous(), gemm=gemm, epi=3, res=rd[c:c + 1].contiguous(), want_silu=True)
        assert conv.last_kernel == kern
        assert torch.equal(y1[0], y[c]) and torch.equal(ys1[0], ys[c]), f"clip {c} alone differs from the batch"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("gemm", ["x6", "f32"])
def test_conv_matches_fp64(case, gemm):
    """The cases this file has always had, now with three clips and the kernel they reach (KERNELS)."""
    shape, L = case[:6], case[6]
    _check_sweep_case(shape, gemm, _row_kernel(shape, gemm, L), L)


@pytest.mark.parametrize("shape,mode,kern,L", _sweep(("x6", "f32", "h3")))
def test_conv_kernel_edges(shape, mode, kern, L):
    """The rest of the table: every kernel at its edge lengths."""
    _check_sweep_case(shape, mode, kern, L)


@pytest.mark.parametrize("shape,mode,kern,L", _one_length(("x6", "f32", "h3")))
def test_conv_epilogues(shape, mode, kern, L):
    """epi = 0 without and with a bias, epi = 1 (GELU against the fp64 erf form)."""
    w, b = _weights(shape)
    x, _ = _data(shape, L)
    gemm = "f32" if mode == "f32" else "x6"
    h3 = mode.startswith("h3")
    tol = 2e-4 if h3 else 1e-5
    v = _ref(shape, L)
    b64 = torch.from_numpy(b).double()
    xd = x.cuda()
    for bias, epi in ((False, 0), (True, 0), (True, 1)):
        conv = _conv(shape, mode, bias)
        y = conv(xd, gemm=gemm, epi=epi)
        assert conv.last_kernel == kern
        pre = v + b64 if bias else v
        ref = _gelu64(pre) if epi == 1 else pre
        err = _maxrel(y, ref)
        print(f"\n{kern} {_sid(shape)} {mode} L={L} bias={bias} epi={epi}: err {err:.3g}", end="")
        assert err < tol, (bias, epi, err)
        if h3 and epi == 0:
            _check_h3_elementwise(y, ref, _mag(shape, L) + b64.abs() if bias else _mag(shape, L), shape)
        y1 = conv(xd[B - 1:].contiguous(), gemm=gemm, epi=epi)
        assert torch.equal(y1[0], y[B - 1])


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


@pytest.mark.parametrize("shape,mode,kern,Ls", [pytest.param(*row, id=f"{row[2]}-{_sid(row[0])}")
                                               for row in KERNELS if row[1] == "bf16"])
def test_conv_bf16_kernels(shape, mode, kern, Ls):
    """The one-product kernels at the edge lengths, by test_gpu_bf16.py::test_conv_bf16's rule."""
    cin, cout, k, d, tr, s = shape
    w, b = _weights(shape)
    conv = _conv(shape, mode)
    w64, b64 = _bf(torch.from_numpy(w).double()), _bf(torch.from_numpy(b).double())
    differing = total = 0
    for L in Ls:
        x, _ = _data(shape, L)
        xd = x.cuda()
        yd = conv(xd, gemm="bf16")
        assert conv.last_kernel == kern
        y = yd.cpu().double()
        ref = _conv64(shape, _bf(x.double()), w64, b64)  # autocast casts the bias with the other operands
        assert torch.equal(y, _bf(y))  # outputs are bf16 values
        err = (y - _bf(ref.float()).double()).abs()
        assert bool((err <= 2.0 ** -7 * ref.abs() + 1e-6 * ref.abs().max()).all()), L
        differing += int((err > 0).sum())
        total += err.numel()
        for c in range(B):
            assert torch.equal(conv(xd[c:c + 1].contiguous(), gemm="bf16")[0], yd[c]), (L, c)
    print(f"\n{kern} {_sid(shape)}: differing {differing / total:.5f}", end="")
    assert differing / total < 0.01


H3_TAP_ROWS = [row for row in KERNELS if row[1].startswith("h3") and row[0][2] > 1]


@pytest.mark.parametrize("shape,mode,kern,Ls", [pytest.param(*row, id=f"{row[2]}-{_sid(row[0])}-{row[1].replace('/', '_')}")
                                               for row in H3_TAP_ROWS])
def test_h3_mixed_scale_clips(shape, mode, kern, Ls):
    """Clips scaled by 2^-10, 1 and 2^10 in one batch: each clip is split with its own range, so each
    clip's error stays within the contract of its own maximum, and a clip alone gives the same bits."""
    L = max(Ls)
    x, _ = _data(shape, L)
    scale = torch.tensor([2.0 ** -10, 1.0, 2.0 ** 10]).reshape(B, 1, 1)
    xs = (x * scale).contiguous()  # exact: powers of two
    v, mag = _ref(shape, L), _mag(shape, L)
    conv = _conv(shape, mode, False)
    xd = xs.cuda()
    y = conv(xd, gemm="x6", epi=0)
    assert conv.last_kernel == kern
    for c in range(B):
        ref, m = v[c] * scale[c].double(), mag[c] * scale[c].double()
        err = _maxrel(y[c], ref)
        print(f"\n{kern} {_sid(shape)} clip scale 2^{int(np.log2(scale[c].item()))}: err {err:.3g}", end="")
        assert err < 2e-4, (c, err)
        _check_h3_elementwise(y[c], ref, m, shape)
        assert torch.equal(conv(xd[c:c + 1].contiguous(), gemm="x6", epi=0)[0], y[c])


@pytest.mark.parametrize("shape", [S_64_512_K11, T_64_512, S_256_512_K1, S_64_128_K11], ids=_sid)
def test_h3_tilings_and_split_issue_same_bits(shape):
    """DCX_H3_BN's other tilings and DCX_H3_SPLIT = 0 (conv_gemm_x3dw's DMA issued by one wave group)
    sum every output in the same order as the default kernel: same bits, on the primitive."""
    from distilcodec_nabeel_amd.engine import NativeConv

    cin, cout, k, d, tr, s = shape
    w, b = _weights(shape)
    L = 257 if cout % 256 == 0 else 385
    x, res = _data(shape, L)
    xd, rd = x.cuda(), res.cuda()
    y0 = _conv(shape, "h3")(xd, gemm="x6", epi=3, res=rd)
    default = _conv(shape, "h3").last_kernel
    conv = NativeConv(w, b, dilation=d, transposed=tr, stride=s, h3=True)
    seen = {default}
    for knob, value in (("DCX_H3_SPLIT", 0), ("DCX_H3_BN", 128), ("DCX_H3_BN", 256)):
        conv.set_knob("DCX_H3_SPLIT", 1)
        conv.set_knob("DCX_H3_BN", 0)
        conv.set_knob(knob, value)
        if knob == "DCX_H3_BN" and k // s < 3 and k > 1:
            continue  # conv_gemm_x3dq's tap kernels need 3 taps; the dispatch refuses fewer
        y = conv(xd, gemm="x6", epi=3, res=rd)
        seen.add(conv.last_kernel)
        assert torch.equal(y, y0), (knob, value, conv.last_kernel)
    assert conv.last_kernel.startswith("conv_gemm_x3d")
    if cout % 256 == 0 and (k == 1 or k // s >= 3):
        assert len(seen) == 3, seen  # the default and both DCX_H3_BN kernels ran


def test_h3_switch_is_off_by_default_and_selective():
    """Without h3=True the primitive runs x6; with it, a conv the stages would not run in h3 (Cout 64)
    and the other GEMM modes keep their kernels."""
    x, _ = _data(S_64_512_K11, 257)
    conv = _conv(S_64_512_K11, "x6")
    conv(x.cuda(), gemm="x6")
    assert conv.last_kernel == X6PP_H
    h3 = _conv(S_64_512_K11, "h3")
    h3(x.cuda(), gemm="f32")
    assert h3.last_kernel == F32_128
    h3(x.cuda(), gemm="bf16")
    assert h3.last_kernel == "conv_gemm_bf16w8<256,128,halo>"
    x, _ = _data(S_256_64_K7, 257)
    narrow = _conv(S_256_64_K7, "h3")
    narrow(x.cuda(), gemm="x6")
    assert narrow.last_kernel == "conv_gemm_x6w4<256,64,halo>"
    with pytest.raises(Exception):
        narrow.set_knob("DCX_NOT_A_KNOB", 1)
