"""The line-major lane map of the compile-time h3 epilogues (csrc/dcx_epi_lines.h: a thread owns 4
channels of a row and twice the rows; h2 units are written by lane pairs) against the run-time epilogue
(DCX_EPI_GENERIC=1, 8 channels per thread, untouched): every element goes through the same operations, so
every output must be the same bits.  tests/test_gpu_epi_forms.py holds the forms' own cases; here are
the ones the new map can get wrong and those tests do not reach:

  * row counts 1, 2, 127, 129, 255, 257: odd ends (a lane pair's row present or not), and both sides of
    the 128-row pass boundary of the 256 x 256 tiles (a thread's rows are now 8 apart, 16 on 384 x 128);
  * Cout = 512 (the second tile's column offset is 256), 256 and 128 (two rows per wave instruction);
  * ragged lengths with an odd clip and an empty one;
  * the residual form in place (y == res) and the mean chain FIRST -> MID -> LAST on one accumulator,
    where a lane may store only what it has loaded;
  * the ConvT forms inside generate, whose rows lie out_mul rows apart in memory (the model's ConvTs:
    out_mul 8 / 4 / 2 with 2 / 3 / 2 taps per phase; out_mul 3 does not occur and has no entry point,
    tests/host/epi_lines_check.cpp covers its offsets), at 127 and 129 frames, padded and ragged;
  * the one-tap forms with per-row input and output scales (a ConvNeXt block, C = 256 and 512); they and
    the ragged 256-column EpiC2 / last-of-mean forms keep 8 channels per thread (LINES in epilogue_form)
    and are held to the same bits.

Compared: the fp32 outputs, the h2 images, the mean accumulator, the y_amax words, the y_ash shifts (per
clip; per row they lie in the module's workspace, compared byte for byte) and the range flags.  The
launch counters show that the fixed forms ran as shipped and none under the knob.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3
ROWS = (1, 2, 127, 129, 255, 257)
FORMS = ("EpiC1", "EpiUp", "EpiC2", "EpiMeanF", "EpiMeanM", "EpiMeanLH", "EpiMeanLF", "EpiPw1", "EpiPw2", "generic")
GENERATOR = ("EpiC1", "EpiUp", "EpiC2", "EpiMeanF", "EpiMeanM", "EpiMeanLH", "EpiMeanLF")


@pytest.fixture(scope="module")
def eng(cfg, state):
    from distilcodec_nabeel_amd.engine import NativeCodec

    e = NativeCodec(cfg, state, "cuda:0", gemm="x6")
    assert e.get_knob("DCX_EPI_GENERIC") == 0 and e.get_knob("DCX_H3_SPLIT") == 1
    return e


def _x(seed, L, C):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, L, C, generator=g) * torch.tensor([0.25, 1.0, 3.0]).view(B, 1, 1)).to("cuda:0")


def _counted(eng, fn):
    eng.epi_form_launches(reset=True)
    out = fn()
    torch.cuda.synchronize()
    return out, dict(zip(FORMS, eng.epi_form_launches(reset=True)))


@functools.lru_cache(maxsize=None)
def _conv(cout):
    from distilcodec_nabeel_amd.engine import NativeConv

    r = np.random.default_rng(cout)
    w = (r.standard_normal((cout, 128, 3)) / np.sqrt(128 * 3)).astype(np.float32)
    return NativeConv(w, (0.1 * r.standard_normal(cout)).astype(np.float32), dilation=5, h3=True)


def _tap_forms(conv, x, res, lens):
    """Every tap form once: {label: tensor}."""
    kw = dict(lens=lens)
    out = {}

    def put(tag, d):
        out.update({f"{tag}.{k}": v.clone() for k, v in d.items()})

    put("c1", conv.forward_h3(x, want_silu_h2=True, want_amax=True, **kw))
    put("up", conv.forward_h3(x, want_y=True, want_silu_h2=True, want_amax=True, **kw))
    put("c2", conv.forward_h3(x, want_y=True, want_silu_h2=True, want_amax=True, res=res.clone(), in_place=True, **kw))  # y == res
    macc = torch.zeros_like(res)  # the chain in place on one accumulator
    put("mean_first", conv.forward_h3(x, res=res, macc=macc, mean=1, **kw))
    put("mean_mid", conv.forward_h3(x, res=res, macc=macc, mean=2, **kw))
    put("mean_last_h2", conv.forward_h3(x, res=res, macc=macc, mean=3, want_silu_h2=True, want_amax=True, **kw))
    put("mean_last_f32", conv.forward_h3(x, res=res, macc=macc, mean=3, want_silu=True, want_amax=True, **kw))
    return out


def _primitive(eng, conv, x, res, lens=None):
    eng.range_flags(reset=True)
    a, na = _counted(eng, lambda: _tap_forms(conv, x, res, lens))
    conv.set_knob("DCX_EPI_GENERIC", 1)
    try:
        b, nb = _counted(eng, lambda: _tap_forms(conv, x, res, lens))
    finally:
        conv.set_knob("DCX_EPI_GENERIC", 0)
    assert eng.range_flags() == 0
    assert na == dict(zip(FORMS, (1, 1, 1, 1, 1, 1, 1, 0, 0, 0))), na
    assert nb == dict(zip(FORMS, (0,) * 9 + (7,))), nb
    assert set(a) == set(b)
    for kind in ("y", "y_silu", "y_silu_h2", "macc", "y_amax", "y_ash"):
        assert any(k.endswith("." + kind) for k in a), kind
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), f"{k}: {int((a[k] != b[k]).sum())} of {a[k].numel()} differ"
    return a


@pytest.mark.parametrize("L", ROWS)
@pytest.mark.parametrize("cout", [512, 256, 128])
def test_tap_forms(eng, cout, L):
    conv = _conv(cout)
    a = _primitive(eng, conv, _x(cout + L, L, 128), _x(1 + cout + L, L, cout))
    assert conv.last_kernel == ("conv_gemm_x3dw<384,128,halo>" if cout == 128 else "conv_gemm_x3dw<256,256,halo>")
    assert torch.equal(a["c2.y_amax"], a["c2.y"].abs().amax(dim=(1, 2)))
    assert torch.equal(a["mean_first.macc"], a["c2.y"]) and torch.equal(a["mean_mid.macc"], a["c2.y"] + a["c2.y"])
    assert bool(a["c1.y_silu_h2"].any()) and bool(torch.isfinite(a["mean_last_f32.y_silu"]).all())


@pytest.mark.parametrize("cout", [512, 256, 128])
def test_tap_forms_ragged(eng, cout):
    """Clips of 0, 129 (odd, one row into the second pass) and all of 257 rows."""
    L = 257
    lens = torch.tensor([0, 129, L], dtype=torch.int32, device="cuda:0")
    live = (torch.arange(L, device="cuda:0").view(1, L, 1) < lens.view(B, 1, 1)).float()
    a = _primitive(eng, _conv(cout), _x(cout, L, 128) * live, _x(cout + 1, L, cout) * live, lens)
    for k in ("up.y", "c2.y", "mean_mid.macc", "mean_last_f32.y_silu"):
        assert not bool((a[k] * (1 - live)).any()), k
    assert not bool(a["c1.y_silu_h2"][0].any()) and not bool(a["c1.y_silu_h2"][1, 129:].any())
    assert bool(a["c1.y_silu_h2"][1, 128].any()) and float(a["up.y_amax"][0]) == 0.0


def _same(eng, run, ws_bytes, forms):
    """run(ws) as shipped and under DCX_EPI_GENERIC=1, each on a zeroed workspace: outputs and workspaces
    bit-equal, no range flag, `forms` and nothing else launched as shipped, no form under the knob."""
    def once():
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda:0")
        out = run(ws)
        return (out if isinstance(out, tuple) else (out,)) + (ws,)

    eng.range_flags(reset=True)
    a, na = _counted(eng, once)
    with eng.knobs(DCX_EPI_GENERIC=1):
        b, nb = _counted(eng, once)
    assert eng.range_flags() == 0
    assert {f for f in FORMS[:-1] if na[f]} == set(forms) and na["generic"] == 0, na
    assert not any(nb[f] for f in FORMS[:-1]) and nb["generic"] == sum(na.values()), nb
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.shape == v.shape
        assert torch.equal(u, v), f"{int((u != v).sum())} of {u.numel()} elements differ"
    assert bool(a[-1].any()) and bool(torch.isfinite(a[0].float()).all())
    return a


@pytest.mark.parametrize("T", [2, 127, 129])
def test_convt_forms_in_generate(eng, cfg, T):
    """EpiUp at out_mul 8 / 4 / 2 (rows 8 T, 32 T, 64 T after them), with every tap form around it."""
    z = _x(T, T, cfg["quantizer"]["input_dim"])
    _same(eng, lambda ws: eng.generate(z, ws), eng.workspace_size(B, T), GENERATOR)


def test_convt_forms_ragged(eng, cfg):
    """The ragged instantiations: clips of 0, 127 (odd) and all of 129 frames."""
    T = 129
    z = _x(78, T, cfg["quantizer"]["input_dim"])
    w = _same(eng, lambda ws: eng.generate_ragged(z, [0, 127, T], ws), eng.workspace_size(B, T), GENERATOR)[0]
    hop = cfg["decoder"]["hop_length"]
    assert w.shape[1] == T * hop and not bool(w[0].any()) and not bool(w[1, 127 * hop:].any()) and bool(w[1, 126 * hop:127 * hop].any())


@pytest.mark.parametrize("L", ROWS)
@pytest.mark.parametrize("block", ["encoder.stages.0.0", "encoder.stages.1.0"])
def test_one_tap_forms(eng, cfg, block, L):
    """EpiPw1 (GELU, an h2 output scaled per row: the row shifts lie in the workspace) and EpiPw2 (gamma and
    the residual in place, its input scaled per row), C = 256 and 512."""
    C = cfg["encoder"]["dims"][int(block.split(".")[2])]
    x = _x(L + C, L, C)
    need = eng.module_workspace_size(block, B, L)
    assert need > 0
    _same(eng, lambda ws: eng.module(block, x, ws), need, ("EpiPw1", "EpiPw2"))
