"""The compile-time epilogue forms of the h3 convs (dcx_conv_common.h EpiForm / epilogue_form) against
the run-time epilogue they replace (DCX_EPI_GENERIC=1): the same operations in the same order, so
every output must be the same bits, and the h3 range flags must stay clear.

Two routes.  (1) The conv primitive, NativeConv.forward_h3 (dcx_conv_forward_h3: the fp32, h2, mean
accumulator, y_amax and shift outputs of a tap conv), at Cin = 128, Cout = 256 and 128, 3 taps at
dilation 5 and 11 taps, B = 3: every tap form, the in-place residual, the mean chain on one
accumulator, ragged lengths 0 / 1 / full, one combination outside the list, each output compared by
name.  (2) The modules and stage calls that produce each form, with the model's own shapes (the
one-tap forms need a ConvNeXt block's row ranges and are reached this way only):

  form        reached by                                            tiles
  EpiC1       ParallelBlock c1 convs (grouped, taps 3 / 7 / 11),    256 x 256 (C = 512, 256), 384 x 128 (C = 128)
              conv_pre in generate (single launch, 13 taps)
  EpiC2       ParallelBlock c2 convs (grouped; the second pair's    the same
              in place, y == res), ResBlock module (single)
  EpiMeanF/M  ParallelBlock's last convs, FIRST -> MID -> LAST on   the same
              one accumulator
  EpiMeanLH   ... LAST inside generate at C = 512, 256 (h2 out)     256 x 256
  EpiMeanLF   ... LAST inside generate at C = 128 (fp32 out)        384 x 128
  EpiUp       the ConvTs inside generate (2 and 3 taps per phase)   256 x 256, 384 x 128
  EpiPw1/Pw2  a ConvNeXt block's 1x1 convs (one tap, row ranges)    256 x 256
  (generic)   combinations outside the list run the run-time epilogue under either setting: the
              ResBlock module's last c2 (fp32 only), the ParallelBlock module's LAST (no measured max)

Row counts per clip: 1, 255, 257, 300, 385, i.e. a single row, a partial last tile, a second tile with
one row, a last batch whose rows are all past the end (300 = 256 + 44 at 16 rows per thread step; 385 =
384 + 1 on the 384-row tiles), B = 3 clips of different data.

What is compared.  A module or stage call lays out everything it produces in the caller's workspace, in
the same places for the same shapes: the ResBlock states (fp32), the h2 images, the mean accumulator,
the range arena with every conv's measured maximum (y_amax) and stored shift (y_ash), the ConvNeXt
blocks' row shifts.  Each run gets its own zeroed workspace and the two workspaces are compared byte
for byte, with the call's output.  (encode_decode's workspace also holds the VQ search's candidate
lists, whose order is not fixed: there the outputs alone are compared.)

Which epilogue ran.  The kernel names are the same for every form, so the tests read the launch
counters by form (NativeCodec.epi_form_launches): as shipped every form named by the test was
launched, under DCX_EPI_GENERIC=1 none was, and the combinations outside the list ran the run-time
epilogue under both.  The grouped launches are compared with the same convs launched one by one
(DCX_CONV_GROUP=0).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3
ROWS = (1, 255, 257, 300, 385)
FORMS = ("EpiC1", "EpiUp", "EpiC2", "EpiMeanF", "EpiMeanM", "EpiMeanLH", "EpiMeanLF", "EpiPw1", "EpiPw2", "generic")


@pytest.fixture(scope="module")
def eng(cfg, state):
    from distilcodec_nabeel_amd.engine import NativeCodec

    e = NativeCodec(cfg, state, "cuda:0", gemm="x6")
    assert e.get_knob("DCX_EPI_GENERIC") == 0 and e.get_knob("DCX_H3_SPLIT") == 1
    return e


def _x(seed, L, C):
    g = torch.Generator().manual_seed(seed)
    # clips of different scale: the per-clip ranges differ
    return (torch.randn(B, L, C, generator=g) * torch.tensor([0.25, 1.0, 3.0]).view(B, 1, 1)).to("cuda:0")


def _counted(eng, fn):
    """fn() and the launches it made, by form name."""
    eng.epi_form_launches(reset=True)
    out = fn()
    torch.cuda.synchronize()
    return out, dict(zip(FORMS, eng.epi_form_launches(reset=True)))


def _same(eng, run, ws_bytes, forms, generic=False, **knobs):
    """run(ws) as shipped and under the knobs, each on a zeroed workspace of ws_bytes (0: run() without
    one): outputs and workspaces bit-equal, no range flag; `forms` launched as shipped and no form under
    DCX_EPI_GENERIC=1; generic: the call also holds a combination outside the list."""
    def once():
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda:0") if ws_bytes else None
        out = run(ws) if ws_bytes else run()
        return (out if isinstance(out, tuple) else (out,)) + ((ws,) if ws_bytes else ())

    eng.range_flags(reset=True)
    a, na = _counted(eng, once)
    with eng.knobs(**knobs):
        b, nb = _counted(eng, once)
    assert eng.range_flags() == 0
    used = {f for f in FORMS[:-1] if na[f]}
    assert used == set(forms), (na, forms)
    assert (na["generic"] > 0) == generic, na
    if knobs.get("DCX_EPI_GENERIC"):
        assert not any(nb[f] for f in FORMS[:-1]) and nb["generic"] > 0, nb
        if "DCX_CONV_GROUP" not in knobs:  # launch for launch
            assert nb["generic"] == sum(na.values()), (na, nb)
    else:
        assert {f for f in FORMS[:-1] if nb[f]} == set(forms), nb
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.shape == v.shape
        assert torch.equal(u, v), f"{int((u != v).sum())} of {u.numel()} elements differ"
    for u in a[: len(a) - (1 if ws_bytes else 0)]:
        assert bool(torch.isfinite(u.float()).all())
    if ws_bytes:
        assert bool(a[-1].any())
    return a


def _module(eng, name, x, forms, generic, **knobs):
    need = eng.module_workspace_size(name, x.shape[0], x.shape[1])
    assert need > 0
    return _same(eng, lambda ws: eng.module(name, x, ws), need, forms, generic, **knobs)


def _kernels(eng, fn):
    eng.profile(True)
    eng.profile_reset()
    fn()
    torch.cuda.synchronize()
    names = {n for n, d in eng.profile_read().items() if d["launches"] > 0}
    eng.profile(False)
    return names


PBLOCK = ("EpiC1", "EpiC2", "EpiMeanF", "EpiMeanM")  # its MEAN_LAST has no measured maximum: outside the list


@pytest.mark.parametrize("L", ROWS)
@pytest.mark.parametrize("stage", [0, 1, 2])
def test_parallel_block(eng, cfg, stage, L):
    """EpiC1 and EpiC2 in grouped launches, the mean chain FIRST -> MID -> LAST on one accumulator."""
    C = cfg["decoder"]["upsample_initial_channel"] >> (stage + 1)
    _module(eng, f"generator.resblocks.{stage}", _x(100 * stage + L, L, C), PBLOCK, True, DCX_EPI_GENERIC=1)


@pytest.mark.parametrize("stage", [0, 2])
def test_grouped_launch_against_single_launches(eng, cfg, stage):
    """Three members with 3 / 7 / 11 taps in one grid (dealt longest first) against the same convs
    launched one by one, in their forms and in the run-time epilogue."""
    C = cfg["decoder"]["upsample_initial_channel"] >> (stage + 1)
    x = _x(7 + stage, 300, C)
    name = f"generator.resblocks.{stage}"
    grouped = "conv_gemm_x3dw_group<256,256,halo>" if C % 256 == 0 else "conv_gemm_x3dw_group<384,128,halo>"
    assert grouped in _kernels(eng, lambda: eng.module(name, x))
    with eng.knobs(DCX_CONV_GROUP=0):
        assert grouped not in _kernels(eng, lambda: eng.module(name, x))
    _module(eng, name, x, PBLOCK, True, DCX_CONV_GROUP=0)
    _module(eng, name, x, PBLOCK, True, DCX_CONV_GROUP=0, DCX_EPI_GENERIC=1)


@pytest.mark.parametrize("L", ROWS)
@pytest.mark.parametrize("stage,blk", [(1, 0), (2, 2)])
def test_resblock_single_launches(eng, cfg, stage, blk, L):
    """EpiC1 / EpiC2 launched singly (3 taps; 11 taps at dilation 5), the state updated in place
    (y == res), and the last c2, a combination outside the list (fp32 output only): it runs the
    run-time epilogue as shipped too."""
    C = cfg["decoder"]["upsample_initial_channel"] >> (stage + 1)
    _module(eng, f"generator.resblocks.{stage}.blocks.{blk}", _x(31 * stage + L, L, C), ("EpiC1", "EpiC2"), True,
            DCX_EPI_GENERIC=1)


GENERATOR = ("EpiC1", "EpiUp", "EpiC2", "EpiMeanF", "EpiMeanM", "EpiMeanLH", "EpiMeanLF")


@pytest.mark.parametrize("T", [1, 5, 33])
def test_generate(eng, cfg, T):
    """The whole generator: EpiUp, EpiMeanLH, EpiMeanLF and conv_pre's EpiC1 as well (stage rows 8 T,
    32 T, 64 T: 264 = 256 + 8 and 2112 = 5 * 384 + 192); no conv of it is outside the list."""
    z = _x(T, T, cfg["quantizer"]["input_dim"])
    _same(eng, lambda ws: eng.generate(z, ws), eng.workspace_size(B, T), GENERATOR, False, DCX_EPI_GENERIC=1)


def test_generate_ragged(eng, cfg):
    """The ragged instantiations, clips of 0, 1 and all frames."""
    T = 9
    z = _x(77, T, cfg["quantizer"]["input_dim"])
    w = _same(eng, lambda ws: eng.generate_ragged(z, [0, 1, T], ws), eng.workspace_size(B, T), GENERATOR, False,
              DCX_EPI_GENERIC=1)[0]
    assert not bool(w[0].any()) and not bool(w[1, 256:].any()) and bool(w[2].any())
    # the full-length clip is what it gives alone in a padded call
    assert torch.equal(w[2], eng.generate(z[2:3])[0])


@pytest.mark.parametrize("L", [1, 255, 257, 300, 385])
def test_convnext_block(eng, cfg, L):
    """EpiPw1 (GELU, h2 output with row ranges: the row shifts lie in the workspace) and EpiPw2 (gamma,
    residual in place) on the one-tap 256 x 256 tiles."""
    C = cfg["encoder"]["dims"][0]
    x = _x(L, L, C)
    assert "conv_gemm_x3dw<256,256>" in _kernels(eng, lambda: eng.module("encoder.stages.0.0", x))
    _module(eng, "encoder.stages.0.0", x, ("EpiPw1", "EpiPw2"), False, DCX_EPI_GENERIC=1)


def test_encode_decode(eng):
    """End to end (every form in place): codes and waveform."""
    from distilcodec_nabeel_amd import synth

    audio = torch.zeros(B, 12001)
    for i, c in enumerate(synth.clips(B, 12000, seed=11, kind="mix")):
        audio[i, 1:] = torch.from_numpy(np.asarray(c))
    audio = audio.to("cuda:0")
    _same(eng, lambda: eng.encode_decode(audio), 0, GENERATOR + ("EpiPw1", "EpiPw2"), True, DCX_EPI_GENERIC=1)


# ---- the conv primitive: Cin = 128, every tap form by name -------------------------------------------
import functools  # noqa: E402


@functools.lru_cache(maxsize=None)
def _conv(cout, k):
    from distilcodec_nabeel_amd.engine import NativeConv

    r = np.random.default_rng(cout + k)
    w = (r.standard_normal((cout, 128, k)) / np.sqrt(128 * k)).astype(np.float32)
    return NativeConv(w, (0.1 * r.standard_normal(cout)).astype(np.float32), dilation=5, h3=True)


def _all_forms(conv, x, res, lens=None):
    """Every tap form once, and one combination outside the list; {label: tensor}."""
    kw = dict(lens=lens)
    out = {}

    def put(tag, d):
        out.update({f"{tag}.{k}": v.clone() for k, v in d.items()})

    put("c1", conv.forward_h3(x, want_silu_h2=True, want_amax=True, **kw))                                # EpiC1
    put("up", conv.forward_h3(x, want_y=True, want_silu_h2=True, want_amax=True, **kw))                   # EpiUp
    put("c2", conv.forward_h3(x, want_y=True, want_silu_h2=True, want_amax=True, res=res.clone(), in_place=True, **kw))  # EpiC2, y == res
    macc = torch.zeros_like(res)
    put("mean_first", conv.forward_h3(x, res=res, macc=macc, mean=1, **kw))                                # EpiMeanF
    put("mean_mid", conv.forward_h3(x, res=res, macc=macc, mean=2, **kw))                                  # EpiMeanM
    put("mean_last_h2", conv.forward_h3(x, res=res, macc=macc, mean=3, want_silu_h2=True, want_amax=True, **kw))  # EpiMeanLH
    put("mean_last_f32", conv.forward_h3(x, res=res, macc=macc, mean=3, want_silu=True, want_amax=True, **kw))    # EpiMeanLF
    put("outside", conv.forward_h3(x, want_y=True, **kw))                                                  # fp32 only, no maximum
    return out


def _primitive(eng, conv, x, res, lens=None):
    a, na = _counted(eng, lambda: _all_forms(conv, x, res, lens))
    conv.set_knob("DCX_EPI_GENERIC", 1)
    try:
        b, nb = _counted(eng, lambda: _all_forms(conv, x, res, lens))
    finally:
        conv.set_knob("DCX_EPI_GENERIC", 0)
    assert na == dict(zip(FORMS, (1, 1, 1, 1, 1, 1, 1, 0, 0, 1))), na
    assert nb == dict(zip(FORMS, (0,) * 9 + (8,))), nb
    assert set(a) == set(b) and any(k.endswith("y_amax") for k in a) and any(k.endswith("y_ash") for k in a)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), f"{k}: {int((a[k] != b[k]).sum())} of {a[k].numel()} differ"
        if a[k].dtype == torch.float32:
            assert bool(torch.isfinite(a[k]).all()), k
    return a


@pytest.mark.parametrize("L", ROWS)
@pytest.mark.parametrize("k", [3, 11])
@pytest.mark.parametrize("cout", [256, 128])
def test_primitive_tap_forms(eng, cout, k, L):
    conv = _conv(cout, k)
    x = _x(cout + k + L, L, 128)
    res = _x(1 + cout + k + L, L, cout)
    a = _primitive(eng, conv, x, res)
    assert conv.last_kernel == ("conv_gemm_x3dw<256,256,halo>" if cout == 256 else "conv_gemm_x3dw<384,128,halo>")
    # the outputs hang together: the measured maximum is the fp32 output's, the chain is a mean
    assert torch.equal(a["up.y_amax"], a["up.y"].abs().amax(dim=(1, 2)))
    assert torch.equal(a["c2.y_amax"], a["c2.y"].abs().amax(dim=(1, 2)))
    assert torch.equal(a["mean_first.macc"], a["c2.y"])
    assert torch.equal(a["mean_mid.macc"], a["c2.y"] + a["c2.y"])
    assert bool(a["c1.y_silu_h2"].any()) and a["c1.y_ash"].abs().max() <= 64


@pytest.mark.parametrize("cout", [256, 128])
def test_primitive_ragged_forms(eng, cout):
    """The ragged instantiations: clips of 0, 1 and all of 300 rows."""
    conv = _conv(cout, 3)
    L = 300
    lens = torch.tensor([0, 1, L], dtype=torch.int32, device="cuda:0")
    live = (torch.arange(L, device="cuda:0").view(1, L, 1) < lens.view(B, 1, 1)).float()
    x = _x(cout, L, 128) * live
    res = _x(cout + 1, L, cout) * live
    a = _primitive(eng, conv, x, res, lens)
    for k in ("up.y", "c2.y", "mean_mid.macc", "mean_last_f32.y_silu"):
        assert not bool((a[k] * (1 - live)).any()), k
    assert not bool(a["c1.y_silu_h2"][0].any()) and not bool(a["c1.y_silu_h2"][1, 1:].any())
    assert float(a["up.y_amax"][0]) == 0.0 and float(a["up.y_amax"][2]) > 0.0
