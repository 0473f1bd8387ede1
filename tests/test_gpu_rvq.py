"""Residual VQ (n_codebooks > 1) on the native path.

The chain's definition is exact (tests/_rvq_ref.py, pinned to the reference by tests/test_rvq_host.py):
every layer's code is the fp64 argmin of the fp32 residual and quantized_fup the fp32 sum in layer
order, so the x6 and bf16 modes are compared with no tolerance on the engine's own x_pjt_in.  Tolerances
against the reference fixture are those of tests/test_gpu_modules.py (2e-4 per row) and
tests/test_gpu_bf16.py::test_conv_bf16 (2^-7 |ref| + 1e-6 max|ref|)."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
import torch

import _rvq_ref as RV
from _parity import rel_per_row

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rvq.npz")
# (codebook_size, codebook_dim, n_codebooks, batch, frames): vq_prefilter_b1 with a partial second
# 256-row panel; the planes prefilter (2048 codes: below vq_prefilter_b1's 4096-code panels); the
# published row width.  The planes case has codebook_dim 256, not 128: the fp64 rescore the search ends
# in reads rows as 256-float vectors (dim % 256 == 0, with one codebook as well), so 128 cannot be searched.
SHAPES = {"b1": (4096, 256, 3, 2, 131), "planes": (2048, 256, 2, 1, 300), "wide": (4096, 3584, 2, 2, 70)}


def _state(cfg, state, with_generator=False):
    from distilcodec_nabeel_amd import weights

    s = {"encoder": state["encoder"], "quantizer": weights.synthetic_quantizer(cfg, seed=RV.FIXTURE_SEED)}
    if with_generator:
        s["generator"] = state["generator"]
    return s


def _engine(cfg, state, gemm="x6", with_generator=False):
    from distilcodec_nabeel_amd.engine import NativeCodec

    return NativeCodec(cfg, _state(cfg, state, with_generator), "cuda:0", with_generator=with_generator, gemm=gemm)


@pytest.fixture(scope="module")
def engines(state):
    """Quantizer-only engines by (shape name, gemm mode), built on first use and kept for the module."""
    cache = {}

    def get(name, gemm):
        if (name, gemm) not in cache:
            NC, CD, R = SHAPES[name][:3]
            cfg = RV.rvq_cfg(NC, CD, R)
            cache[(name, gemm)] = (_engine(cfg, state, gemm), cfg)
        return cache[(name, gemm)]

    yield get
    cache.clear()


@pytest.fixture(scope="module")
def gen2(state):
    """An R = 2 engine with the generator (x6), for the tests that need a waveform."""
    cfg = RV.rvq_cfg(4096, 256, 2)
    return _engine(cfg, state, "x6", with_generator=True), cfg


def _profiled(eng, fn):
    eng.profile(True)
    try:
        eng.profile_reset()
        y = fn()
        prof = eng.profile_read()
    finally:
        eng.profile(False)
        eng.profile_reset()
    return y, {k: int(v["launches"]) for k, v in prof.items() if v["launches"] > 0}


def _feat(B, T, seed):
    return torch.randn(B, T, 1024, generator=torch.Generator().manual_seed(seed)) * 0.5


def _Es(eng, cfg):
    R = cfg["quantizer"]["n_codebooks"]
    return RV.codebooks(_state(cfg, {"encoder": None})["quantizer"], R, "cuda:0")


@pytest.mark.parametrize("gemm", ["x6", "bf16"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_chain_exact(engines, name, gemm):
    eng, cfg = engines(name, gemm)
    NC, CD, R, B, T = SHAPES[name]
    assert eng.R == R
    (codes, pin, fup, q), names = _profiled(eng, lambda: eng.vq_encode(_feat(B, T, 3)))
    assert codes.shape == (B, T, R) and codes.dtype == torch.int32 and q.shape == (B, T, 1024)
    ref_codes, ref_fup, _ = RV.chain(pin.reshape(-1, CD), _Es(eng, cfg))
    assert torch.equal(codes.reshape(-1, R).long(), ref_codes)
    assert torch.equal(fup.reshape(-1, CD).view(torch.int32), ref_fup.view(torch.int32))
    if gemm == "bf16":  # layer 0 searches the bf16-valued x_pjt_in
        assert torch.equal(pin, pin.bfloat16().float())
    print(f"\n{name} {gemm}: {sorted(names)}", end="")
    assert names["vq_residual_step"] == R and names["gather_sum_rows"] == 1 and "gather_rows" not in names
    assert names["vq_certify"] == R and "row_sqnorm" in names and names["row_sqnorm"] == 1
    if name == "planes":  # layer 0 of the bf16 mode drops the zero planes of x, the residual layers cannot
        want = {"vq_prefilter_x3<256,128>": R} if gemm == "x6" else {"vq_prefilter_x2<256,128>": 1, "vq_prefilter_x3<256,128>": R - 1}
    else:
        want = {"vq_prefilter_b1<256,256>": R}
    assert {k: v for k, v in names.items() if k.startswith("vq_prefilter")} == want


def test_chain_f32_decisive(engines):
    eng, cfg = engines("b1", "f32")
    NC, CD, R, B, T = SHAPES["b1"]
    codes, pin, fup, _ = eng.vq_encode(_feat(B, T, 3))
    ref_codes, _, dec = RV.chain(pin.reshape(-1, CD), _Es(eng, cfg))
    share = float(dec.float().mean())
    print(f"\nf32: decisive share {share:.4f}", end="")
    assert share >= 0.9
    assert torch.equal(codes.reshape(-1, R).long()[dec], ref_codes[dec])
    got = RV.gather_sum(codes.long(), _Es(eng, cfg))  # fup is the fp32 sum of the codes it returned
    assert torch.equal(fup.view(torch.int32), got.view(torch.int32))


def test_tie_rule_in_layer_one(state):
    """Layer 1 holds copies of the rows layer 1 chose, one in the same tile and one in another: the
    lowest index wins, as test_gpu_vq.py::test_search_duplicate_codes_lowest_index checks for layer 0."""
    from distilcodec_nabeel_amd.engine import NativeCodec

    cfg = RV.rvq_cfg(8192, 256, 2)
    st = _state(cfg, state)
    feat = _feat(1, 64, 11)
    base = NativeCodec(cfg, st, "cuda:0", with_generator=False, gemm="x6")
    c0 = base.vq_encode(feat, want_fup=False, want_quantized=False)[0][0].cpu().numpy()
    del base
    key = "grvq.rvqs.0.layers.1._codebook.embed"
    E1 = st["quantizer"][key].copy()
    NC = E1.shape[1]
    chosen = sorted(set(c0[:, 1].tolist()))[:8]
    expect = {}
    for c in chosen:
        same_tile, other_tile = c ^ 1, (c + 4096 + 64) % NC
        if same_tile in chosen or other_tile in chosen:
            continue
        E1[0, same_tile] = E1[0, c]
        E1[0, other_tile] = E1[0, c]
        expect[c] = min(c, same_tile, other_tile)
    assert expect
    st["quantizer"] = dict(st["quantizer"], **{key: E1})
    eng = NativeCodec(cfg, st, "cuda:0", with_generator=False, gemm="x6")
    codes, pin, _, _ = eng.vq_encode(feat, want_fup=False, want_quantized=False)
    Es = RV.codebooks(st["quantizer"], 2, "cuda:0")
    ref_codes, _, _ = RV.chain(pin.reshape(-1, 256), Es)
    assert torch.equal(codes.reshape(-1, 2).long(), ref_codes)
    c1 = codes[0].cpu().numpy()
    assert np.array_equal(c1[:, 0], c0[:, 0])
    hit = [i for i in range(64) if int(c0[i, 1]) in expect]
    assert hit
    for i in hit:
        assert c1[i, 1] == expect[int(c0[i, 1])]


def test_against_reference_fixture(engines, state):
    from distilcodec_nabeel_amd.codec import DistilCodec

    fx = dict(np.load(GOLDEN))
    eng, cfg = engines("b1", "x6")
    feat = RV.fixture_feat()
    sd_q = _state(cfg, {"encoder": None})["quantizer"]
    dec = RV.forward(feat, sd_q, 3)["decisive"].numpy()
    assert dec.mean() >= 0.9
    codes, pin, fup, q = eng.vq_encode(feat.transpose(1, 2).contiguous())
    assert np.array_equal(codes.cpu().numpy()[dec], fx["codes"][dec])
    assert rel_per_row(pin, fx["x_pjt_in"], channel_axis=2).max() < 2e-4
    if np.array_equal(codes.cpu().numpy(), fx["codes"]):
        assert rel_per_row(q.transpose(1, 2), fx["quantized"]).max() < 2e-4
    else:  # a non-decisive flip: hold the decode of the reference's codes to the bound instead
        z = eng.vq_decode(torch.from_numpy(fx["codes"]))
        assert rel_per_row(z.transpose(1, 2), fx["quantized"]).max() < 2e-4
    z = eng.vq_decode(torch.from_numpy(fx["masked_codes"]))
    assert rel_per_row(z.transpose(1, 2), fx["z_masked"]).max() < 2e-4
    # the drop-in surface: Quantizer.encode (B, R, T), Quantizer.decode of (1, B, T, R)
    codec = DistilCodec(cfg, only_quantizer=True)
    codec.load_state_dict(_state(cfg, state))
    idx = codec.quantizer.encode(feat)
    assert tuple(idx.shape) == fx["encode"].shape and idx.dtype == torch.int64
    assert np.array_equal(idx.cpu().numpy().transpose(0, 2, 1)[dec], fx["codes"][dec])
    ret = codec.quantizer(feat)
    assert tuple(ret.codes.shape) == (1,) + fx["codes"].shape and tuple(ret.quantized.shape) == fx["quantized"].shape
    zq = codec.quantizer.decode(torch.from_numpy(fx["masked_codes"]).long()[None])
    assert tuple(zq.shape) == fx["z_masked"].shape
    assert rel_per_row(zq, fx["z_masked"]).max() < 2e-4
    with pytest.raises(ValueError):
        codec.quantizer.decode(torch.zeros(1, 2, 45, 1, dtype=torch.int64))
    bad = fx["masked_codes"].copy()
    bad[1, 7, 2] = 4096
    with pytest.raises(IndexError):
        codec.quantizer.decode(torch.from_numpy(bad).long()[None])


@pytest.mark.parametrize("name", ["b1", "wide"])
def test_project_out_hook_x6(engines, name):
    eng, cfg = engines(name, "x6")
    CD = SHAPES[name][1]
    sd_q = _state(cfg, {"encoder": None})["quantizer"]
    W = torch.from_numpy(sd_q["grvq.rvqs.0.project_out.weight"]).double().cuda()
    b = torch.from_numpy(sd_q["grvq.rvqs.0.project_out.bias"]).double().cuda()
    assert eng.module_io("quantizer.grvq.rvqs.0.project_out") == (CD, 1024, 1)
    x0 = torch.randn(2, 37, CD, generator=torch.Generator().manual_seed(2)).cuda()
    eng.range_flags(reset=True)
    for scale in (2.0 ** -12, 1.0, 2.0 ** 12):
        x = x0 * scale
        y = eng.module("quantizer.grvq.rvqs.0.project_out", x)
        ref = x.double() @ W.T + b
        assert rel_per_row(y, ref, channel_axis=2).max() < 2e-4, scale
    assert eng.range_flags() == 0


def test_project_out_hook_bf16(engines):
    eng, cfg = engines("b1", "bf16")
    sd_q = _state(cfg, {"encoder": None})["quantizer"]
    bf = lambda t: t.float().bfloat16().double()  # noqa: E731
    W = bf(torch.from_numpy(sd_q["grvq.rvqs.0.project_out.weight"])).cuda()
    b = bf(torch.from_numpy(sd_q["grvq.rvqs.0.project_out.bias"])).cuda()
    x = torch.randn(2, 300, 256, generator=torch.Generator().manual_seed(4)).cuda()
    y = eng.module("quantizer.grvq.rvqs.0.project_out", x).double()
    ref = bf(x) @ W.T + b
    assert torch.equal(y, bf(y))
    err = (y - bf(ref)).abs()
    assert bool((err <= 2.0 ** -7 * ref.abs() + 1e-6 * ref.abs().max()).all())


def _audio(B, n, seed):
    from distilcodec_nabeel_amd import synth

    clips = synth.clips(B, n, seed=seed, kind="mix")
    return torch.from_numpy(np.stack([np.concatenate([[0.0], c]) for c in clips]).astype(np.float32)).cuda()


def test_same_bits_across_plans(gen2):
    eng, cfg = gen2
    x = _audio(3, 24000 + 77, 5)
    with eng.knobs(DCX_ENC_STREAMS=2):
        (codes, wav), names = _profiled(eng, lambda: eng.encode_decode(x))
    assert codes.shape == (3, eng.num_frames(x.shape[1]), 2)
    assert names["vq_residual_step"] >= 2 and "gather_sum_rows" in names
    # staged: mel -> encode -> vq_encode -> vq_decode -> generate
    c2, _, _, q = eng.vq_encode(eng.encode(eng.mel(x)))
    z = eng.vq_decode(c2)
    assert torch.equal(c2, codes) and torch.equal(z, q) and torch.equal(eng.generate(z), wav)
    with eng.knobs(DCX_ENC_STREAMS=0):
        c0, w0 = eng.encode_decode(x)
    assert torch.equal(c0, codes) and torch.equal(w0, wav)
    for b in range(3):  # a clip alone equals its row in the batch
        cb, wb = eng.encode_decode(x[b:b + 1])
        assert torch.equal(cb[0], codes[b]) and torch.equal(wb[0], wav[b])


def test_ragged_calls(gen2):
    from distilcodec_nabeel_amd import synth
    from distilcodec_nabeel_amd.codec import DistilCodec

    eng, cfg = gen2
    frames = (1, 7, 65)
    clips = [synth.clips(1, 256 * t + 200, seed=20 + t, kind="mix")[0].astype(np.float32) for t in frames]
    codes, offsets, pin, fup = eng.tokenize_ragged(clips, want_pjt_in=True, want_fup=True)
    off = offsets.tolist()
    assert codes.shape == (sum(frames), 2) and [off[i + 1] - off[i] for i in range(3)] == list(frames)
    for b, c in enumerate(clips):
        ca, _, pa, fa = eng.tokenize_ragged([c], want_pjt_in=True, want_fup=True)
        assert torch.equal(ca, codes[off[b]: off[b + 1]])
        assert torch.equal(pa, pin[off[b]: off[b + 1]]) and torch.equal(fa, fup[off[b]: off[b + 1]])
    # decode_ragged with lengths (5, 0, 33): entries beyond the lengths hold out-of-range values
    lens = (5, 0, 33)
    g = torch.Generator().manual_seed(8)
    cr = torch.randint(0, 4096, (3, 33, 2), generator=g, dtype=torch.int32)
    lists = [cr[b, :n].reshape(-1).tolist() for b, n in enumerate(lens)]
    for b, n in enumerate(lens):
        cr[b, n:] = 1 << 20
    n_invalid = torch.zeros(1, dtype=torch.int32, device="cuda")
    wav = eng.decode_ragged(cr, lens, n_invalid=n_invalid)
    assert int(n_invalid) == 0
    codec = DistilCodec(cfg)
    codec._eng = eng  # the module's engine: same weights, same kernels
    for b, n in enumerate(lens):
        assert not wav[b, 256 * n:].any()
        if n:
            alone = codec.decode_from_codes(lists[b], minus_token_offset=False)
            assert torch.equal(alone[0, 0], wav[b, : 256 * n])
    outs = codec.decode_from_codes_batch(lists, minus_token_offset=False, ragged=True)
    assert [o.shape[-1] for o in outs] == [256 * n for n in lens]
    assert torch.equal(outs[2][0, 0], wav[2, : 256 * 33])
    with pytest.raises(ValueError, match="multiple"):
        codec.decode_from_codes(lists[0][:-1], minus_token_offset=False)
    with pytest.raises(ValueError, match="multiple"):
        codec.decode_from_codes_batch([lists[0][:-1]], minus_token_offset=False, ragged=True)
    bad = list(lists[2])
    bad[5] = 4096
    with pytest.raises(IndexError):
        codec.decode_from_codes(bad, minus_token_offset=False)
    cr[2, 3, 1] = 4096  # below clip 2's length: counted
    eng.decode_ragged(cr, lens, n_invalid=n_invalid)
    assert int(n_invalid) == 1


def test_graph_and_halo_stream(gen2):
    from distilcodec_nabeel_amd import synth
    from distilcodec_nabeel_amd.streaming import GraphedHop, HaloStream

    eng, _ = gen2
    hop = GraphedHop(eng, 24000)
    assert hop.codes.shape == (1, 93, 2)
    audio = np.concatenate(synth.clips(1, 24000 * 2, seed=9, kind="speech")).astype(np.float32)
    for i in range(2):
        chunk = torch.from_numpy(audio[i * 24000:(i + 1) * 24000]).cuda()[None]
        codes, wav = eng.encode_decode(torch.nn.functional.pad(chunk, (1, 0)))
        gc, gw = hop(chunk)
        torch.cuda.synchronize()
        assert torch.equal(gc, codes) and torch.equal(gw, wav)
    clip = synth.clips(1, 2 * 24000 + 77, seed=11, kind="mix")[0].astype(np.float32)
    hs = HaloStream(eng, record_codes=True)
    outs = [hs.push(clip[i:i + 24000]) for i in range(0, clip.size, 24000)] + [hs.flush()]
    stream_codes = torch.cat(hs.code_log)
    full, wav_full = eng.encode_decode(torch.from_numpy(np.concatenate([[0.0], clip]).astype(np.float32)).cuda()[None])
    assert stream_codes.shape == full[0].shape and hs.n_codes == full.shape[1]
    assert torch.equal(stream_codes, full[0])
    assert torch.cat(outs).numel() == wav_full.shape[1]


def test_errors(engines, state):
    from distilcodec_nabeel_amd import _native
    from distilcodec_nabeel_amd.engine import NativeCodec

    eng, cfg = engines("b1", "x6")
    assert eng.L.dcx_num_codebooks(eng.h) == 3 and eng.L.dcx_abi_version() == 4
    assert eng.L.dcx_set_num_codebooks(eng.h, 2) == _native.DCX_ERR_STATE  # after finalize
    st = _state(cfg, state)
    q = dict(st["quantizer"])
    del q["grvq.rvqs.0.layers.2._codebook.embed"]
    with pytest.raises(KeyError, match="layers.2"):
        NativeCodec(cfg, dict(st, quantizer=q), "cuda:0", with_generator=False)
    # the setter's range, on a handle that is not finalized
    h = ctypes.c_void_p()
    assert eng.L.dcx_create(ctypes.byref(eng.c), ctypes.byref(h)) == _native.DCX_OK
    try:
        assert eng.L.dcx_num_codebooks(h) == 1
        for n in (0, 9):
            assert eng.L.dcx_set_num_codebooks(h, n) == _native.DCX_ERR_INVALID_ARG
        assert eng.L.dcx_set_num_codebooks(h, 8) == _native.DCX_OK and eng.L.dcx_num_codebooks(h) == 8
    finally:
        eng.L.dcx_destroy(h)
    with pytest.raises(ValueError, match="n_codebooks"):
        NativeCodec(RV.rvq_cfg(n_codebooks=9), st, "cuda:0", with_generator=False)
    with pytest.raises(ValueError):
        eng.vq_decode(torch.zeros(1, 5, dtype=torch.int32))  # codes without the layer axis
    # an out-of-range code in layer 2 is counted by the kernel (the Python surface raises before)
    codes = torch.zeros(1, 9, 3, dtype=torch.int32, device="cuda")
    codes[0, 4, 2] = 4096
    z = torch.empty(1, 9, eng.D, device="cuda")
    n_invalid = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = eng.workspace(1, 9)
    eng._check(eng.L.dcx_vq_decode(eng.h, eng._ptr(codes), 1, 9, eng._ptr(z), eng._ptr(n_invalid), eng._ptr(ws),
                                   ws.numel(), eng._stream()))
    assert int(n_invalid) == 1
