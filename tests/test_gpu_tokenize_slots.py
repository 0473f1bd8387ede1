"""Slot tokenization (dcx_tokenize_slots, NativeCodec.tokenize_slots): the ragged contract in the padded
layout with the per-slot sample counts in device memory.

Slot b's first T_b = num_frames(n_b + 1) rows equal, bit for bit, `eng.tokenize_ragged([clip])` of the clip
alone (that path's own batch independence is asserted bit-exact in tests/test_gpu_ragged_scale.py);
codes beyond T_b are -1, x_pjt_in rows zero; a slot of fewer than 384 samples is dead.  The same holds
with the audio beyond every n_b and the whole workspace poisoned (NaN and 1e30), with the range flags
of the clean run; in the three dwconv_ln forms (4-row tiles: 5 slots x 40 frames; register ring: 64
slots x 129 frames = 8256 rows; 16-row tiles: the same with DCX_DWCONV_TILED); in bf16 mode (bit-equal
to the bf16 ragged call on each clip alone, which is within any bound tests/test_gpu_ragged.py holds);
and through one graph captured once and replayed with three length vectors.

Lengths: 0, 383 (dead), 384 (one frame), both ends of a frame count's sample range (1278 / 1279: 4 / 5
frames; 1534 / 1535: 5 / 6; 2303 / 2304: 8 / 9), and the full slot."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _rvq_ref as RV

pytestmark = pytest.mark.gpu

B, WF = 5, 40
WS = 256 * WF
VECTORS = [[0, 383, 384, WS, 1279], [1278, 1535, 1534, 5000, 640], [WS, 0, 2303, 2304, 9999]]
# the ring geometry: 64 slots of 129 frames, mostly short clips from a pool of (clip, length)
RB, RWF = 64, 129
RWS = 256 * RWF
RING_POOL = [0, 383, 384, 700, 1279, 3000, 20000, RWS]
JUNK_CODE, JUNK_PIN = 7777, 3.0


@pytest.fixture(scope="module")
def engines(state):
    """Tokenizing engines (no generator) by (mode, codebooks), with a synthetic 4096-entry quantizer as
    tests/test_gpu_token_stream.py builds its engines."""
    from distilcodec_nabeel_amd import weights
    from distilcodec_nabeel_amd.engine import NativeCodec

    cache = {}

    def get(mode="x6", R=1):
        if (mode, R) not in cache:
            cfg = RV.rvq_cfg(4096, 256, R)
            st = {"encoder": state["encoder"], "quantizer": weights.synthetic_quantizer(cfg, seed=RV.FIXTURE_SEED)}
            cache[(mode, R)] = NativeCodec(cfg, st, "cuda:0", with_generator=False, gemm=mode)
        return cache[(mode, R)]

    yield get
    cache.clear()


@pytest.fixture(scope="module")
def audio():
    from distilcodec_nabeel_amd import synth

    return torch.from_numpy(np.stack(synth.clips(B, WS, seed=300, kind="mix"))).float().cuda()


@pytest.fixture(scope="module")
def alone(engines, audio):
    """(mode, R, slot, n) -> (codes, x_pjt_in) of audio[slot, :n] through tokenize_ragged alone; computed
    once per key and never changed."""
    cache = {}

    def get(mode, R, b, n, src=None):
        key = (mode, R, b, n, None if src is None else src.data_ptr())
        if key not in cache:
            clip = (audio if src is None else src)[b, :n]
            codes, off, pin, _ = engines(mode, R).tokenize_ragged([clip], want_pjt_in=True)
            cache[key] = (codes.clone(), pin.clone())
        return cache[key]

    yield get
    cache.clear()


def _frames(n):
    return (n + 1) // 256 if n >= 384 else 0


def _check_against_alone(eng, alone, mode, R, lens, codes, pin, wf, src=None, slot_of=None):
    assert codes.shape == eng._codes_shape(len(lens), wf) and pin.shape == (len(lens), wf, eng.CD)
    for b, n in enumerate(lens):
        t = _frames(n)
        assert t == (eng.num_frames(n + 1) if n >= 384 else 0)
        if t:
            c1, p1 = alone(mode, R, b if slot_of is None else slot_of[b], n, src)
            assert c1.shape[0] == t
            assert torch.equal(codes[b, :t], c1), (b, n, "codes differ from the clip alone")
            assert torch.equal(pin[b, :t], p1), (b, n, "x_pjt_in differs from the clip alone",
                                                 float((pin[b, :t] - p1).abs().max() / p1.abs().max()))
        assert bool((codes[b, t:] == -1).all()), (b, n, "codes beyond the slot's length")
        assert not bool(pin[b, t:].any()), (b, n, "x_pjt_in beyond the slot's length")


@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("vec", range(len(VECTORS)))
def test_x6_equals_each_clip_alone(engines, audio, alone, vec, R):
    eng, lens = engines("x6", R), VECTORS[vec]
    codes, pin = eng.tokenize_slots(audio, lens, want_pjt_in=True)
    _check_against_alone(eng, alone, "x6", R, lens, codes, pin, WF)
    codes_only, none = eng.tokenize_slots(audio, lens)
    assert none is None and torch.equal(codes_only, codes)
    assert eng.range_flags(reset=True) == 0


def test_host_lengths_are_validated(engines, audio):
    eng = engines("x6")
    for bad in ([0, 1, 2, 3], [0, 0, 0, 0, WS + 1], [0, -1, 0, 0, 0]):
        with pytest.raises(ValueError):
            eng.tokenize_slots(audio, bad)
    with pytest.raises(ValueError):
        eng.tokenize_slots(audio, torch.zeros(B, dtype=torch.int64, device="cuda"))
    # a device tensor is used as it stands: the kernels clamp to [0, WS]
    n_dev = torch.tensor([-5, WS + 999, 384, 383, 1 << 30], dtype=torch.int32, device="cuda")
    codes, _ = eng.tokenize_slots(audio, n_dev)
    want, _ = eng.tokenize_slots(audio, [0, WS, 384, 383, WS])
    assert torch.equal(codes, want)


@pytest.mark.parametrize("poison", [float("nan"), 1e30])
def test_dead_regions_are_never_read(engines, audio, poison):
    """The audio beyond every n_b and the whole workspace filled with NaN / 1e30: the same bits and the
    same range flags."""
    eng = engines("x6")
    ws = torch.zeros(eng.slots_workspace_size(B, WS), dtype=torch.uint8, device="cuda")
    for lens in VECTORS:
        eng.range_flags(reset=True)
        codes, pin = eng.tokenize_slots(audio, lens, want_pjt_in=True, ws=ws)
        codes, pin = codes.clone(), pin.clone()
        flags = eng.range_flags(reset=True)
        dirty = audio.clone()
        for b, n in enumerate(lens):
            dirty[b, n:] = poison
        ws[:ws.numel() // 4 * 4].view(torch.float32).fill_(poison)
        codes2 = torch.full_like(codes, JUNK_CODE)
        pin2 = torch.full_like(pin, poison)
        eng.tokenize_slots(dirty, lens, ws=ws, codes=codes2, pjt_in=pin2)
        assert torch.equal(codes2, codes) and torch.equal(pin2, pin), lens
        assert eng.range_flags(reset=True) == flags == 0


def test_slot_independence(engines, audio):
    """A slot's bits depend on neither its neighbours' lengths nor their contents."""
    eng = engines("x6")
    base_c, base_p = eng.tokenize_slots(audio, VECTORS[1], want_pjt_in=True)
    for keep in range(B):
        other = audio.flip(1) * 3.0
        other[keep] = audio[keep]
        lens = [VECTORS[2][b] if b != keep else VECTORS[1][b] for b in range(B)]
        c, p = eng.tokenize_slots(other, lens, want_pjt_in=True)
        assert torch.equal(c[keep], base_c[keep]) and torch.equal(p[keep], base_p[keep]), keep


def test_bf16(engines, audio, alone):
    eng = engines("bf16")
    for lens in VECTORS[:2]:
        codes, pin = eng.tokenize_slots(audio, lens, want_pjt_in=True)
        assert torch.equal(pin, pin.to(torch.bfloat16).to(torch.float32))  # bf16-valued, as the ragged path's
        _check_against_alone(eng, alone, "bf16", 1, lens, codes, pin, WF)


@pytest.fixture(scope="module")
def ring_case():
    from distilcodec_nabeel_amd import synth

    rng = np.random.default_rng(5)
    pool_audio = torch.from_numpy(np.stack(synth.clips(len(RING_POOL), RWS, seed=400, kind="mix"))).float().cuda()
    pick = [int(x) for x in rng.integers(0, 6, size=RB)]  # mostly the short entries
    pick[3], pick[17], pick[40], pick[63] = 6, 7, 6, 7  # and a few long ones, the last slot full
    return pool_audio, pick, pool_audio[pick].contiguous(), [RING_POOL[i] for i in pick]


@pytest.mark.parametrize("tiled", [0, 1])
def test_ring_and_16_row_tiles(engines, alone, ring_case, tiled):
    """8256 rows: the register ring (run width 4), and with DCX_DWCONV_TILED the 16-row tiles (576 tiles
    >= 512); both give every slot the bits of its clip alone."""
    eng = engines("x6")
    pool_audio, pick, batch, lens = ring_case
    assert RB * RWF >= 8192 and RB * ((RWF + 15) // 16) >= 512
    with eng.knobs(DCX_DWCONV_TILED=tiled):
        codes, pin = eng.tokenize_slots(batch, lens, want_pjt_in=True)
    _check_against_alone(eng, alone, "x6", 1, lens, codes, pin, RWF, src=pool_audio, slot_of=pick)
    assert eng.range_flags(reset=True) == 0


def test_one_captured_graph_serves_any_lengths(engines, audio):
    eng = engines("x6")
    n_dev = torch.zeros(B, dtype=torch.int32, device="cuda")
    static = audio.clone()
    codes = torch.empty(B, WF, dtype=torch.int32, device="cuda")
    pin = torch.empty(B, WF, eng.CD, device="cuda")
    ws = torch.empty(eng.slots_workspace_size(B, WS), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eng.tokenize_slots(static, n_dev, ws=ws, codes=codes, pjt_in=pin)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.tokenize_slots(static, n_dev, ws=ws, codes=codes, pjt_in=pin)
    for lens in VECTORS:
        want_c, want_p = eng.tokenize_slots(audio, lens, want_pjt_in=True)
        n_dev.copy_(torch.tensor(lens, dtype=torch.int32))
        codes.fill_(JUNK_CODE)
        pin.fill_(JUNK_PIN)
        graph.replay()
        assert torch.equal(codes, want_c) and torch.equal(pin, want_p), lens


def test_refusals_leave_the_outputs_untouched(engines, audio):
    from distilcodec_nabeel_amd import _native

    eng = engines("x6")
    lens = VECTORS[0]
    codes = torch.full((B, WF), JUNK_CODE, dtype=torch.int32, device="cuda")
    pin = torch.full((B, WF, eng.CD), JUNK_PIN, device="cuda")
    ws = torch.empty(eng.slots_workspace_size(B, WS) + (160 << 20), dtype=torch.uint8, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((codes == JUNK_CODE).all()) and bool((pin == JUNK_PIN).all())

    eng.set_gemm("f32")
    try:
        with pytest.raises(ValueError, match="DCX_GEMM_X6 or DCX_GEMM_BF16"):
            eng.tokenize_slots(audio, lens, ws=ws, codes=codes, pjt_in=pin)
    finally:
        eng.set_gemm("x6")
    assert untouched()
    eng.set_split_k(4)
    try:
        with pytest.raises(_native.NativeError, match="split-K") as e:
            eng.tokenize_slots(audio, lens, ws=ws, codes=codes, pjt_in=pin)
        assert e.value.status == _native.DCX_ERR_STATE
    finally:
        eng.set_split_k(0)
    assert untouched()
    # a short workspace and a slot size below the reflect pad are refused before any launch too
    n_dev = torch.tensor(lens, dtype=torch.int32, device="cuda")
    rc = eng.L.dcx_tokenize_slots(eng.h, eng._ptr(audio), eng._ptr(n_dev), B, WS, eng._ptr(codes), eng._ptr(pin),
                                  eng._ptr(ws), 1 << 16, eng._stream())
    assert rc == _native.DCX_ERR_WORKSPACE and untouched()
    rc = eng.L.dcx_tokenize_slots(eng.h, eng._ptr(audio), eng._ptr(n_dev), B, 383, eng._ptr(codes), eng._ptr(pin),
                                  eng._ptr(ws), ws.numel(), eng._stream())
    assert rc == _native.DCX_ERR_INVALID_ARG and untouched()
    got, _ = eng.tokenize_slots(audio, lens, ws=ws, codes=codes, pjt_in=pin)  # and the next call is as ever
    assert bool((got[0] == -1).all()) and bool((got[3] >= 0).all())
