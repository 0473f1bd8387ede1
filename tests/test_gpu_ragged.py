"""Ragged-batch tokenization (dcx_tokenize_ragged, NativeCodec.tokenize_ragged, DistilCodec.encode(ragged=True)):
clips of different lengths packed row-wise with no padding, every clip's result what the clip gives
ALONE.  The reference for a clip is therefore the CPU oracle on that clip alone (`pad_batch([clip])`),
never on the padded batch.

Set A: raw lengths 400, 700, 1800, 4300, 8500, 30000 -> 1, 2, 7, 16, 33, 117 frames (shorter than the k7
halo, equal to the kernel size, at and across several 4-row tile edges, long); 176 rows in 15 16-row
tiles, fewer than 512: dwconv_ln_seg_kernel<NV, 4>, the 4-row tiles.  No clip here meets a 16-row tile.
Set B: 24 clips of 80000 + 1111 i samples (312 .. 412 frames each), 8684 rows (the sum of
dcx_num_frames(n + 1)): dwconv_ln_run_seg_kernel<NV, 4, D>, the register ring at run width 4 (8192 ..
16383 rows).
The 16-row tiles (dwconv_ln_seg_kernel<NV, 16>), the run widths 8, 16 and 32, and clips shorter than a
run or the ring's window inside such batches are in tests/test_gpu_ragged_scale.py.

Tolerances: codes exact on decisive frames (fp64 relative top-2 gap > 1e-4) and >= 97 % overall
(tests/_parity.py); x_pjt_in max relative error < 2e-4 (the bound of tests/test_gpu_stages.py).  bf16
mode: the ragged path's error against the oracle's fp32 x_pjt_in at most 1.25 x the existing bf16
path's on the same clips alone (relative Frobenius error over the 176 rows, and the max-norm relative
error of tests/test_gpu_stages.py: the stem sums its K = 896 in another order, which moves single bf16
roundings but not the error statistics).  Measured on the MI355X: Frobenius 8.0348e-3 (padded path,
each clip alone) against 8.0364e-3 (ragged), max norm 8.956e-3 against 9.583e-3; not bit-equal.
"""
import numpy as np
import pytest
import torch
from _parity import check_codes

pytestmark = pytest.mark.gpu

LEN_A = [400, 700, 1800, 4300, 8500, 30000]
FRAMES_A = [1, 2, 7, 16, 33, 117]


def _rel(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def _fro(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


@pytest.fixture(scope="module")
def clips_a():
    from distilcodec_nabeel_amd import synth

    return [synth.clips(1, n, seed=40 + i, kind="mix")[0] for i, n in enumerate(LEN_A)]


@pytest.fixture(scope="module")
def oracle_a(clips_a, cfg, state):
    """The CPU oracle on each clip alone, concatenated over the clips: codes [176], x_pjt_in [176][3584],
    the decisive mask and the fp64 argmin."""
    from oracle import reference_cpu as R

    emb = R.codebook(state["quantizer"])
    codes, pin = [], []
    with torch.no_grad():
        for c in clips_a:
            audio, _ = R.pad_batch([c])
            feat = R.encoder(R.log_mel(audio), state["encoder"], tuple(cfg["encoder"]["depths"]))
            vq = R.vq_forward(feat, state["quantizer"])
            codes.append(vq["codes"][0, 0, :, 0])
            pin.append(vq["x_pjt_in"][0])
    codes, pin = torch.cat(codes), torch.cat(pin)
    best, second, arg = R.top2_gap_fp64(pin, emb)
    return {"codes": codes.numpy(), "pin": pin, "decisive": (((second - best) / best) > 1e-4).numpy(), "arg64": arg.numpy(),
            "emb": emb}


@pytest.fixture(scope="module")
def engines(cfg, state):
    from distilcodec_nabeel_amd.engine import NativeCodec

    return {"x6": NativeCodec(cfg, state, "cuda:0", gemm="x6"), "bf16": NativeCodec(cfg, state, "cuda:0", gemm="bf16")}


@pytest.fixture(scope="module")
def ragged_a(engines, clips_a):
    """Set A through the ragged call, once per mode: (codes, offsets, x_pjt_in, quantized_fup) on the host side
    of a synchronised stream."""
    out = {}
    for mode, eng in engines.items():
        codes, off, pin, fup = eng.tokenize_ragged(clips_a, want_pjt_in=True, want_fup=True)
        torch.cuda.synchronize()
        out[mode] = (codes.clone(), off, pin.clone(), fup.clone())
    return out


def test_set_a_frames_and_decisive_share(engines, ragged_a, oracle_a):
    codes, off, pin, fup = ragged_a["x6"]
    assert np.diff(off.numpy()).tolist() == FRAMES_A
    assert codes.shape == (176,) and codes.dtype == torch.int32
    assert pin.shape == (176, 3584) and fup.shape == (176, 3584)
    share = float(oracle_a["decisive"].mean())
    print(f"\nset A: {int(oracle_a['decisive'].sum())} of 176 frames decisive ({share:.3f})")
    assert share >= 0.90
    assert np.array_equal(oracle_a["codes"], oracle_a["arg64"])  # the oracle's fp32 codes are the fp64 argmin


def test_set_a_x6_against_oracle(engines, ragged_a, oracle_a):
    codes, off, pin, fup = ragged_a["x6"]
    match = check_codes(codes, oracle_a["codes"], oracle_a["decisive"])
    err = _rel(pin, oracle_a["pin"])
    print(f"\nset A x6: codes match {match:.4f}, x_pjt_in max rel err {err:.3e}")
    assert err < 2e-4
    assert torch.equal(fup.cpu(), oracle_a["emb"][codes.cpu().long()])
    assert engines["x6"].range_flags(reset=True) == 0


@pytest.mark.parametrize("mode", ["x6", "bf16"])
def test_set_a_isolation(engines, ragged_a, clips_a, mode):
    """In order, in reverse order, and each clip as a batch of one: bit-identical per clip.  The same
    kernels on independent rows, so any difference is a leak across a clip boundary."""
    eng = engines[mode]
    codes, off, pin, _ = ragged_a[mode]
    off = off.tolist()
    rc, roff, rpin, _ = eng.tokenize_ragged(clips_a[::-1], want_pjt_in=True)
    roff = roff.tolist()
    B = len(clips_a)
    for b in range(B):
        rb = B - 1 - b
        sl, rsl = slice(off[b], off[b + 1]), slice(roff[rb], roff[rb + 1])
        assert torch.equal(codes[sl], rc[rsl]), (b, "reverse codes")
        assert torch.equal(pin[sl], rpin[rsl]), (b, "reverse x_pjt_in")
        c1, o1, p1, _ = eng.tokenize_ragged([clips_a[b]], want_pjt_in=True)
        assert o1.tolist() == [0, FRAMES_A[b]]
        assert torch.equal(codes[sl], c1), (b, "alone codes")
        assert torch.equal(pin[sl], p1), (b, "alone x_pjt_in")


def test_set_a_bf16(engines, ragged_a, clips_a, oracle_a):
    from oracle import reference_cpu as R

    eng = engines["bf16"]
    codes, off, pin, _ = ragged_a["bf16"]
    assert torch.equal(pin, _bf(pin))  # bf16-valued, like autocast's Linear output
    E = oracle_a["emb"].to("cuda:0", torch.float64)
    P = pin.double()
    d = (P ** 2).sum(1)[:, None] + (E ** 2).sum(1)[None] - 2.0 * P @ E.T
    assert np.array_equal(codes.cpu().numpy(), torch.argmin(d, 1).cpu().numpy())
    # accuracy against the parent's path: the existing bf16 stages on each clip alone
    pad = []
    for c in clips_a:
        audio, _ = R.pad_batch([c])
        _, p, _, _ = eng.vq_encode(eng.encode(eng.mel(audio)), want_fup=False, want_quantized=False)
        pad.append(p[0].clone())
    pad = torch.cat(pad)
    e_pad, e_rag = _fro(pad, oracle_a["pin"]), _fro(pin, oracle_a["pin"])
    same = torch.equal(pad, pin)
    print(f"\nset A bf16: e_pad {e_pad:.6e} e_rag {e_rag:.6e} ratio {e_rag / e_pad:.4f} "
          f"(max-norm: pad {_rel(pad, oracle_a['pin']):.4e} rag {_rel(pin, oracle_a['pin']):.4e}); bit-equal to the alone path: {same}")
    assert e_rag <= 1.25 * e_pad
    assert _rel(pin, oracle_a["pin"]) <= 1.25 * _rel(pad, oracle_a["pin"])  # and in the max norm of test_gpu_stages.py


def test_set_b_register_ring_kernel(engines, state):
    """8684 rows: the >= 8192-row dwconv_ln form, against the ragged call on each clip alone (the
    tiled form, validated by set A)."""
    from distilcodec_nabeel_amd import synth
    from oracle import reference_cpu as R

    eng = engines["x6"]
    lens = [80000 + 1111 * i for i in range(24)]
    clips = [synth.clips(1, n, seed=100 + i, kind="mix")[0] for i, n in enumerate(lens)]
    codes, off, pin, _ = eng.tokenize_ragged(clips, want_pjt_in=True)
    off = off.tolist()
    assert off[-1] == sum(eng.num_frames(n + 1) for n in lens) == 8684 and off[-1] >= 8192
    E = R.codebook(state["quantizer"]).to("cuda:0", torch.float64)
    e2 = (E ** 2).sum(1)
    total = differ = 0
    worst = 0.0
    for b, c in enumerate(clips):
        c1, _, p1, _ = eng.tokenize_ragged([c], want_pjt_in=True)
        sl = slice(off[b], off[b + 1])
        worst = max(worst, _rel(pin[sl], p1))
        ne = (codes[sl] != c1).nonzero().reshape(-1)
        total += c1.numel()
        differ += int(ne.numel())
        for s in range(0, int(ne.numel()), 32):  # fp64 top-2 gap of the differing rows only
            x = p1[ne[s: s + 32]].double()
            dist = ((x ** 2).sum(1)[:, None] + e2[None] - 2.0 * x @ E.T).clamp(min=0).sqrt()
            v, _ = torch.topk(dist, 2, dim=1, largest=False)
            assert bool((((v[:, 1] - v[:, 0]) / v[:, 0]) <= 1e-4).all()), (b, "a decisive frame differs")
    print(f"\nset B: x_pjt_in max rel err {worst:.3e}, {differ} of {total} codes differ")
    assert worst < 2e-4
    assert 1.0 - differ / total >= 0.97
    assert eng.range_flags(reset=True) == 0


def test_launch_count_independent_of_clip_count(engines, clips_a):
    eng = engines["x6"]
    counts = []
    eng.profile(True)
    try:
        for clips in (clips_a[:2], clips_a):
            eng.profile_reset()
            eng.tokenize_ragged(clips, want_pjt_in=True, want_fup=True)
            prof = eng.profile_read()
            counts.append(sum(v["launches"] for v in prof.values()))
            assert any(k.startswith("dwconv_ln_ragged") for k in prof), sorted(prof)
    finally:
        eng.profile(False)
        eng.profile_reset()
    print(f"\nlaunches: 2 clips {counts[0]}, 6 clips {counts[1]}")
    assert counts[0] == counts[1] > 0


@pytest.fixture(scope="module")
def codec(cfg):
    from distilcodec_nabeel_amd import DistilCodec

    c = DistilCodec(cfg)
    c.move_to_cuda()
    return c


def test_codec_encode_ragged(codec, clips_a):
    from oracle import reference_cpu as R

    sel = [clips_a[2], clips_a[4], clips_a[3]]
    frames = [7, 33, 16]
    items = [[c, 24000] for c in sel]
    eng = codec._engine()
    ret, gen_len, n_hop = codec.encode(items, raw_audio=True, ragged=True, codes_only=True)
    assert ret.codes.shape == (1, 3, 33, 1) and ret.codes.dtype == torch.int64
    assert ret.quantized is None and ret.x_pjt_in is None and ret.quantized_fup is None
    codes, off, _, _ = eng.tokenize_ragged(sel)
    off = off.tolist()
    for b, t in enumerate(frames):
        row = ret.codes[0, b, :, 0]
        assert torch.equal(row[:t].to(torch.int32), codes[off[b]: off[b + 1]])
        assert bool((row[:t] >= 0).all()) and bool((row[t:] == -1).all())
        n = sel[b].shape[0] // 256
        assert n_hop[b] == n and len(ret.codes_list[b]) == n
        want = codec.audio_tokenize(codes=codes[off[b]: off[b] + n].cpu().tolist(), n_groups=codec.ngroups, n_residual=codec.nresiduals)
        assert ret.codes_list[b] == want
    # with the features: packed tensors and trimmed per-clip lists
    full, _, _ = codec.encode(items, raw_audio=True, ragged=True)
    assert full.x_pjt_in.shape == (56, 3584) and full.quantized_fup.shape == (56, 3584)
    for b in range(3):
        n = sel[b].shape[0] // 256
        assert full.x_pjt_in_list[b].shape == (2 * n, 1792)
        assert torch.equal(full.x_pjt_in_list[b].reshape(n, -1), full.x_pjt_in[off[b]: off[b] + n].cpu())
    # the default stays the padded batch: same codes as the staged calls on the padded audio, no -1
    dflt, _, n_hop2 = codec.encode(items, raw_audio=True, codes_only=True)
    audio, _ = R.pad_batch(sel)
    staged, *_ = eng.vq_encode(eng.encode(eng.mel(audio)), want_pjt_in=False, want_fup=False, want_quantized=False)
    assert dflt.codes.shape == (1, 3, 33, 1)
    assert torch.equal(dflt.codes[0, :, :, 0], staged.long())
    assert bool((dflt.codes >= 0).all())
    assert n_hop2 == n_hop


def test_minus_one_padding_decodes(codec, clips_a):
    """A ragged row with its -1 tail kept goes through decode_from_codes_batch: -1 is the reference's
    masked code (dcx_vq_decode), not an index error."""
    items = [[clips_a[2], 24000], [clips_a[3], 24000]]
    ret, _, _ = codec.encode(items, raw_audio=True, ragged=True, codes_only=True)
    row = ret.codes[0, 0, :, 0].cpu().tolist()
    assert row[7:] == [-1] * 9
    wavs = codec.decode_from_codes_batch([row], minus_token_offset=False)
    assert len(wavs) == 1 and wavs[0].shape == (1, 1, 256 * 16)
    assert bool(torch.isfinite(wavs[0]).all())
