"""h3 range scaling on batches whose clips and rows differ in scale.

The h3 arithmetic stores every operand tensor as x * 2^a, a chosen per clip (the tap convs) or per
row (the one-tap convs) and undone in the consumer's accumulators (dcx_kernels.h h2_shift, RangeProg;
DESIGN.md §3 "h3 dynamic range").  tests/test_gpu_range.py scales a whole call by one power of two, so
every clip and every row of a call gets the same shift and a kernel that reads clip 0's shift for
clip 1, the previous tile's clip for the next, or row q for row r0 + q computes the same bits.  Here
the scale differs inside the batch: a loud clip beside a near-silent one, a spike in a quiet clip,
all-zero rows and an all-zero clip, rows of one clip 2^24 apart, more pair-kernel tiles than CUs
(every workgroup crosses clips), and the encoder's half-batches.

Every error is taken per clip or per row (tests/_parity.py rel_per_clip / rel_per_row /
snr_per_clip): the batch-wide max|err| / max|ref| is carried by the loudest clip.  The reference is
the fp64 oracle (oracle/reference_cpu.py).  Bounds, the project's own:
  * relative error < 2e-4 for every clip (every row in the per-row cases);
  * per clip, h3 error < 4 * max(x6 error, 1e-7), x6 measured in the same test with the knob off
    (the rule of tests/test_gpu_range.py); the rows of the spike clip outside the spike's reach get the
    2e-4 bound alone, relative to their own maximum: the clip's shift is set by the spike, so the
    absolute floor 2^-39 B of the h3 error bound 2^-22 |x| + 2^-39 B (dcx_kernels.h) grows relative
    to them, which x6 (full fp32 exponent) does not pay (measured: 3.5e-7 at worst, as every other
    clip; the floor is 2^-29 of rows 2^10 below their clip's bound);
  * waveforms: per-clip SNR >= 80 dB and >= the x6 run's - 12 dB (test_generator_scaled_vs_fp64);
  * range flags clear; a clip alone, a reordered batch, every instantiated pair-kernel tile height
    (forced with DCX_RP_R), another h3 tiling or stream split: same bits.
Reference modules: generators.py:118-147, convnext_utils.py:106-113,137-138,186-213,263-282,
encoders.py:68-76, grfvq.py:68-96, residual_vq.py:152.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import reference_cpu as R

from _parity import check_codes, check_wave, rel_per_clip, rel_per_row, snr_per_clip

pytestmark = pytest.mark.gpu

SPIKE = slice(20, 24)   # rows of the spike clip multiplied by 2^10
# rows a ParallelBlock carries the spike: k = 11, dilations 1, 3, 5 (c1) and 1 (c2) of three pairs:
# 5 (1 + 3 + 5) + 3 * 5 = 60 rows either side, so rows 84 onward never see it
QUIET0 = SPIKE.stop - 1 + 60 + 1


@pytest.fixture(scope="module")
def eng(cfg, state):
    from distilcodec_nabeel_amd.engine import NativeCodec

    e = NativeCodec(cfg, state, "cuda:0", gemm="x6")
    e.range_flags(reset=True)
    return e


@pytest.fixture(autouse=True)
def _clear_flags(eng):
    eng.range_flags(reset=True)
    yield


def mixed_clips(C, L, seed):
    """(4, C, L): a 2^12 clip, a 2^-12 clip, an N(0, 1) clip with rows 20..23 at 2^10, a zero clip."""
    x = np.random.default_rng(seed).standard_normal((4, C, L))
    x[0] *= 2.0 ** 12
    x[1] *= 2.0 ** -12
    x[2][:, SPIKE] *= 2.0 ** 10
    x[3] = 0.0
    return x.astype(np.float32)


def mixed_rows(C, seed, L=96):
    """(3, C, L): row blocks of 24 at 2^12, 2^-12, 1, 2^6; a uniform 2^-12 clip; rows 30..59 zero."""
    x = np.random.default_rng(seed).standard_normal((3, C, L))
    for i, sc in enumerate((12, -12, 0, 6)):
        x[0][:, 24 * i: 24 * (i + 1)] *= 2.0 ** sc
    x[1] *= 2.0 ** -12
    x[2][:, 30:60] = 0.0
    return x.astype(np.float32)


def _cl(x):
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to("cuda:0")


def _run(eng, name, x, **knobs):
    """Module `name` on x (B, C, L) as the oracle lays it out -> (B, C', L')."""
    with eng.knobs(**knobs):
        y = eng.module(name, _cl(x)).cpu().numpy()
    return y.transpose(0, 2, 1)


def _fmt(v):
    return "[" + ", ".join(f"{float(a):.3g}" for a in np.asarray(v).reshape(-1)) + "]"


def _check_clips(tag, y6, y3, ref):
    """The per-clip bounds; returns (x6, h3) per-clip errors."""
    e6, e3 = rel_per_clip(y6, ref), rel_per_clip(y3, ref)
    print(f"\n{tag}: per clip, x6 rel err {_fmt(e6)}, h3 rel err {_fmt(e3)}")
    assert np.isfinite(y3).all(), tag
    assert (e3 < 2e-4).all(), (tag, e3)
    assert (e3 < 4 * np.maximum(e6, 1e-7)).all(), (tag, e3, e6)
    return e6, e3


def _check_alone(eng, name, x, full, tag, clips=None, **knobs):
    for b in (range(x.shape[0]) if clips is None else clips):
        one = _run(eng, name, x[b: b + 1], **knobs)
        assert np.array_equal(one[0], full[b]), f"{tag}: clip {b} alone differs from its row of the batch"


def _pblock_ref(x, state, cfg, stage):
    with torch.no_grad():
        return F.silu(R.parallel_block(torch.from_numpy(x).double(), state["generator"], stage, cfg["decoder"],
                                       torch.float64)).numpy()


# conv_res_pair_h3's instantiated tile heights per stage (dcx_resblock.hip launch_res_pair: kH3_64,
# kH3_32); DCX_RP_R forces one of them, any other value leaves the launcher's choice
PAIR_ROWS = {3: (240, 112, 48), 4: (624, 240, 112)}


def _pblock_knob(stage):
    return "DCX_H3" if stage < 3 else "DCX_H3_PAIRS"


# ---------------------------------------------------------------------------------------------
# 1. ParallelBlocks: per-clip ranges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", [0, 1, 2, 3, 4])
def test_parallel_block_mixed_clips(eng, state, cfg, stage):
    """generator.resblocks.<stage> (grouped conv_gemm_x3dw / x3dq launches at stages 0-2, the
    persistent conv_res_pair_h3 at 3-4) on mixed_clips: per-clip bounds against the fp64
    ParallelBlock, the spike clip's quiet rows on their own, a clip alone and the reversed batch."""
    C = cfg["decoder"]["upsample_initial_channel"] >> (stage + 1)
    L = 400
    name, knob = f"generator.resblocks.{stage}", _pblock_knob(stage)
    x = mixed_clips(C, L, 200 + stage)
    ref = _pblock_ref(x, state, cfg, stage)
    y6 = _run(eng, name, x, **{knob: 0})
    y3 = _run(eng, name, x, **{knob: 1})
    assert not np.array_equal(y3, y6)  # the h3 path ran
    _check_clips(f"resblocks.{stage} mixed clips", y6, y3, ref)

    # the spike clip's rows outside the spike's reach: the fp64 reference there does not depend on the
    # spike, and the kernel's error is held to 2e-4 of that region's own maximum
    flat = x[2:3].copy()
    flat[0][:, SPIKE] *= 2.0 ** -10
    ref_flat = _pblock_ref(flat, state, cfg, stage)
    qmax = np.abs(ref[2][:, QUIET0:]).max()
    # unchanged up to fp64 rounding (the oracle's conv blocks its sums by the whole input: measured
    # 5e-16); one row earlier the spike moves the reference by 5e-3 of qmax
    assert np.abs(ref_flat[0][:, QUIET0:] - ref[2][:, QUIET0:]).max() <= 1e-12 * qmax
    assert np.abs(ref_flat[0][:, QUIET0 - 1] - ref[2][:, QUIET0 - 1]).max() > 1e-6 * qmax
    q6 = rel_per_clip(y6[2:3, :, QUIET0:], ref[2:3, :, QUIET0:])[0]
    q3 = rel_per_clip(y3[2:3, :, QUIET0:], ref[2:3, :, QUIET0:])[0]
    ratio = np.abs(ref[2]).max() / qmax
    print(f"resblocks.{stage} spike clip, rows {QUIET0}..: x6 rel err {q6:.3g}, h3 rel err {q3:.3g} "
          f"(clip max / quiet max {ratio:.3g})")
    assert q3 < 2e-4, q3

    _check_alone(eng, name, x, y3, f"resblocks.{stage}")
    rev = _run(eng, name, np.ascontiguousarray(x[::-1]))
    assert np.array_equal(rev[::-1], y3), f"resblocks.{stage}: reversed batch differs"
    for r in PAIR_ROWS.get(stage, ()):  # the pair kernel at each of its tile heights, forced
        assert np.array_equal(_run(eng, name, x, DCX_RP_R=r), y3), f"resblocks.{stage}: tile height {r} differs"
    assert eng.range_flags() == 0


# ---------------------------------------------------------------------------------------------
# 2. the persistent pair kernel across clips of different scale
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage,rows,L", [(3, 48, 4800), (4, 112, 11200)])
def test_pair_kernel_tiles_cross_clips(eng, state, cfg, stage, rows, L):
    """conv_res_pair_h3 at its smallest tile (DCX_RP_R) on 6 clips alternating 2^10 / 2^-10: at least
    twice as many tiles as CUs, so every workgroup runs tiles of more than one clip with the next
    clip's shift prefetched (dcx_resblock.hip tile_shifts)."""
    C = cfg["decoder"]["upsample_initial_channel"] >> (stage + 1)
    B = 6
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = -(-L // rows) * B
    assert tiles >= 2 * cus, (tiles, cus)
    name = f"generator.resblocks.{stage}"
    x = np.random.default_rng(300 + stage).standard_normal((B, C, L))
    for b in range(B):
        x[b] *= 2.0 ** (10 if b % 2 == 0 else -10)
    x = x.astype(np.float32)
    ref = _pblock_ref(x, state, cfg, stage)
    y6 = _run(eng, name, x, DCX_H3_PAIRS=0)
    y3 = _run(eng, name, x, DCX_H3_PAIRS=1, DCX_RP_R=rows)
    assert not np.array_equal(y3, y6)
    _check_clips(f"resblocks.{stage} R={rows}, {tiles} tiles on {cus} CUs", y6, y3, ref)
    # every other instantiated tile height, forced, on the same batch (on 256 CUs the launcher's own
    # choice here is `rows` already, so the unforced run would compare the kernel with itself)
    assert PAIR_ROWS[stage][-1] == rows
    for r in PAIR_ROWS[stage][:-1]:
        assert np.array_equal(_run(eng, name, x, DCX_RP_R=r), y3), f"tile height {r} differs from {rows}"
    assert np.array_equal(_run(eng, name, x), y3), "the launcher's own tile height differs"
    _check_alone(eng, name, x, y3, f"resblocks.{stage} R={rows}", clips=(0, 5), DCX_RP_R=rows)
    assert eng.range_flags() == 0


# ---------------------------------------------------------------------------------------------
# 3. tilings and grouped launches
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage,knobs", [(0, {"DCX_H3_BN": 128}), (0, {"DCX_H3_BN": 256}), (0, {"DCX_H3_SPLIT": 0}),
                                         (2, {"DCX_H3_BN": 128}), (2, {"DCX_H3_SPLIT": 0})],
                         ids=lambda v: "-".join(f"{k}={w}" for k, w in v.items()) if isinstance(v, dict) else str(v))
def test_tilings_agree_mixed_clips(eng, cfg, stage, knobs):
    """Every h3 tiling (conv_gemm_x3dw, the x3dq tilings of DCX_H3_BN) and the unsplit DMA issue derive
    the clip of a tile on their own (local / tiles_per_clip in the grouped launches): on clips of
    different shifts they give the default run's bits."""
    C = cfg["decoder"]["upsample_initial_channel"] >> (stage + 1)
    name = f"generator.resblocks.{stage}"
    x = mixed_clips(C, 400, 200 + stage)
    y = _run(eng, name, x)
    assert np.isfinite(y).all()
    assert np.array_equal(_run(eng, name, x, **knobs), y)
    assert eng.range_flags() == 0


# ---------------------------------------------------------------------------------------------
# 4. caller-supplied conv inputs (launch_h2_ranged)
# ---------------------------------------------------------------------------------------------
def _five_clips(C, L, seed):
    """(5, C, L): 2^18, 2^-12, 1, the spike clip, zeros."""
    x = np.random.default_rng(seed).standard_normal((5, C, L))
    x[0] *= 2.0 ** 18
    x[1] *= 2.0 ** -12
    x[3][:, SPIKE] *= 2.0 ** 10
    x[4] = 0.0
    return x.astype(np.float32)


def test_conv_pre_mixed_clips(eng, state, cfg):
    """generator.conv_pre (k 13) on a tensor the caller hands over, range-scaled per clip."""
    d, g = cfg["decoder"], state["generator"]
    x = _five_clips(cfg["quantizer"]["input_dim"], 120, 407)
    ref = F.conv1d(torch.from_numpy(x).double(), R._w(g, "conv_pre", torch.float64),
                   R._t(g, "conv_pre.bias", torch.float64), padding=(d["pre_conv_kernel_size"] - 1) // 2).numpy()
    y6 = _run(eng, "generator.conv_pre", x, DCX_H3=0)
    y3 = _run(eng, "generator.conv_pre", x, DCX_H3=1)
    assert not np.array_equal(y3, y6)
    _check_clips("conv_pre five clips", y6, y3, ref)
    _check_alone(eng, "generator.conv_pre", x, y3, "conv_pre")
    assert eng.range_flags() == 0


@pytest.mark.parametrize("i", [0, 1, 2])
def test_conv_transpose_mixed_clips(eng, state, cfg, i):
    """generator.ups.<i> (the h3 ConvTs) likewise."""
    d, g = cfg["decoder"], state["generator"]
    u, k = d["upsample_rates"][i], d["upsample_kernel_sizes"][i]
    x = _five_clips(d["upsample_initial_channel"] >> i, 64, 410 + i)
    ref = F.conv_transpose1d(torch.from_numpy(x).double(), R._w(g, f"ups.{i}", torch.float64),
                             R._t(g, f"ups.{i}.bias", torch.float64), stride=u, padding=(k - u) // 2).numpy()
    name = f"generator.ups.{i}"
    y6 = _run(eng, name, x, DCX_H3=0)
    y3 = _run(eng, name, x, DCX_H3=1)
    assert not np.array_equal(y3, y6)
    _check_clips(f"ups.{i} five clips", y6, y3, ref)
    _check_alone(eng, name, x, y3, f"ups.{i}")
    assert eng.range_flags() == 0


# ---------------------------------------------------------------------------------------------
# 5. per-row ranges
# ---------------------------------------------------------------------------------------------
def _rows_ref(name, x, state, cfg):
    xt = torch.from_numpy(x).double()
    f64 = torch.float64
    with torch.no_grad():
        if name.startswith("encoder.stages."):
            return R.convnext_block(xt, state["encoder"], name[len("encoder."):], f64).numpy()
        if name.startswith("encoder.downsample_layers."):
            sd, p = state["encoder"], name[len("encoder."):]
            h = R.layer_norm_cf(xt, R._t(sd, f"{p}.0.weight", f64), R._t(sd, f"{p}.0.bias", f64))
            return F.conv1d(h, R._t(sd, f"{p}.1.weight", f64), R._t(sd, f"{p}.1.bias", f64)).numpy()
        sd = state["quantizer"]
        if name == "quantizer.downsample.0":
            h = F.conv1d(xt, R._t(sd, "downsample.0.0.weight", f64), R._t(sd, "downsample.0.0.bias", f64))
            return R.convnext_block(h, sd, "downsample.0.1", f64).numpy()
        assert name == "quantizer.grvq.rvqs.0.project_in"
        return F.linear(xt.mT, R._t(sd, "grvq.rvqs.0.project_in.weight", f64),
                        R._t(sd, "grvq.rvqs.0.project_in.bias", f64)).mT.numpy()


ROW_MODULES = [f"encoder.stages.{s}.0" for s in range(4)] + [f"encoder.downsample_layers.{i}" for i in (1, 2, 3)] + \
    ["quantizer.downsample.0", "quantizer.grvq.rvqs.0.project_in"]


@pytest.mark.parametrize("name", ROW_MODULES)
def test_row_ranges_mixed_rows(eng, state, cfg, name):
    """The one-tap convs' per-row shifts (ash_row, the rowwise bound programs, h2_rows, the ln_rows /
    dwconv_ln row maxima) on mixed_rows: every row within 2e-4 of the fp64 module relative to its own
    maximum, the per-clip rule against DCX_H3_1X1=0, a clip alone equal to its row of the batch.
    A zero row of a LayerNorm + 1x1 module gives LayerNorm rows equal to the bias."""
    cin = eng.module_io(name)[0]
    x = mixed_rows(cin, 500 + ROW_MODULES.index(name))
    ref = _rows_ref(name, x, state, cfg)
    y6 = _run(eng, name, x, DCX_H3_1X1=0)
    y3 = _run(eng, name, x, DCX_H3_1X1=1)
    assert not np.array_equal(y3, y6)
    r6, r3 = rel_per_row(y6, ref), rel_per_row(y3, ref)
    w = np.unravel_index(r3.argmax(), r3.shape)
    print(f"\n{name} mixed rows: per row, x6 max rel err {r6.max():.3g}, h3 max rel err {r3.max():.3g} "
          f"(clip {w[0]}, row {w[1]}); h3 per clip {_fmt(r3.max(axis=1))}")
    assert (r3 < 2e-4).all(), (name, r3.max(), w)
    _check_clips(f"{name} mixed rows", y6, y3, ref)
    _check_alone(eng, name, x, y3, name)
    assert eng.range_flags() == 0


# ---------------------------------------------------------------------------------------------
# 6. half-batches
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mel5(golden):
    """(5, n_mels, T): the e2e_3s mel scaled by 2^-6, 1, 2^6 (cycled); clip 2 holds 20 zero rows."""
    m = golden["e2e_3s"]["mel"][0]
    x = np.stack([m * 2.0 ** (-6, 0, 6)[b % 3] for b in range(5)]).astype(np.float32)
    x[2][:, 100:120] = 0.0
    return x


@pytest.fixture(scope="module")
def feat5_ref(mel5, state, cfg):
    with torch.no_grad():  # clips 3 and 4 repeat clips 0 and 1, and the encoder treats every clip alone
        f = R.encoder(torch.from_numpy(mel5[:3]).double(), state["encoder"], tuple(cfg["encoder"]["depths"]),
                      torch.float64).numpy()
    assert np.array_equal(mel5[3], mel5[0]) and np.array_equal(mel5[4], mel5[1])
    return np.concatenate([f, f[:2]])


def _poisoned(eng, B, T):
    """A private workspace for a (B, T) call (sized under the knobs in force) with every word set to
    0xA5A5A5A5 (as a range shift: 2^-1515870811), so that a slot a half-batch reads but never wrote
    cannot hold an earlier run's correct value.  Handed to the call as `ws=`: the engine's shared
    buffer is not involved."""
    return torch.full((eng.workspace_size(B, T),), 0xA5, dtype=torch.uint8, device=eng.device)


@pytest.mark.parametrize("B", [3, 5])
def test_staged_encoder_half_batches(eng, mel5, feat5_ref, B):
    """eng.encode on clips of different scale: the two half-batches (act_rows offsets the per-clip
    and per-row range pointers by b0 / r0) give the one-stream bits, every clip alone gives its row,
    and every clip is within 2e-4 of the fp64 encoder.  Every run starts from a poisoned workspace: the
    halves share one buffer, and a slot of the other half left from an earlier run would hold the
    right value."""
    mel = _cl(mel5[:B])
    assert eng.get_knob("DCX_ENC_STREAMS") == 2
    T = mel.shape[1]
    two = eng.encode(mel, ws=_poisoned(eng, B, T)).clone()
    with eng.knobs(DCX_ENC_STREAMS=0):
        one = eng.encode(mel, ws=_poisoned(eng, B, T)).clone()
    torch.cuda.synchronize()
    assert torch.equal(two, one)
    for b in range(B):
        alone = eng.encode(mel[b: b + 1], ws=_poisoned(eng, 1, T))
        assert torch.equal(alone[0], two[b]), f"clip {b} alone differs from its row"
    e = rel_per_clip(two.transpose(1, 2).cpu().numpy(), feat5_ref[:B])
    print(f"\nencoder B={B}: per clip rel err {_fmt(e)}")
    assert (e < 2e-4).all(), e
    assert eng.range_flags() == 0


def test_encode_decode_half_batches(eng, state, cfg):
    """dcx_encode_decode on a music clip, digital silence and the music clip at 2^-10: every
    DCX_ENC_STREAMS mode gives the same bits, each clip alone its row, and each clip on its own meets
    the code and waveform checks against the fp64 oracle (the loud clip cannot carry the others).
    Every run starts from a poisoned workspace (_poisoned)."""
    from distilcodec_nabeel_amd import synth

    music = synth.music_like(12000, 5).astype(np.float32)
    audio, _ = R.pad_batch([music, np.zeros(12000, np.float32), music * np.float32(2.0 ** -10)])
    ref = R.encode_decode(audio, state, cfg, torch.float64)
    dev = audio.cuda()
    T = eng.num_frames(dev.shape[1])
    with eng.knobs(DCX_ENC_STREAMS=0):
        codes, wav = [t.clone() for t in eng.encode_decode(dev, ws=_poisoned(eng, 3, T))]
    for mode in (1, 2, 3):
        with eng.knobs(DCX_ENC_STREAMS=mode):
            c, w = [t.clone() for t in eng.encode_decode(dev, ws=_poisoned(eng, 3, T))]
        torch.cuda.synchronize()
        assert torch.equal(c, codes) and torch.equal(w, wav), mode
    for b in range(3):
        c, w = [t.clone() for t in eng.encode_decode(dev[b: b + 1], ws=_poisoned(eng, 1, T))]
        assert torch.equal(c[0], codes[b]) and torch.equal(w[0], wav[b]), f"clip {b} alone differs from its row"
    rc = ref["codes"][0, :, :, 0].numpy()
    rw = ref["wav"][:, 0].numpy()
    best, second, _ = R.top2_gap_fp64(ref["x_pjt_in"], R.codebook(state["quantizer"], torch.float64))
    dec = (((second - best) / best) > 1e-4).numpy().reshape(rc.shape)
    for b in range(3):
        match = check_codes(codes[b: b + 1], rc[b: b + 1], dec[b: b + 1], min_match=0.0)
        snr = check_wave(eng, codes[b: b + 1], rc[b: b + 1], wav[b: b + 1], rw[b: b + 1], 80)
        print(f"\nencode_decode clip {b}: codes match {match:.3f} ({int(dec[b].sum())} of {dec[b].size} decisive), "
              f"waveform SNR {snr:.1f} dB")
    assert eng.range_flags() == 0


# ---------------------------------------------------------------------------------------------
# 7. the generator's [slot][clip] range tables
# ---------------------------------------------------------------------------------------------
def test_generator_mixed_clips(eng, golden, state, cfg):
    """eng.generate on three clips of the e2e_3s features scaled by 2^-8, 1, 2^8: every range slot of
    the call (RangeArena, [slot][clip]) holds three different values.  Per-clip SNR against the fp64
    generator (>= 80 dB and >= x6 - 12 dB), each clip alone equal to its row."""
    z1 = golden["e2e_3s"]["quantized"][:, :, :24]
    z = torch.from_numpy(np.concatenate([z1 * 2.0 ** -8, z1, z1 * 2.0 ** 8]).astype(np.float32))  # (3, 1024, 24)
    with torch.no_grad():
        ref = R.generator(z.double(), state["generator"], cfg["decoder"], torch.float64)[:, 0].numpy()
    zc = z.transpose(1, 2).contiguous()
    with eng.knobs(DCX_H3=0, DCX_H3_PAIRS=0):
        w6 = eng.generate(zc).cpu().numpy().reshape(ref.shape)
    w3t = eng.generate(zc).clone()
    w3 = w3t.cpu().numpy().reshape(ref.shape)
    s6, s3 = snr_per_clip(w6, ref), snr_per_clip(w3, ref)
    print(f"\ngenerator 2^-8 / 1 / 2^8: per clip against fp64, x6 {_fmt(s6)} dB, h3 {_fmt(s3)} dB")
    assert np.isfinite(w3).all()
    assert (s3 >= 80).all() and (s3 >= s6 - 12).all(), (s3, s6)
    for b in range(3):
        assert torch.equal(eng.generate(zc[b: b + 1])[0], w3t[b]), f"clip {b} alone differs from its row"
    assert eng.range_flags() == 0
