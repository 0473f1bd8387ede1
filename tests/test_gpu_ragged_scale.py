"""Ragged tokenization (dcx_tokenize_ragged) at the batch sizes where launch_dwconv_ln_ragged leaves
the 4-row tiles of tests/test_gpu_ragged.py's set A: the 16-row tiles (>= 512 of them below 8192 rows)
and the register ring at run widths 4, 8, 16 and 32 (8192 * {1, 2, 4, 8} rows); the last case also
takes ragged_frames_kernel and ragged_unfold_kernel through the second trip of their grid-stride
loops (> 65536 rows).

The pool (tests/_parity.py): 19 short clips of 1 .. 65 frames, below the 7-row window and the ring's
prefetch distance, then just below, at and just above every tile and run width, their sample counts at
the two ends of the range that gives T frames, and one 937-frame filler.  A batch is the pool
repeated and shuffled with a fixed seed, so that long and short clips alternate, a workgroup's four
runs belong to different clips and seg_find searches up to 480 clips.  Every case asserts its row
class from the plan (host only) before anything is launched.

Checks, per case:
 (a) every copy of a pool clip in one call has bit-identical x_pjt_in rows and codes (x6, bf16): one
     launch per step over independent rows, so a difference is a leak across a clip boundary or a
     wrong clip lookup;
 (b) DCX_DWCONV_TILED=1 (dwconv_ln_seg_kernel<NV, 16> from 8192 rows on) gives the same bits (x6,
     bf16): both forms claim the same per-row arithmetic in the same order;
 (c) x6 against each pool clip through tokenize_ragged([clip]) (the 4-row tiles set A pins to the
     oracle): BIT-EQUAL x_pjt_in and codes in all five cases, measured on the MI355X and asserted here
     (DESIGN.md §3 "Batch independence": in x6 mode no kernel choice follows the total row count);
     set B's bounds (max relative error < 2e-4 per clip, codes differing only where the alone
     x_pjt_in's fp64 top-2 gap is <= 1e-4, >= 97 % equal) are asserted first and hold trivially;
 (d) x6 against the CPU oracle on each of the 19 short clips alone: x_pjt_in max relative error < 2e-4
     per clip copy, codes exact on decisive frames (fp64 relative top-2 gap > 1e-4; 339 of the 376
     frames, 0.902) and >= 97 % overall, and the batch's codes the fp64 argmin of its own x_pjt_in;
 (e) the h3 range flags stay clear.

Measured on the MI355X, the same in all five cases: ragged against alone max relative error 0 and 0
codes differing (bit-equal); ragged against the oracle 2.457e-6 over the 380 / 418 copies of the short
clips, every code equal.
"""
import numpy as np
import pytest
import torch
from _parity import (RAGGED_CASES, RAGGED_LONG_T, RAGGED_SHORT_T, check_codes, ragged_case_order,
                     ragged_pool_lengths)

pytestmark = pytest.mark.gpu

POOL_T = RAGGED_SHORT_T + [RAGGED_LONG_T]
N_SHORT = len(RAGGED_SHORT_T)
SHORT_ROWS = sum(RAGGED_SHORT_T)  # the short clips' rows lead the pool's concatenation


@pytest.fixture(scope="module")
def pool():
    """The pool's clips as host arrays (the oracle's input) and device tensors (the batches')."""
    from distilcodec_nabeel_amd import synth

    host = [synth.clips(1, n, seed=300 + i, kind="mix")[0] for i, n in enumerate(ragged_pool_lengths())]
    return host, [torch.from_numpy(np.ascontiguousarray(c)).to("cuda:0", torch.float32) for c in host]


@pytest.fixture(scope="module")
def engines(cfg, state):
    from distilcodec_nabeel_amd.engine import NativeCodec

    sd = {"encoder": state["encoder"], "quantizer": state["quantizer"]}
    return {m: NativeCodec(cfg, sd, "cuda:0", with_generator=False, gemm=m) for m in ("x6", "bf16")}


@pytest.fixture(scope="module")
def emb(state):
    from oracle import reference_cpu as R

    return R.codebook(state["quantizer"])


@pytest.fixture(scope="module")
def oracle(pool, cfg, state, emb):
    """The CPU oracle on each short clip alone (as oracle_a of tests/test_gpu_ragged.py), concatenated:
    codes [376], x_pjt_in [376][3584], the decisive mask, and each clip's max |x_pjt_in|."""
    from oracle import reference_cpu as R

    codes, pin = [], []
    with torch.no_grad():
        for c in pool[0][:N_SHORT]:
            audio, _ = R.pad_batch([c])
            feat = R.encoder(R.log_mel(audio), state["encoder"], tuple(cfg["encoder"]["depths"]))
            vq = R.vq_forward(feat, state["quantizer"])
            codes.append(vq["codes"][0, 0, :, 0])
            pin.append(vq["x_pjt_in"][0])
    assert [p.shape[0] for p in pin] == RAGGED_SHORT_T
    amax = torch.stack([p.abs().max() for p in pin])
    codes, pin = torch.cat(codes), torch.cat(pin)
    best, second, arg = R.top2_gap_fp64(pin.cuda(), emb.cuda())
    decisive = (((second - best) / best) > 1e-4).cpu().numpy()
    assert np.array_equal(codes.numpy(), arg.cpu().numpy())  # the oracle's fp32 codes are the fp64 argmin
    return {"codes": codes.numpy(), "pin": pin.cuda(), "amax": amax.cuda().double(), "decisive": decisive}


@pytest.fixture(scope="module")
def alone(engines, pool, emb):
    """x6, every pool clip as a ragged batch of one (1 .. 59 16-row tiles: the 4-row tiles),
    concatenated in pool order: codes [1313], x_pjt_in [1313][3584], the decisive mask of these
    x_pjt_in rows and each clip's max |x_pjt_in|."""
    from oracle import reference_cpu as R

    eng = engines["x6"]
    codes, pin = [], []
    for c, t in zip(pool[1], POOL_T):
        plan, _, tf = eng.ragged_plan([c.numel()])
        assert tf == t and (t + 15) // 16 < 512 and t < 8192
        cd, off, p, _ = eng.tokenize_ragged([c], want_pjt_in=True)
        assert off.tolist() == [0, t]
        codes.append(cd.clone())
        pin.append(p.clone())
    amax = torch.stack([p.abs().max() for p in pin]).double()
    codes, pin = torch.cat(codes), torch.cat(pin)
    best, second, _ = R.top2_gap_fp64(pin, emb.cuda())
    assert eng.range_flags(reset=True) == 0
    return {"codes": codes, "pin": pin, "amax": amax, "decisive": ((second - best) / best) > 1e-4}


def _row_class(eng, lengths):
    """The dwconv_ln form launch_dwconv_ln_ragged selects for these clips, from the plan alone: 0 for
    the 16-row tiles, -1 for the 4-row tiles, else the ring's run width."""
    plan, _, tf = eng.ragged_plan(lengths)
    B = len(lengths)
    arrs = plan[plan.shape[0] - 5 * (B + 1):].reshape(5, B + 1)
    frames = [eng.num_frames(n + 1) for n in lengths]
    assert np.diff(arrs[1]).tolist() == frames and tf == sum(frames)
    if tf < 8192:
        return tf, (0 if sum((t + 15) // 16 for t in frames) >= 512 else -1)
    rw = 32 if tf >= 65536 else 16 if tf >= 32768 else 8 if tf >= 16384 else 4
    assert np.diff(arrs[4]).tolist() == [(t + rw - 1) // rw for t in frames]  # the runs the ring walks
    return tf, rw


@pytest.fixture(scope="module", params=list(RAGGED_CASES))
def batch(request, engines, pool):
    """One case through the ragged call in both modes, with and without DCX_DWCONV_TILED (the knob
    changes nothing below 8192 rows, so t16 runs once per mode).  Module-scoped so that the tests of one
    case share the launches; the results (0.95 GB of x_pjt_in per run at rw32) go when the case ends."""
    case = request.param
    _, _, total, form = RAGGED_CASES[case]
    order = ragged_case_order(case)
    lengths = ragged_pool_lengths()
    rows, got = _row_class(engines["x6"], [lengths[i] for i in order])
    assert (rows, got) == (total, form), (case, rows, got)  # before anything is launched
    clips = [pool[1][i] for i in order]
    out = {"case": case, "order": order, "tiled": form != 0}
    for mode, eng in engines.items():
        codes, off, pin, _ = eng.tokenize_ragged(clips, want_pjt_in=True)
        out[mode] = (codes.clone(), pin.clone())
        if form != 0:
            with eng.knobs(DCX_DWCONV_TILED=1):
                codes, _, pin, _ = eng.tokenize_ragged(clips, want_pjt_in=True)
                out[mode + "_tiled"] = (codes.clone(), pin.clone())
                torch.cuda.synchronize()
        if mode == "x6":
            out["flags"] = eng.range_flags(reset=True)
    assert off[-1] == total and np.diff(off.numpy()).tolist() == [POOL_T[i] for i in order]
    # row -> its clip in the batch, the first copy's same row, and the same row of the pool's concatenation
    t = torch.tensor([POOL_T[i] for i in order])
    clip = torch.repeat_interleave(torch.arange(len(order)), t)
    within = torch.arange(total) - off[:-1][clip]
    first = {}
    for b, i in enumerate(order.tolist()):
        first.setdefault(i, b)
    first_of = torch.tensor([first[i] for i in order.tolist()])
    pool_off = torch.tensor(np.concatenate([[0], np.cumsum(POOL_T)]))
    out["clip"] = clip.cuda()
    out["first_row"] = (off[:-1][first_of[clip]] + within).cuda()
    out["pool_row"] = (pool_off[torch.from_numpy(order)[clip]] + within).cuda()
    out["pool_clip"] = torch.from_numpy(order).cuda()
    yield out
    out.clear()
    torch.cuda.empty_cache()


def _bad_clips(batch, rows_bad):
    """(batch position, pool index) of the clips that own the flagged rows."""
    pos = torch.unique(batch["clip"][rows_bad]).cpu().tolist()
    return [(b, int(batch["order"][b])) for b in pos][:8]


@pytest.mark.parametrize("mode", ["x6", "bf16"])
def test_copies_agree(batch, mode):
    codes, pin = batch[mode]
    assert bool(torch.isfinite(pin).all())
    fr = batch["first_row"]
    bad = (pin != pin[fr]).any(1) | (codes != codes[fr])
    assert not bool(bad.any()), (batch["case"], mode, "copies differ at (position, pool clip)", _bad_clips(batch, bad))


@pytest.mark.parametrize("mode", ["x6", "bf16"])
def test_tiled_and_ring_forms_agree(batch, mode):
    if not batch["tiled"]:
        return  # below 8192 rows the knob selects nothing else: t16 is the tiled form already
    codes, pin = batch[mode]
    tcodes, tpin = batch[mode + "_tiled"]
    bad = (pin != tpin).any(1) | (codes != tcodes)
    assert not bool(bad.any()), (batch["case"], mode, "forms differ at (position, pool clip)", _bad_clips(batch, bad))
    assert torch.equal(pin, tpin) and torch.equal(codes, tcodes)


def _rel_per_copy(batch, pin, ref, amax):
    """max |pin - ref| over each clip copy's rows / max |ref| of its pool clip: [clips in the batch]."""
    err = (pin.double() - ref.double()).abs().amax(1)
    per = torch.zeros(batch["pool_clip"].numel(), dtype=torch.float64, device=pin.device)
    per.scatter_reduce_(0, batch["clip"], err, "amax", include_self=True)
    return per / amax[batch["pool_clip"]]


def test_against_each_clip_alone(batch, alone):
    codes, pin = batch["x6"]
    ref, rcodes = alone["pin"][batch["pool_row"]], alone["codes"][batch["pool_row"]]
    rel = _rel_per_copy(batch, pin, ref, alone["amax"])
    ne = codes != rcodes
    bit_equal = torch.equal(pin, ref) and not bool(ne.any())
    print(f"\n{batch['case']} ragged against alone: x_pjt_in max rel err {float(rel.max()):.3e}, "
          f"{int(ne.sum())} of {ne.numel()} codes differ, bit-equal: {bit_equal}")
    assert float(rel.max()) < 2e-4, (batch["case"], _bad_clips(batch, (rel >= 2e-4)[batch["clip"]]))
    assert not bool((ne & alone["decisive"][batch["pool_row"]]).any()), "a decisive frame differs"
    assert 1.0 - float(ne.sum()) / ne.numel() >= 0.97
    assert bit_equal  # measured on the MI355X in all five row classes (module docstring)


def test_against_oracle(batch, oracle, emb):
    from test_gpu_vq import _argmin_fp64

    codes, pin = batch["x6"]
    share = float(oracle["decisive"].mean())
    assert share >= 0.85, share
    short = batch["pool_row"] < SHORT_ROWS  # rows of the short clips' copies
    rows = batch["pool_row"][short]
    clips = batch["pool_clip"] < N_SHORT
    # the long clip's rows compare with themselves (no oracle for them) and are left out below
    ref = torch.where(short[:, None], oracle["pin"][batch["pool_row"].clamp(max=SHORT_ROWS - 1)], pin)
    amax = torch.cat([oracle["amax"], oracle["amax"].new_ones(1)])
    rel = _rel_per_copy(batch, pin, ref, amax)[clips]
    assert rel.numel() == N_SHORT * RAGGED_CASES[batch["case"]][0]
    rows_h = rows.cpu().numpy()
    got = codes[short].cpu().numpy()
    print(f"\n{batch['case']} ragged against the oracle: x_pjt_in max rel err {float(rel.max()):.3e} over {rel.numel()} "
          f"copies of the short clips, decisive share {share:.3f}")
    assert float(rel.max()) < 2e-4
    match = check_codes(got, oracle["codes"][rows_h], oracle["decisive"][rows_h])
    print(f"{batch['case']} codes match {match:.4f}")
    assert np.array_equal(got, _argmin_fp64(pin[short], emb))


def test_range_flags_clear(batch):
    assert batch["flags"] == 0
