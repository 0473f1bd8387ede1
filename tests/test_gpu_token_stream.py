"""Token streams (streaming.TokenStream, dcx_stream_decode_step): batched streaming decode of codes
that arrive a few frames per step, for several sessions at once.

The bookkeeping is exact: every step's samples are, bit for bit, the slices of `eng.decode_ragged` on
windows the test assembles itself from plain Python lists by the documented semantics.  A graph replay
equals the eager step bit for bit; a slot's bits do not depend on what its neighbours do.  Against the
full-clip decode of an utterance's codes the concatenated output has the same length and SNR >= 110 dB,
the bound tests/test_gpu_stream_halo.py holds HaloStream to for the same comparison (windows of another
length pick other conv tilings and other per-clip h3 range scales: fp32 summation order).  Measured on
MI355X (DESIGN.md §5 "Token streams"): 125.0-155.7 dB with one codebook, 126.5-129.1 dB with two, and
bit-equal for the utterances that fit one window; 10.3 dB with the halo of 4.  A halo of 4 frames, well below the decoder's receptive field
(streaming.receptive_field: 22 frames, rounded up), falls below 80 dB on the long utterance: the
comparison can fail.  The tests run with a halo of 21 frames, W = 50."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _rvq_ref as RV

pytestmark = pytest.mark.gpu

B, P, H = 3, 8, 21
W = P + 2 * H
FINAL, RESTART = 1, 2
MIN_DB = 110.0
JUNK = 1 << 20


def _snr(x, ref):
    err = (x.double() - ref.double()).pow(2).sum().item()
    return 10 * np.log10(ref.double().pow(2).sum().item() / max(err, 1e-300))


@pytest.fixture(scope="module")
def engines(state):
    """x6 engines with the generator by codebook count, built as tests/test_gpu_rvq.py builds gen2."""
    from distilcodec_nabeel_amd import weights
    from distilcodec_nabeel_amd.engine import NativeCodec

    cache = {}

    def get(R):
        if R not in cache:
            cfg = RV.rvq_cfg(4096, 256, R)
            st = {"encoder": state["encoder"], "quantizer": weights.synthetic_quantizer(cfg, seed=RV.FIXTURE_SEED),
                  "generator": state["generator"]}
            cache[R] = NativeCodec(cfg, st, "cuda:0", with_generator=True, gemm="x6")
        return cache[R]

    yield get
    cache.clear()


# ------------------------------------------------------------------------------------------------
# schedules: per step, per slot (codes [n, R] or None, flags)
# ------------------------------------------------------------------------------------------------
def _utterance(seed, frames, R, nc=4096):
    return np.random.default_rng(seed).integers(0, nc, size=(frames, R)).astype(np.int32)


def _pushes(codes, pattern, start, final_extra=None):
    """{step: (codes, flags)} of one utterance pushed by `pattern` (cycled) from step `start`; FINAL with
    the last codes, or on the step `final_extra` later that pushes none."""
    out, at, i = {}, 0, 0
    while at < len(codes):
        n = min(pattern[i % len(pattern)], len(codes) - at)
        last = at + n == len(codes) and final_extra is None
        out[start + i] = (codes[at:at + n], FINAL if last else 0)
        at += n
        i += 1
    if final_extra is not None:
        out[start + i - 1 + final_extra] = (codes[:0], FINAL)
    return out


def _slot1(R, seed=20):
    """Idle, a 5-frame utterance that ends in its first step (shorter than the halo), then a RESTART with
    a 30-frame one."""
    s = _pushes(_utterance(seed, 5, R), [8], 3)
    for k, (c, f) in _pushes(_utterance(seed + 1, 30, R), [8], 6).items():
        s[k] = (c, f | (RESTART if k == 6 else 0))
    return s


def _main_slots(R):
    """Slot 0: 130 frames pushed as 8, 3, 0, 8, 1, 8, 8, 5, ... (the ring wraps more than twice); slot 1:
    _slot1; slot 2: 61 frames, FINAL on a later step that pushes nothing."""
    return [_pushes(_utterance(10, 130, R), [8, 3, 0, 8, 1, 8, 8, 5], 0), _slot1(R),
            _pushes(_utterance(30, 61, R), [8], 0, final_extra=2)]


def _steps(slots):
    n = 1 + max(max(s) for s in slots if s)
    return [[s.get(i) for s in slots] for i in range(n)]


def _drive(ts, steps):
    """Push a schedule through a TokenStream -> per step (outputs per slot, n_out, wav_out), on the host."""
    rec = []
    for step in steps:
        codes = [None if e is None else e[0] for e in step]
        final = [b for b, e in enumerate(step) if e is not None and e[1] & FINAL]
        restart = [b for b, e in enumerate(step) if e is not None and e[1] & RESTART]
        outs = ts.push(codes, final=final, restart=restart)
        rec.append(([o.cpu() for o in outs], ts.n_out.cpu().tolist(), ts.wav_out.cpu()))
    return rec


def _reference(eng, steps, halo=H):
    """The semantics on plain Python lists: per step, the windows [B][W] and lengths assembled here,
    decoded by eng.decode_ragged, and the emitted slices of its output.  Also every finished utterance
    as (slot, codes, [its emitted pieces])."""
    R = eng.R
    codes = [[] for _ in range(B)]
    E, closed = [0] * B, [False] * B
    pieces = [[] for _ in range(B)]
    rec, done = [], []
    for step in steps:
        win = np.full((B, P + 2 * halo, R), JUNK, dtype=np.int32)
        lens, cut = [0] * B, [(0, 0)] * B
        for b, e in enumerate(step):
            new, flags = (np.zeros((0, R), np.int32), 0) if e is None else e
            if flags & RESTART:
                codes[b], E[b], closed[b], pieces[b] = [], 0, False, []
            if not closed[b]:
                codes[b].extend(new.tolist())
            T = len(codes[b])
            g0 = max(0, E[b] - halo)
            f_new = T if flags & FINAL else max(E[b], T - halo)
            lens[b] = T - g0
            if lens[b]:
                win[b, :lens[b]] = np.asarray(codes[b][g0:T], dtype=np.int32).reshape(-1, R)
            cut[b] = (E[b] - g0, f_new - E[b])
            E[b] = f_new
        wav = eng.decode_ragged(torch.from_numpy(win if R > 1 else win[:, :, 0]), lens).cpu()
        outs = [wav[b, 256 * s:256 * (s + t)] for b, (s, t) in enumerate(cut)]
        rec.append((outs, [t for _, t in cut]))
        for b, e in enumerate(step):
            pieces[b].append(outs[b])
            if e is not None and e[1] & FINAL and not closed[b]:
                closed[b] = True
                done.append((b, np.asarray(codes[b], dtype=np.int32).reshape(-1, R), torch.cat(pieces[b])))
    return rec, done


@pytest.fixture(scope="module")
def runs(engines):
    """The main schedule through an eager TokenStream and through the reference, per codebook count."""
    from distilcodec_nabeel_amd.streaming import TokenStream

    cache = {}

    def get(R):
        if R not in cache:
            eng = engines(R)
            steps = _steps(_main_slots(R))
            ts = TokenStream(eng, B, P, H)
            assert ts.wav_out.shape == (B, 256 * (P + H))
            got = _drive(ts, steps)
            assert int(ts.n_invalid.item()) == 0
            ref, done = _reference(eng, steps)
            cache[R] = {"steps": steps, "got": got, "ref": ref, "done": done, "slots": [ts.slot(b) for b in range(B)]}
        return cache[R]

    yield get
    cache.clear()


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2])
def test_bookkeeping_is_exact(runs, R):
    r = runs(R)
    assert len(r["steps"]) >= 25
    emitted = 0
    for i, ((outs, n_out, wav_out), (want, take)) in enumerate(zip(r["got"], r["ref"])):
        assert n_out == take, i
        for b in range(B):
            assert outs[b].shape == (256 * take[b],), (i, b)
            assert torch.equal(outs[b], want[b]), (i, b)
            assert torch.equal(wav_out[b, :256 * take[b]], want[b]), (i, b)
            assert not wav_out[b, 256 * take[b]:].any(), (i, b)  # the zero tail
            emitted += take[b]
    assert emitted == 130 + 5 + 30 + 61
    assert r["slots"] == [(130, 130, True), (30, 30, True), (61, 61, True)]
    assert max(t for _, take in r["ref"] for t in take) == 7 + H  # slot 0's FINAL step: its 7 frames and the halo's


def test_graph_replay_equals_eager(engines, runs):
    """One graph, captured before any code is pushed, replayed for every step of the schedule."""
    from distilcodec_nabeel_amd.streaming import TokenStream

    r = runs(1)
    ts = TokenStream(engines(1), B, P, H, graph=True)
    assert ts.graph is not None
    got = _drive(ts, r["steps"])
    for i, ((outs, n_out, wav_out), (outs_e, n_out_e, wav_out_e)) in enumerate(zip(got, r["got"])):
        assert n_out == n_out_e, i
        assert torch.equal(wav_out, wav_out_e), i
        assert all(torch.equal(a, b) for a, b in zip(outs, outs_e)), i
    assert int(ts.n_invalid.item()) == 0


def test_isolation(engines, runs):
    """Slot 1's schedule with its neighbours idle, busy, and busy with other codes and restarts: the same
    bits.  The same utterance in slot 0 and in slot 2: the same bits."""
    from distilcodec_nabeel_amd.streaming import TokenStream

    eng = engines(1)
    s1 = _slot1(1)
    n = 1 + max(s1)
    busy = [step[0][1] for step in runs(1)["got"][:n]]
    idle = [step[0][1] for step in _drive(TokenStream(eng, B, P, H), _steps([{}, s1, {}]))]
    # both neighbours: a 40-frame utterance, then a RESTART with a 12-frame one while slot 1 is busy
    other = _pushes(_utterance(40, 40, 1), [8, 5], 0)
    k = 1 + max(other)
    for j, (c, f) in _pushes(_utterance(41, 12, 1), [8], k).items():
        other[j] = (c, f | (RESTART if j == k else 0))
    both = _drive(TokenStream(eng, B, P, H), _steps([other, s1, dict(other)]))
    assert k + 1 < n
    assert sum(o.numel() for o in idle) == 256 * 35
    for i in range(n):
        assert torch.equal(idle[i], busy[i]), i
        assert torch.equal(idle[i], both[i][0][1]), i
        assert torch.equal(both[i][0][0], both[i][0][2]), i
    assert sum(step[0][0].numel() for step in both) == 256 * 52


@pytest.mark.parametrize("R", [1, 2])
def test_against_full_clip_decode(engines, runs, R):
    eng = engines(R)
    done = runs(R)["done"]
    assert sorted(len(c) for _, c, _ in done) == [5, 30, 61, 130]
    for b, codes, wav in done:
        c = torch.from_numpy(codes if R > 1 else codes[:, 0])[None]
        full = eng.generate(eng.vq_decode(c))[0].cpu()
        snr = _snr(wav, full)
        print(f"\nR={R} slot {b}, {len(codes)} frames: SNR vs the full-clip decode {snr:.1f} dB", end="")
        assert wav.numel() == full.numel() == 256 * len(codes)
        assert snr >= MIN_DB


def test_short_halo_breaks_equality(engines):
    from distilcodec_nabeel_amd.streaming import TokenStream

    eng = engines(1)
    steps = _steps([_main_slots(1)[0], {}, {}])
    ts = TokenStream(eng, B, P, halo_frames=4)
    wav = torch.cat([step[0][0] for step in _drive(ts, steps)])
    full = eng.generate(eng.vq_decode(torch.from_numpy(_utterance(10, 130, 1)[:, 0])[None]))[0].cpu()
    assert wav.numel() == full.numel()
    snr = _snr(wav, full)
    print(f"\nhalo 4: SNR vs the full-clip decode {snr:.1f} dB", end="")
    assert snr < 80


def test_codes_never_read(engines):
    """Entries of new_codes at or beyond a slot's count hold 1 << 20 throughout and are never read or
    counted; a code equal to codebook_size inside a count is counted once, not again by the later windows
    that hold it."""
    eng = engines(1)
    dev = eng.device
    state = eng.stream_state(B, P, H)
    new = torch.full((B, P), JUNK, dtype=torch.int32, device=dev)
    n_new = torch.zeros(B, dtype=torch.int32, device=dev)
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    wav = torch.empty(B, 256 * (P + H), device=dev)
    n_out = torch.zeros(B, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    u = _utterance(50, 40, 1)[:, 0]

    def step(counts, fl=(0, 0, 0)):
        n_new.copy_(torch.tensor(counts, dtype=torch.int32))
        flags.copy_(torch.tensor(fl, dtype=torch.int32))
        eng.stream_step(state, B, P, H, new, n_new, flags, wav, n_out, bad)
        return n_out.cpu().tolist()

    at = 0
    for counts in ([3, 0, 8], [0, 0, 0], [8, 1, 5], [8, 8, 8]):
        new.fill_(JUNK)
        for b, n in enumerate(counts):
            new[b, :n] = torch.from_numpy(u[at:at + n]).to(dev)
        at += 8
        step(counts)
    assert int(bad.item()) == 0 and torch.isfinite(wav).all()
    new.fill_(JUNK)
    new[0, :4] = torch.tensor([1, eng.NC, 2, 3], dtype=torch.int32)
    assert step([4, 0, 0]) == [2, 0, 0]  # slot 0: T = 23, E 0 -> 2
    assert int(bad.item()) == 1
    new.fill_(JUNK)
    assert step([0, 0, 0], (FINAL, FINAL, FINAL)) == [21, 9, 21]
    assert int(bad.item()) == 1  # the window held the bad code again


def test_errors(engines):
    from distilcodec_nabeel_amd import _native
    from distilcodec_nabeel_amd.streaming import TokenStream

    eng = engines(1)
    ts = TokenStream(eng, B, P, H)
    first = ts.push([np.arange(8), None, [5, 6]], final=[2])
    assert [o.numel() for o in first] == [0, 0, 512]
    before = [ts.slot(b) for b in range(B)]
    assert before == [(8, 0, False), (0, 0, False), (2, 2, True)]
    with pytest.raises(ValueError, match="push_frames"):
        ts.push([np.arange(9), None, None])
    with pytest.raises(ValueError):
        ts.push([None, None])
    with pytest.raises(ValueError):
        ts.push([np.zeros((2, 2), np.int64), None, None])
    with pytest.raises(RuntimeError, match="closed"):
        ts.push([None, None, [1]])
    for bad in (eng.NC, -1):
        with pytest.raises(IndexError):
            ts.push([[1, bad], None, None])
    assert [ts.slot(b) for b in range(B)] == before  # a refused push changes nothing
    again = ts.push([None, None, [7, 8, 9]], restart=[2])  # a closed slot takes codes with a restart
    assert ts.slot(2) == (3, 0, False) and again[2].numel() == 0
    from distilcodec_nabeel_amd.streaming import receptive_field

    assert TokenStream(eng, B, P).halo_frames == receptive_field(eng.cfg)[1]
    with pytest.raises(ValueError):
        TokenStream(eng, 0, P)
    with pytest.raises(ValueError):
        TokenStream(eng, B, 0)
    with pytest.raises(ValueError):
        TokenStream(eng, B, P, halo_frames=-1)
    # the arithmetic the ragged decode refuses is refused here with the same status and reason, and the
    # refused step leaves the slots as they were
    probe = TokenStream(eng, B, P, H)
    want = probe.push([np.arange(8), np.arange(3), None])
    want2 = probe.push([np.arange(8) + 9, None, None], final=[1])
    ts = TokenStream(eng, B, P, H)
    ts.push([np.arange(8), np.arange(3), None])
    for mode in ("bf16", "f32"):
        eng.set_gemm(mode)
        try:
            with pytest.raises(ValueError, match="DCX_GEMM_X6"):
                ts.push([np.arange(8) + 9, None, None], final=[1])
        finally:
            eng.set_gemm("x6")
    eng.set_split_k(16)
    try:
        with pytest.raises(_native.NativeError, match="split-K") as e:
            ts.push([np.arange(8) + 9, None, None], final=[1])
        assert e.value.status == _native.DCX_ERR_STATE
    finally:
        eng.set_split_k(0)
    for knob in ("DCX_H3", "DCX_H3_PAIRS"):
        with eng.knobs(**{knob: 0}):
            with pytest.raises(ValueError, match="ragged decode"):
                ts.push([np.arange(8) + 9, None, None], final=[1])
    assert [ts.slot(b) for b in range(B)] == [(8, 0, False), (3, 0, False), (0, 0, False)]
    got2 = ts.push([np.arange(8) + 9, None, None], final=[1])
    assert all(torch.equal(a, b) for a, b in zip(got2, want2)) and got2[1].numel() == 256 * 3 and len(want) == B
    # a short state buffer or workspace
    state = eng.stream_state(B, P, H)
    args = (torch.zeros(B, P, dtype=torch.int32, device=eng.device), *(torch.zeros(B, dtype=torch.int32, device=eng.device) for _ in range(2)),
            torch.zeros(B, 256 * (P + H), device=eng.device), torch.zeros(B, dtype=torch.int32, device=eng.device))
    with pytest.raises(ValueError, match="state buffer"):
        eng.stream_step(state[:-256], B, P, H, *args)
    with pytest.raises(ValueError):
        eng.stream_step(state, B, P, H, *args, ws=torch.empty(1 << 16, dtype=torch.uint8, device=eng.device))
    with pytest.raises(ValueError):
        eng.stream_step(state, B, P, H, args[0][:, :4].contiguous(), *args[1:])


def test_token_surface(engines, runs):
    """DistilCodec.token_stream: push_tokens with ids offset by token_id_offset reproduces the
    engine-level outputs bit for bit (a second engine with the same weights, one captured graph)."""
    import distilcodec_nabeel_amd as pkg
    from distilcodec_nabeel_amd import DistilCodec

    assert pkg.TokenStream is not None and "TokenStream" in pkg.__all__
    cfg = RV.rvq_cfg(4096, 256, 1)
    cfg["token_id_offset"] = 151665
    codec = DistilCodec(cfg)
    codec.move_to_cuda()
    ts = codec.token_stream(B, P, H)
    assert ts.graph is not None and ts.halo_frames == H and ts.token_id_offset == 151665
    r = runs(1)
    for i, step in enumerate(r["steps"][:12]):
        ids = [None if e is None else (e[0].reshape(-1).astype(np.int64) + 151665).tolist() for e in step]
        final = [b for b, e in enumerate(step) if e is not None and e[1] & FINAL]
        restart = [b for b, e in enumerate(step) if e is not None and e[1] & RESTART]
        outs = ts.push_tokens(ids, final=final, restart=restart)
        for b in range(B):
            assert outs[b].shape == (1, 1, r["got"][i][0][b].numel())
            assert torch.equal(outs[b][0, 0].cpu(), r["got"][i][0][b]), (i, b)
    raw = ts.push_tokens([[3, 4], None, None], minus_token_offset=False)
    assert raw[0].shape[:2] == (1, 1)
    with pytest.raises(IndexError):
        ts.push_tokens([[3, 4], None, None])  # ids below the offset
    # R ids per frame
    ts2 = pkg.TokenStream(engines(2), B, P, H)
    with pytest.raises(ValueError, match="multiple"):
        ts2.push_tokens([[1, 2, 3], None, None])
    outs = ts2.push_tokens([[1, 2, 3, 4], None, None], final=[0])
    assert outs[0].shape == (1, 1, 512) and ts2.slot(0) == (2, 2, True)
