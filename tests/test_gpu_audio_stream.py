"""Audio streams (streaming.AudioStream, dcx_stream_encode_step): batched streaming tokenization of
audio that arrives a chunk per step, for several sessions at once; the mirror of
tests/test_gpu_token_stream.py.

The bookkeeping is exact: every step's codes and x_pjt_in rows are, bit for bit, the slices of
`eng.tokenize_slots` on windows the test assembles itself from plain Python lists by the documented
semantics (include/distilcodec_amd.h, "Audio streams"), with everything beyond a window's length
poisoned.  A graph replay equals the eager step bit for bit; a slot's bits do not depend on what its
neighbours do.  An utterance's concatenated codes have the full clip's length and equal
`eng.tokenize_ragged([clip])` on every frame, x_pjt_in included: with the halo of 60 frames (the
encoder's half receptive field) every emitted frame sees the inputs it sees in the full clip, and the
ragged path's kernels compute a row the same way whatever shares its launch.  With a halo of 8 frames
x_pjt_in differs on the long utterance: the comparison can fail.

B = 3, P = 2048, h = 60: Ws = 34048 samples, Wf = 133 frames, K = 70.  Slot 0: 72000 samples pushed as
2048, 700, 0, 2048, 1, 2048, 2048, 1500, ... (the ring wraps twice); slot 1: idle, then 5000 samples
that end in their third push (a push holds at most 2048), then a RESTART with 20000; slot 2: 30000
samples, FINAL on a later push that holds nothing."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _rvq_ref as RV

pytestmark = pytest.mark.gpu

B, P, H = 3, 2048, 60
WS, WF, K = 34048, 133, 70
FINAL, RESTART = 1, 2
N_COUNTERS = 12


@pytest.fixture(scope="module")
def engines(state):
    """x6 engines by codebook count, built as tests/test_gpu_token_stream.py builds its own (no generator:
    the stream tokenizes)."""
    from distilcodec_nabeel_amd import weights
    from distilcodec_nabeel_amd.engine import NativeCodec

    cache = {}

    def get(R):
        if R not in cache:
            cfg = RV.rvq_cfg(4096, 256, R)
            st = {"encoder": state["encoder"], "quantizer": weights.synthetic_quantizer(cfg, seed=RV.FIXTURE_SEED)}
            cache[R] = NativeCodec(cfg, st, "cuda:0", with_generator=False, gemm="x6")
        return cache[R]

    yield get
    cache.clear()


# ------------------------------------------------------------------------------------------------
# schedules: per step, per slot (samples [n] or None, flags)
# ------------------------------------------------------------------------------------------------
def _utterance(seed, n):
    from distilcodec_nabeel_amd import synth

    return np.asarray(synth.clips(1, n, seed=seed, kind="mix")[0], dtype=np.float32)


def _pushes(x, pattern, start, final_extra=None):
    out, at, i = {}, 0, 0
    while at < len(x):
        n = min(pattern[i % len(pattern)], len(x) - at)
        last = at + n == len(x) and final_extra is None
        out[start + i] = (x[at:at + n], FINAL if last else 0)
        at += n
        i += 1
    if final_extra is not None:
        out[start + i - 1 + final_extra] = (x[:0], FINAL)
    return out


def _main_slots():
    s1 = _pushes(_utterance(21, 5000), [P], 3)
    first = 3 + len(s1)
    for k, (c, f) in _pushes(_utterance(22, 20000), [P], first).items():
        s1[k] = (c, f | (RESTART if k == first else 0))
    return [_pushes(_utterance(20, 72000), [2048, 700, 0, 2048, 1, 2048, 2048, 1500], 0), s1,
            _pushes(_utterance(23, 30000), [P], 0, final_extra=2)]


def _steps(slots):
    n = 1 + max(max(s) for s in slots if s)
    return [[s.get(i) for s in slots] for i in range(n)]


def _drive(st, steps):
    """Push a schedule through an AudioStream -> per step (codes per slot, n_out, x_pjt_in rows per slot)."""
    rec = []
    for step in steps:
        chunks = [None if e is None else e[0] for e in step]
        final = [b for b, e in enumerate(step) if e is not None and e[1] & FINAL]
        restart = [b for b, e in enumerate(step) if e is not None and e[1] & RESTART]
        outs = st.push(chunks, final=final, restart=restart)
        n_out = st.n_out.cpu().tolist()
        codes_out = st.codes_out.cpu()
        for b in range(len(step)):
            assert outs[b].shape[0] == n_out[b] and bool((codes_out[b, n_out[b]:] == -1).all())
        pins = None
        if st.pjt_in_out is not None:
            pin = st.pjt_in_out.cpu()
            for b in range(len(step)):
                assert not bool(pin[b, n_out[b]:].any())
            pins = [pin[b, :n_out[b]].clone() for b in range(len(step))]
        rec.append(([o.cpu() for o in outs], n_out, pins))
    return rec


def _frames(M):
    return (M + 1) // 256 if M >= 384 else 0


def _avail(M):
    return (M - 639) // 256 + 1 if M >= 639 else 0


def _reference(eng, steps, halo=H):
    """The semantics on plain Python lists: per step the windows [B][Ws] (NaN beyond their lengths) and
    lengths assembled here, tokenized by eng.tokenize_slots, and the emitted slices.  Also every finished
    utterance as (slot, samples, [its emitted code pieces], [its x_pjt_in pieces])."""
    Ws = -(-(P + 256 * (2 * halo + 2) + 638) // 256) * 256
    samples = [[] for _ in range(B)]
    C, closed = [0] * B, [False] * B
    pieces = [([], []) for _ in range(B)]
    rec, done = [], []
    for step in steps:
        win = np.full((B, Ws), np.nan, dtype=np.float32)
        lens, cut = [0] * B, [(0, 0)] * B
        for b, e in enumerate(step):
            new, flags = (np.zeros(0, np.float32), 0) if e is None else e
            if flags & RESTART:
                samples[b], C[b], closed[b], pieces[b] = [], 0, False, ([], [])
            if not closed[b]:
                samples[b].extend(new.tolist())
            M = len(samples[b])
            a = max(0, C[b] - halo - 2)
            c_new = _frames(M) if flags & FINAL else max(C[b], _avail(M) - halo)
            if c_new > C[b]:
                lens[b] = M - 256 * a
                assert lens[b] <= Ws
                win[b, :lens[b]] = samples[b][256 * a:]
            cut[b] = (C[b] - a, c_new - a)
            C[b] = c_new
            if flags & FINAL and not closed[b]:
                closed[b] = True
                done.append((b, np.asarray(samples[b], np.float32), pieces[b]))
        codes, pin = eng.tokenize_slots(torch.from_numpy(win), lens, want_pjt_in=True)
        codes, pin = codes.cpu(), pin.cpu()
        out = [(codes[b, lo:hi].clone(), pin[b, lo:hi].clone()) for b, (lo, hi) in enumerate(cut)]
        for b, (c, p) in enumerate(out):
            pieces[b][0].append(c)
            pieces[b][1].append(p)
        rec.append(out)
    return rec, done


@pytest.fixture(scope="module")
def runs(engines):
    """Per codebook count: the schedule, the eager stream's outputs and the reference's, computed once."""
    from distilcodec_nabeel_amd.streaming import AudioStream

    cache = {}

    def get(R):
        if R not in cache:
            eng = engines(R)
            steps = _steps(_main_slots())
            st = AudioStream(eng, B, P, H, want_pjt_in=True)
            assert (st.window_samples, st.window_frames, st.out_frames) == (WS, WF, K)
            got = _drive(st, steps)
            want, done = _reference(eng, steps)
            cache[R] = {"steps": steps, "got": got, "want": want, "done": done, "slots": [st.slot(b) for b in range(B)]}
        return cache[R]

    yield get
    cache.clear()


@pytest.mark.parametrize("R", [1, 2])
def test_every_step_equals_the_reference_windows(runs, R):
    r = runs(R)
    assert len(r["steps"]) >= 50
    emitted = 0
    for i, ((outs, n_out, pins), want) in enumerate(zip(r["got"], r["want"])):
        for b in range(B):
            c, p = want[b]
            assert n_out[b] == c.shape[0], (i, b)
            assert torch.equal(outs[b], c), (i, b, "codes")
            assert torch.equal(pins[b], p), (i, b, "x_pjt_in")
            emitted += n_out[b]
    assert emitted == sum(_frames(len(x)) for _, x, _ in r["done"])
    assert r["slots"][0] == (72000, _frames(72000), True) and r["slots"][1] == (20000, _frames(20000), True)
    assert r["slots"][2] == (30000, _frames(30000), True)


@pytest.mark.parametrize("R", [1, 2])
def test_graph_replay_equals_eager(engines, runs, R):
    from distilcodec_nabeel_amd.streaming import AudioStream

    r = runs(R)
    st = AudioStream(engines(R), B, P, H, graph=True, want_pjt_in=True)
    assert st.graph is not None
    got = _drive(st, r["steps"])
    for i, ((outs, n_out, pins), (eo, en, ep)) in enumerate(zip(got, r["got"])):
        assert n_out == en, i
        for b in range(B):
            assert torch.equal(outs[b], eo[b]) and torch.equal(pins[b], ep[b]), (i, b)


def test_slots_do_not_depend_on_their_neighbours(engines, runs):
    """Slot 0's schedule with other neighbours (idle, and another utterance on another schedule)."""
    from distilcodec_nabeel_amd.streaming import AudioStream

    r = runs(1)
    s0 = _main_slots()[0]
    other = [s0, {}, _pushes(_utterance(77, 9000) * 40.0, [1000, 2048, 3], 1)]
    steps = _steps(other)[:len(r["steps"])]
    got = _drive(AudioStream(engines(1), B, P, H, want_pjt_in=True), steps)
    for i, (outs, n_out, pins) in enumerate(got):
        assert torch.equal(outs[0], r["got"][i][0][0]) and torch.equal(pins[0], r["got"][i][2][0]), i


@pytest.mark.parametrize("R", [1, 2])
def test_utterances_equal_the_full_clip(engines, runs, R):
    """The concatenated codes of every finished utterance: the full clip's length, and the full clip's
    codes and x_pjt_in on every frame."""
    eng, r = engines(R), runs(R)
    assert sorted(len(x) for _, x, _ in r["done"]) == [5000, 20000, 30000, 72000]
    for b, x, (cp, pp) in r["done"]:
        codes, pin = torch.cat(cp), torch.cat(pp)
        full_c, _, full_p, _ = eng.tokenize_ragged([x], want_pjt_in=True)
        full_c, full_p = full_c.cpu(), full_p.cpu()
        assert codes.shape == full_c.shape and codes.shape[0] == _frames(len(x))
        rel = float((pin - full_p).abs().max() / full_p.abs().max())
        print(f"\nR={R} slot {b}, {len(x)} samples: x_pjt_in max rel diff {rel:.3e}, "
              f"{int((codes != full_c).sum())} of {codes.numel()} codes differ")
        assert torch.equal(codes, full_c), (b, len(x))
        assert torch.equal(pin, full_p), (b, len(x), rel)


def test_short_halo_differs(engines, runs):
    """A halo of 8 frames, well below the encoder's receptive field of 60: the long utterance's x_pjt_in
    is no longer the full clip's, so the comparison above can fail."""
    from distilcodec_nabeel_amd.streaming import AudioStream

    eng = engines(1)
    x = _utterance(20, 72000)
    steps = _steps([_pushes(x, [P], 0), {}, {}])
    got = _drive(AudioStream(eng, B, P, 8, want_pjt_in=True), steps)
    codes, pin = torch.cat([g[0][0] for g in got]), torch.cat([g[2][0] for g in got])
    _, _, full_p, _ = eng.tokenize_ragged([x], want_pjt_in=True)
    assert codes.shape[0] == _frames(72000) == pin.shape[0]
    rel = float((pin - full_p.cpu()).abs().max() / full_p.abs().max())
    print(f"\nhalo 8: x_pjt_in max rel diff {rel:.3e}")
    assert rel > 1e-6


def _counters(state):
    return state[:4 * 3 * B].view(torch.int32).cpu().tolist()


def test_refused_steps_change_nothing(engines):
    """f32 mode, split-K and a short workspace are refused before any launch: the counters and the next
    step's outputs are those of a stream that never saw the refused steps."""
    from distilcodec_nabeel_amd import _native

    eng = engines(1)
    x = torch.from_numpy(_utterance(31, 3 * P * B)).cuda().view(3, B, P)
    ws = torch.empty(eng.audio_stream_workspace_size(B, P, H) + (160 << 20), dtype=torch.uint8, device="cuda")

    def buffers():
        return (torch.zeros(B, dtype=torch.int32, device="cuda"), torch.full((B, K), 7777, dtype=torch.int32, device="cuda"),
                torch.zeros(B, dtype=torch.int32, device="cuda"))

    n_new = torch.tensor([P, 700, P], dtype=torch.int32, device="cuda")
    flags_fin = torch.tensor([FINAL, 0, FINAL], dtype=torch.int32, device="cuda")
    results = []
    for refuse in (False, True):
        state = eng.audio_stream_state(B, P, H)
        flags, codes_out, n_out = buffers()
        eng.audio_stream_step(state, B, P, H, x[0], n_new, flags, codes_out, n_out, ws=ws)
        if refuse:
            before = _counters(state)
            junk = torch.full_like(codes_out, 4242)
            eng.set_gemm("f32")
            try:
                with pytest.raises(ValueError, match="DCX_GEMM_X6 or DCX_GEMM_BF16"):
                    eng.audio_stream_step(state, B, P, H, x[1], n_new, flags, junk, n_out, ws=ws)
            finally:
                eng.set_gemm("x6")
            eng.set_split_k(4)
            try:
                with pytest.raises(_native.NativeError, match="split-K") as e:
                    eng.audio_stream_step(state, B, P, H, x[1], n_new, flags, junk, n_out, ws=ws)
                assert e.value.status == _native.DCX_ERR_STATE
            finally:
                eng.set_split_k(0)
            with pytest.raises(_native.NativeError, match="workspace too small") as e:
                eng.audio_stream_step(state, B, P, H, x[1], n_new, flags, junk, n_out, ws=ws[:1 << 16])
            assert e.value.status == _native.DCX_ERR_WORKSPACE
            with pytest.raises(ValueError, match="state buffer"):
                eng.audio_stream_step(state[:-256], B, P, H, x[1], n_new, flags, junk, n_out, ws=ws)
            torch.cuda.synchronize()
            assert _counters(state) == before and bool((junk == 4242).all())
        eng.audio_stream_step(state, B, P, H, x[2], n_new, flags_fin, codes_out, n_out, ws=ws)
        results.append((codes_out.cpu(), n_out.cpu().tolist(), _counters(state)))
    assert torch.equal(results[0][0], results[1][0]) and results[0][1:] == results[1][1:]
    assert results[0][1] == [_frames(2 * P), 0, _frames(2 * P)]
    assert results[0][2] == [2 * P, 1400, 2 * P, _frames(2 * P), 0, _frames(2 * P), 1, 0, 1]


def test_python_errors_come_before_any_upload(engines):
    from distilcodec_nabeel_amd.streaming import AudioStream

    st = AudioStream(engines(1), B, P, H)
    st.push([np.zeros(500, np.float32), None, np.zeros(200, np.float32)], final=[0])
    turn, slots = st._turn, [st.slot(b) for b in range(B)]
    assert slots == [(500, 1, True), (0, 0, False), (200, 0, False)]
    with pytest.raises(ValueError, match="exceeds push_samples"):
        st.push([None, np.zeros(P + 1, np.float32), None])
    with pytest.raises(ValueError, match="fewer than"):
        st.push([None, None, np.zeros(183, np.float32)], final=[2])  # 383 samples in all
    with pytest.raises(ValueError, match="fewer than"):
        st.push([None, None, None], final=[1])  # an empty utterance
    with pytest.raises(RuntimeError, match="closed"):
        st.push([np.zeros(10, np.float32), None, None])
    with pytest.raises(ValueError, match="one entry per slot"):
        st.push([None, None])
    with pytest.raises(ValueError, match="outside"):
        st.push([None, None, None], final=[3])
    assert st._turn == turn and [st.slot(b) for b in range(B)] == slots
    outs = st.push([np.zeros(400, np.float32), None, np.zeros(184, np.float32)], final=[0, 2], restart=[0])
    assert [o.shape[0] for o in outs] == [1, 0, 1]
    assert [st.slot(b) for b in range(B)] == [(400, 1, True), (0, 0, False), (384, 1, True)]
    with pytest.raises(ValueError):
        AudioStream(engines(1), 0, P, H)


def test_token_surface(runs):
    """DistilCodec.audio_stream: push_tokens yields the LLM token ids `encode` yields (codes offset by
    token_id_offset), and they round-trip through token_stream().push_tokens to audio of the right length."""
    import distilcodec_nabeel_amd as pkg
    from distilcodec_nabeel_amd import DistilCodec

    assert pkg.AudioStream is not None and "AudioStream" in pkg.__all__
    cfg = RV.rvq_cfg(4096, 256, 1)
    cfg["token_id_offset"] = 151665
    codec = DistilCodec(cfg)
    codec.move_to_cuda()
    st = codec.audio_stream(B, P)
    assert st.graph is not None and st.halo_frames == H and st.token_id_offset == 151665 and st.out_frames == K
    ts = codec.token_stream(B, K)
    x = _utterance(55, 9000)
    ids_all, wav = [], []
    at = 0
    while at < len(x):
        n = min(P, len(x) - at)
        fin = [1] if at + n == len(x) else []
        ids = st.push_tokens([None, x[at:at + n], None], final=fin)
        assert ids[0] == [] and ids[2] == []
        ids_all += ids[1]
        wav.append(ts.push_tokens([None, ids[1], None], final=fin)[1])
        at += n
    frames = _frames(9000)
    assert len(ids_all) == frames and all(151665 <= t < 151665 + 4096 for t in ids_all)
    # `encode` on the packed path (every clip alone); its list is trimmed to the clip's whole hops
    ret = codec.encode([[x, 24000]], raw_audio=True, codes_only=True, ragged=True)[0]
    want = [t["absolute_token_id"] for t in ret.codes_list[0]]
    assert frames - 1 <= len(want) <= frames and ids_all[:len(want)] == want
    assert sum(w.shape[-1] for w in wav) == 256 * frames
    assert st.push_tokens([None, x[:400], None], final=[1], restart=[1], add_token_offset=False)[1] == \
        [t - 151665 for t in st.push_tokens([None, x[:400], None], final=[1], restart=[1])[1]]
