"""The token stream's slot arithmetic (dcx_stream_plan_step: the function the plan kernel runs per slot,
dcx_stream_plan.h) and the host-side validation of dcx_stream_state_size / dcx_stream_reset /
dcx_stream_decode_step.  Host-only calls, so this runs without a GPU.

The semantics are those of include/distilcodec_amd.h ("Token streams"); `_model` below restates them
in Python, independently of the library, and every step is compared with it."""
import ctypes
import random

import pytest

FINAL, RESTART = 1, 2
HALOS = [0, 1, 4, 21]
PUSHES = [1, 3, 8, 24, 93]


@pytest.fixture(scope="module")
def L():
    from distilcodec_nabeel_amd import _native

    return _native.lib()


def _step(L, h, P, slot, n, flags):
    """One library step on slot = [T, E, closed] (updated in place) -> (len, skip, take)."""
    v = [ctypes.c_int32(x) for x in slot] + [ctypes.c_int32(-99) for _ in range(3)]
    rc = L.dcx_stream_plan_step(h, P, ctypes.byref(v[0]), ctypes.byref(v[1]), ctypes.byref(v[2]), n, flags,
                                ctypes.byref(v[3]), ctypes.byref(v[4]), ctypes.byref(v[5]))
    assert rc == 0
    slot[:] = [x.value for x in v[:3]]
    return tuple(x.value for x in v[3:])


def _model(h, P, slot, n, flags):
    T, E, closed = slot
    if flags & RESTART:
        T = E = closed = 0
    n = min(max(n, 0), P)
    if closed:
        n = 0
    T += n
    g0 = max(0, E - h)
    f_new = T if flags & FINAL else max(E, T - h)
    out = (T - g0, E - g0, f_new - E)
    slot[:] = [T, E + out[2], 1 if flags & FINAL else closed]
    return out


def _run(L, h, P, counts):
    """A schedule of per-step counts, FINAL on the last step, checked step by step against the four
    properties; returns (largest len, largest take without FINAL, the FINAL step's take)."""
    W = P + 2 * h
    slot, ref = [0, 0, 0], [0, 0, 0]
    emitted = 0
    max_len = max_take = 0
    for i, n in enumerate(counts):
        fin = i == len(counts) - 1
        E0 = slot[1]
        ln, skip, take = _step(L, h, P, slot, n, FINAL if fin else 0)
        assert (ln, skip, take) == _model(h, P, ref, n, FINAL if fin else 0) and slot == ref
        T = slot[0]
        g0 = max(0, E0 - h)
        assert T == sum(counts[:i + 1])
        assert 0 <= ln <= W and ln == T - g0  # the window is codes [g0, T)
        assert 0 <= take <= (P + h if fin else P)
        assert skip == E0 - g0 and skip + take <= ln
        # the emitted intervals tile [0, T) exactly once: each starts where the last one ended
        assert E0 == emitted
        emitted += take
        assert slot[1] == emitted <= T
        # every emitted frame has h window frames on each side, but for the true start and the true end
        if take:
            assert g0 == 0 or skip >= h
            assert fin or ln - (skip + take) >= h
        max_len = max(max_len, ln)
        if not fin:
            max_take = max(max_take, take)
    assert emitted == slot[0] and slot[2] == 1
    return max_len, max_take, take


@pytest.mark.parametrize("h", HALOS)
@pytest.mark.parametrize("P", PUSHES)
def test_random_schedules(L, h, P):
    rng = random.Random(1000 * h + P)
    for _ in range(200):
        steps = rng.randint(1, 12)
        kind = rng.random()
        counts = [rng.randint(0, P) if kind < 0.6 else rng.choice([0, P]) if kind < 0.8 else rng.choice([0, 1, P])
                  for _ in range(steps)]
        _run(L, h, P, counts)


@pytest.mark.parametrize("h", HALOS)
@pytest.mark.parametrize("P", PUSHES)
def test_bounds_are_reached(L, h, P):
    """Full pushes until the window slides: len reaches P + 2 h, take P, and P + h at FINAL, so the
    state buffer, the workspace and wav_out are not oversized."""
    steps = -(-2 * h // P) + 3
    max_len, max_take, final_take = _run(L, h, P, [P] * steps)
    assert max_len == P + 2 * h
    assert max_take == P
    assert final_take == P + h


def test_restart_after_final_starts_from_zero(L):
    h, P = 4, 8
    slot = [0, 0, 0]
    _step(L, h, P, slot, 8, 0)
    _step(L, h, P, slot, 5, FINAL)
    assert slot == [13, 13, 1]
    ln, skip, take = _step(L, h, P, slot, 6, RESTART)
    assert slot == [6, 2, 0] and (ln, skip, take) == (6, 0, 2)
    # RESTART and FINAL in one step: an utterance that starts and ends with this push
    assert _step(L, h, P, slot, 3, RESTART | FINAL) == (3, 0, 3) and slot == [3, 3, 1]


def test_codes_to_a_closed_slot_change_nothing(L):
    h, P = 4, 8
    slot = [0, 0, 0]
    _step(L, h, P, slot, 8, 0)
    _step(L, h, P, slot, 2, FINAL)
    assert slot == [10, 10, 1]
    for flags in (0, FINAL):
        ln, skip, take = _step(L, h, P, slot, 7, flags)
        assert slot == [10, 10, 1] and take == 0 and ln == skip == h


def test_counts_are_clamped(L):
    h, P = 4, 8
    slot = [0, 0, 0]
    assert _step(L, h, P, slot, 1000, 0) == (8, 0, 4) and slot == [8, 4, 0]
    assert _step(L, h, P, slot, -5, 0) == (8, 4, 0) and slot == [8, 4, 0]
    # counters that no step can leave (an unreset state buffer) start the slot over
    bad = [3, 9, 1]
    assert _step(L, h, P, bad, 2, 0) == (2, 0, 0) and bad == [2, 0, 0]


def test_plan_step_argument_errors(L):
    from distilcodec_nabeel_amd import _native

    t, e, c = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    args = (ctypes.byref(t), ctypes.byref(e), ctypes.byref(c), 1, 0, None, None, None)
    assert L.dcx_stream_plan_step(4, 8, *args) == 0 and t.value == 1  # the outputs are optional
    assert L.dcx_stream_plan_step(-1, 8, *args) == _native.DCX_ERR_INVALID_ARG
    assert L.dcx_stream_plan_step(4, 0, *args) == _native.DCX_ERR_INVALID_ARG
    assert L.dcx_stream_plan_step(4, 8, None, ctypes.byref(e), ctypes.byref(c), 1, 0, None, None, None) == \
        _native.DCX_ERR_INVALID_ARG


def test_state_size_and_argument_errors(L, cfg):
    from distilcodec_nabeel_amd import _native

    c = _native.config_from_dict(cfg)
    h = ctypes.c_void_p()
    assert L.dcx_create(ctypes.byref(c), ctypes.byref(h)) == 0
    try:
        size = int(L.dcx_stream_state_size(h, 3, 8, 21))
        # the ring and the window of codes, [3][50] each, and the window's waveform [3][50 * 256]
        floor = 2 * 3 * 50 * 4 + 3 * 50 * 256 * 4
        assert floor < size < floor + 4096
        assert int(L.dcx_stream_state_size(h, 6, 8, 21)) > size
        assert int(L.dcx_stream_state_size(h, 1, 1, 0)) > 0
        for bad in ((0, 8, 21), (-1, 8, 21), (3, 0, 21), (3, 8, -1), (1 << 16, 8, 21), (3, (1 << 16) + 1, 21)):
            assert L.dcx_stream_state_size(h, *bad) == 0, bad
        assert L.dcx_stream_state_size(None, 3, 8, 21) == 0
        # two codebooks per frame: the ring and the window double
        assert L.dcx_set_num_codebooks(h, 2) == 0
        assert int(L.dcx_stream_state_size(h, 3, 8, 21)) >= size + 2 * 3 * 50 * 4 - 512
        # the entry points refuse a bad geometry and a null or short state buffer before any device call
        buf = (ctypes.c_char * (size + 16))()
        state = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
        step_tail = (None, None, None, None, None, None, None, 0, None)
        for bad in ((0, 8, 21), (3, 0, 21), (3, 8, -1)):
            assert L.dcx_stream_reset(h, state, size, *bad, None) == _native.DCX_ERR_INVALID_ARG, bad
            assert L.dcx_stream_decode_step(h, state, size, *bad, *step_tail) == _native.DCX_ERR_INVALID_ARG, bad
        assert L.dcx_stream_reset(h, None, size, 3, 8, 21, None) == _native.DCX_ERR_INVALID_ARG
        assert L.dcx_stream_reset(h, state, 64, 3, 8, 21, None) == _native.DCX_ERR_INVALID_ARG
        assert b"dcx_stream_state_size" in L.dcx_last_error(h)
        assert L.dcx_stream_decode_step(h, state, 64, 3, 8, 21, *step_tail) == _native.DCX_ERR_INVALID_ARG
        assert L.dcx_stream_decode_step(h, state, 2 * size, 3, 8, 21, *step_tail) == _native.DCX_ERR_INVALID_ARG  # null buffers
        assert L.dcx_stream_reset(None, state, size, 3, 8, 21, None) == _native.DCX_ERR_INVALID_ARG
    finally:
        L.dcx_destroy(h)
