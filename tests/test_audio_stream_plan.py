"""The audio stream's slot arithmetic (dcx_stream_encode_plan_step: the function the plan kernel runs per
slot, dcx_stream_plan.h) and the host-side geometry of dcx_stream_encode_state_size /
dcx_stream_encode_geometry.  Host-only calls, so this runs without a GPU.

The semantics are those of include/distilcodec_amd.h ("Audio streams"); `_model` below restates them in
Python, independently of the library, and every step is compared with it.  The bounds the header
states are each held on random schedules and reached by a constructed one:
  len <= P + 256 (2 h + 2) + 638;  take <= ceil(P / 256) without FINAL;  take <= h + (P + 639) // 256 at
  FINAL;  M - 256 C <= 256 h + 638 after a step."""
import ctypes
import random

import pytest

FINAL, RESTART = 1, 2
HALOS = [0, 1, 8, 60]
PUSHES = [1, 100, 256, 700, 2048, 24000]


@pytest.fixture(scope="module")
def lib_handle(cfg):
    from distilcodec_nabeel_amd import _native

    L = _native.lib()
    c = _native.config_from_dict(cfg)
    h = ctypes.c_void_p()
    assert L.dcx_create(ctypes.byref(c), ctypes.byref(h)) == 0
    yield L, h
    L.dcx_destroy(h)


def _frames(M):
    """dcx_num_frames(M + 1) of a clip of M raw samples; none while the reflect pad does not fit."""
    return (M + 1) // 256 if M >= 384 else 0


def _avail(M):
    return (M - 639) // 256 + 1 if M >= 639 else 0


def _step(lh, h, P, slot, n, flags):
    """One library step on slot = [M, C, closed] (updated in place) -> (len, start, skip, take)."""
    L, handle = lh
    v = [ctypes.c_int32(x) for x in slot] + [ctypes.c_int32(-99) for _ in range(4)]
    rc = L.dcx_stream_encode_plan_step(handle, h, P, ctypes.byref(v[0]), ctypes.byref(v[1]), ctypes.byref(v[2]), n, flags,
                                       *[ctypes.byref(x) for x in v[3:]])
    assert rc == 0
    slot[:] = [x.value for x in v[:3]]
    return tuple(x.value for x in v[3:])


def _model(h, P, slot, n, flags):
    M, C, closed = slot
    if flags & RESTART:
        M = C = closed = 0
    n = min(max(n, 0), P)
    if closed:
        n = 0
    M += n
    a = max(0, C - h - 2)
    c_new = _frames(M) if flags & FINAL else max(C, _avail(M) - h)
    take = c_new - C
    out = (M - 256 * a if take > 0 else 0, 256 * a, C - a, take)
    slot[:] = [M, c_new, 1 if flags & FINAL else closed]
    return out


def _bounds(h, P):
    return {"len": P + 256 * (2 * h + 2) + 638, "take": -(-P // 256), "final": h + (P + 639) // 256, "lag": 256 * h + 638}


def _run(lh, h, P, counts, final=True):
    """A schedule of per-step counts (FINAL on the last step), checked step by step against the model and
    the properties; returns the largest (len, take without FINAL, FINAL take, M - 256 C after a step)."""
    bd = _bounds(h, P)
    slot, ref = [0, 0, 0], [0, 0, 0]
    emitted = 0
    top = {"len": 0, "take": 0, "final": 0, "lag": 0}
    for i, n in enumerate(counts):
        fin = final and i == len(counts) - 1
        C0 = slot[1]
        ln, start, skip, take = _step(lh, h, P, slot, n, FINAL if fin else 0)
        assert (ln, start, skip, take) == _model(h, P, ref, n, FINAL if fin else 0) and slot == ref
        M, C, closed = slot
        assert take >= 0 and C == C0 + take and start % 256 == 0 and skip == C0 - start // 256 >= 0
        assert C0 == emitted  # the emitted intervals [C0, C0 + take) tile the frames in order
        emitted += take
        if take:
            assert start + ln == M and 0 < ln <= bd["len"]
            assert skip + take <= _frames(ln)  # the window tokenized alone holds every emitted frame
            assert skip >= min(C0, h + 2)  # an emitted frame has its halo (and the margin) before it
        else:
            assert ln == 0
        assert M - 256 * C <= bd["lag"]
        assert take <= (bd["final"] if fin else bd["take"])
        if not fin:  # frames emitted without FINAL touch no reflected sample, with h such frames after them
            assert C <= max(0, _avail(M) - h) or take == 0
        top["len"] = max(top["len"], ln)
        top["final" if fin else "take"] = max(top["final" if fin else "take"], take)
        top["lag"] = max(top["lag"], M - 256 * C)
    if final:
        assert slot[2] == 1 and emitted == _frames(slot[0])  # [0, dcx_num_frames(M + 1)) exactly once
    return top


def _chunks(total, P):
    return [P] * (total // P) + ([total % P] if total % P else [])


@pytest.mark.parametrize("h", HALOS)
@pytest.mark.parametrize("P", PUSHES)
def test_random_schedules(lib_handle, h, P):
    rng = random.Random(1000 * h + P)
    for _ in range(12):
        steps = rng.randrange(1, 60)
        counts = [rng.choice([0, 1, P, rng.randrange(P + 1), rng.randrange(P + 1)]) for _ in range(steps)]
        if sum(counts) < 384:
            counts += _chunks(384, P)
        _run(lib_handle, h, P, counts)
        _run(lib_handle, h, P, counts + [0])  # FINAL on an empty push


@pytest.mark.parametrize("h", HALOS)
@pytest.mark.parametrize("P", PUSHES)
def test_bounds_are_reached(lib_handle, h, P):
    """M = 638 + 256 q samples (q = 2 h + 2 + 3: avail = q exactly, C = q - h, the window starts at frame
    q - 2 h - 2), then one full push: the longest window, the largest take without and with FINAL, and
    the largest M - 256 C."""
    bd = _bounds(h, P)
    q = 2 * h + 5
    pre = _chunks(638 + 256 * q, P)
    top = _run(lib_handle, h, P, pre + [P], final=False)
    assert top["len"] == bd["len"] and top["take"] == bd["take"] and top["lag"] == bd["lag"]
    top = _run(lib_handle, h, P, pre + [P])
    assert top["final"] == bd["final"] and top["len"] == bd["len"]


@pytest.mark.parametrize("h", HALOS)
@pytest.mark.parametrize("P", PUSHES)
def test_geometry(lib_handle, h, P):
    L, handle = lib_handle
    bd = _bounds(h, P)
    v = [ctypes.c_int64(-1) for _ in range(3)]
    assert L.dcx_stream_encode_geometry(handle, P, h, *[ctypes.byref(x) for x in v]) == 0
    Ws = -(-bd["len"] // 256) * 256
    assert [x.value for x in v] == [Ws, Ws // 256, bd["final"]]
    assert Ws // 256 == L.dcx_num_frames(handle, Ws + 1)
    small = L.dcx_stream_encode_state_size(handle, 3, P, h, 0)
    assert small >= 3 * (12 * 4 + 2 * Ws * 4 + (Ws // 256) * 4) and small % 256 == 0
    assert L.dcx_stream_encode_state_size(handle, 3, P, h, 1) > small


def test_bad_geometry(lib_handle):
    L, handle = lib_handle
    for args in [(0, 2048, 60), (65536, 2048, 60), (3, 0, 60), (3, (1 << 24) + 1, 60), (3, 2048, -1), (3, 2048, 65537),
                 (60000, 1 << 20, 60)]:  # the last: more than 2^31 - 1 window samples in all
        assert L.dcx_stream_encode_state_size(handle, *args, 0) == 0, args
    v = ctypes.c_int64(0)
    assert L.dcx_stream_encode_geometry(handle, 0, 60, ctypes.byref(v), None, None) != 0
    assert L.dcx_stream_encode_geometry(handle, 2048, -1, ctypes.byref(v), None, None) != 0
    s = [ctypes.c_int32(0) for _ in range(3)]
    assert L.dcx_stream_encode_plan_step(handle, -1, 2048, *[ctypes.byref(x) for x in s], 0, 0, None, None, None, None) != 0
    assert L.dcx_stream_encode_plan_step(handle, 60, 0, *[ctypes.byref(x) for x in s], 0, 0, None, None, None, None) != 0
    assert L.dcx_stream_encode_plan_step(handle, 60, 2048, None, None, None, 0, 0, None, None, None, None) != 0


def test_restart_closed_and_short_final(lib_handle):
    h, P = 8, 1000
    slot = [0, 0, 0]
    for _ in range(6):
        _step(lib_handle, h, P, slot, P, 0)
    assert slot == [6000, max(0, _avail(6000) - h), 0]
    ln, start, skip, take = _step(lib_handle, h, P, slot, 500, FINAL)
    assert slot == [6500, _frames(6500), 1] and take == _frames(6500) - max(0, _avail(6000) - h) and start + ln == 6500
    # a closed slot ignores new samples, with or without FINAL, and emits nothing
    for flags in (0, FINAL):
        assert _step(lib_handle, h, P, slot, 700, flags) == (0, 256 * max(0, slot[1] - h - 2), min(slot[1], h + 2), 0)
        assert slot == [6500, _frames(6500), 1]
    # RESTART starts it over with this step's samples; RESTART | FINAL is a whole utterance in one step
    assert _step(lib_handle, h, P, slot, 700, RESTART) == (0, 0, 0, 0) and slot == [700, 0, 0]
    assert _step(lib_handle, h, P, slot, 900, RESTART | FINAL) == (900, 0, 0, 3) and slot == [900, 3, 1]
    # the count is clamped to [0, P]
    slot = [0, 0, 0]
    _step(lib_handle, h, P, slot, -5, 0)
    assert slot == [0, 0, 0]
    _step(lib_handle, h, P, slot, P + 77, 0)
    assert slot == [P, 0, 0]
    # a FINAL on fewer than 384 samples emits nothing and closes; on 384 it emits one frame
    slot = [0, 0, 0]
    assert _step(lib_handle, h, P, slot, 383, FINAL) == (0, 0, 0, 0) and slot == [383, 0, 1]
    slot = [0, 0, 0]
    assert _step(lib_handle, h, P, slot, 384, FINAL) == (384, 0, 0, 1) and slot == [384, 1, 1]
    slot = [0, 0, 0]
    assert _step(lib_handle, h, P, slot, 0, FINAL) == (0, 0, 0, 0) and slot == [0, 0, 1]


@pytest.mark.parametrize("bad", [[-1, 0, 0], [1000, -2, 0], [1000, 4, 0], [5000, 3, 2], [10 ** 6, 5, 0], [300, 1, 1]])
def test_impossible_counters_restart(lib_handle, bad):
    """Counters no step can have left (a state buffer that was never reset) start the slot over."""
    h, P = 8, 1000
    slot, ref = list(bad), [0, 0, 0]
    assert _step(lib_handle, h, P, slot, 600, 0) == _model(h, P, ref, 600, 0) and slot == ref == [600, 0, 0]
