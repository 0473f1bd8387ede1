"""The ragged-batch planner (dcx_ragged_plan_size / dcx_ragged_plan) and the host-side validation
of dcx_tokenize_ragged / dcx_ragged_workspace_size.  Host-only calls, so this runs without a GPU.

The plan table is opaque to callers; these tests read it through its documented invariants only:
its totals, its size, and that every per-clip quantity is a prefix sum (so the table of a permuted
clip list is the permuted table, checked on the differences of each prefix array)."""
import ctypes

import numpy as np
import pytest
import torch

LENGTHS = [384, 400, 700, 1800, 4300, 8500, 30000, 240000]


@pytest.fixture()
def handle(cfg):
    from distilcodec_nabeel_amd import _native

    L = _native.lib()
    c = _native.config_from_dict(cfg)
    h = ctypes.c_void_p()
    assert L.dcx_create(ctypes.byref(c), ctypes.byref(h)) == 0
    yield L, h
    L.dcx_destroy(h)


def _plan(L, h, lengths, words=None):
    n = np.asarray(lengths, dtype=np.int64)
    B = len(lengths)
    size = int(L.dcx_ragged_plan_size(B))
    words = size if words is None else words
    plan = np.full(max(words, 1), -7, dtype=np.int32)
    ts, tf = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = L.dcx_ragged_plan(h, n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), B, plan.ctypes.data_as(ctypes.c_void_p),
                           words, ctypes.byref(ts), ctypes.byref(tf))
    return rc, plan, ts.value, tf.value


def _prefix_arrays(plan, B):
    """The table's prefix arrays: every run of B + 1 ints after the header that starts at 0 and
    increases strictly (sample / frame offsets and the kernels' per-clip work-item prefixes)."""
    size = plan.shape[0]
    n = B + 1
    head = size - 5 * n
    assert head >= 0 and (size - head) % n == 0
    arrs = plan[head:].reshape(-1, n)
    for a in arrs:
        assert a[0] == 0 and (np.diff(a) > 0).all()
    return arrs


def test_plan_frames_and_totals(handle):
    from oracle import reference_cpu as R

    L, h = handle
    rc, plan, ts, tf = _plan(L, h, LENGTHS)
    assert rc == 0, L.dcx_last_error(h)
    frames = [int(L.dcx_num_frames(h, n + 1)) for n in LENGTHS]
    for n, t in zip(LENGTHS, frames):
        assert t == R.log_mel(torch.zeros(1, n + 1)).shape[-1], n
    assert ts == sum(LENGTHS) and tf == sum(frames)
    arrs = _prefix_arrays(plan, len(LENGTHS))
    per_clip = [np.diff(a).tolist() for a in arrs]
    assert LENGTHS in per_clip  # the sample offsets
    assert frames in per_clip  # the frame offsets
    assert (plan != -7).all()  # every word of the table is written


def test_plan_of_a_permutation_is_the_permuted_plan(handle):
    L, h = handle
    perm = [5, 0, 7, 2, 1, 6, 3, 4]
    rc0, p0, ts0, tf0 = _plan(L, h, LENGTHS)
    rc1, p1, ts1, tf1 = _plan(L, h, [LENGTHS[i] for i in perm])
    assert rc0 == 0 and rc1 == 0
    assert (ts0, tf0) == (ts1, tf1)
    B = len(LENGTHS)
    a0, a1 = _prefix_arrays(p0, B), _prefix_arrays(p1, B)
    assert a0.shape == a1.shape
    for x, y in zip(a0, a1):
        assert np.array_equal(np.diff(x)[perm], np.diff(y))
    head = p0.shape[0] - a0.size
    assert np.array_equal(p0[:head], p1[:head])  # the totals do not depend on the order


def _ceil(a, d):
    return [-(-x // d) for x in a]


def _check_plan_at_scale(L, h, lengths, frames, rw):
    """The table of a large batch: the five prefix arrays' per-clip differences are the clip's samples,
    T, ceil(T / 16), ceil(T / 4) and ceil(T / rw) (as a multiset: at rw = 4 two of them coincide), the
    totals are their last entries, and the header holds exactly those totals, the clip count and rw."""
    B = len(lengths)
    rc, plan, ts, tf = _plan(L, h, lengths)
    assert rc == 0, L.dcx_last_error(h)
    assert (plan != -7).all()
    assert ts == sum(lengths) and tf == sum(frames)
    arrs = _prefix_arrays(plan, B)
    assert arrs.shape == (5, B + 1)
    want = [list(lengths), list(frames), _ceil(frames, 16), _ceil(frames, 4), _ceil(frames, rw)]
    assert sorted(np.diff(a).tolist() for a in arrs) == sorted(want)
    totals = sorted(int(a[-1]) for a in arrs)
    assert totals == sorted(sum(w) for w in want)
    head = plan[: plan.shape[0] - arrs.size]
    assert sorted(head[1:].tolist()) == sorted(totals + [B, rw]), head  # head[0]: the table's tag
    return plan


@pytest.mark.parametrize("case", ["t16", "rw4", "rw8", "rw16", "rw32"])
def test_plan_at_scale(handle, case):
    """One total in each row class of launch_dwconv_ln_ragged, the batches of tests/test_gpu_ragged_scale.py:
    run width 4 / 8 / 16 / 32 from 8192 * {1, 2, 4, 8} rows (4 below: the tiled forms do not read it)."""
    from _parity import RAGGED_CASES, RAGGED_LONG_T, RAGGED_SHORT_T, ragged_case_order, ragged_pool_lengths

    L, h = handle
    pool_n, pool_t = ragged_pool_lengths(), RAGGED_SHORT_T + [RAGGED_LONG_T]
    assert [int(L.dcx_num_frames(h, n + 1)) for n in pool_n] == pool_t
    assert sum(RAGGED_SHORT_T) == 376 and sum(_ceil(RAGGED_SHORT_T, 16)) == 33
    k_short, k_long, total, form = RAGGED_CASES[case]
    order = ragged_case_order(case)
    assert len(order) == 19 * k_short + k_long
    lengths, frames = [pool_n[i] for i in order], [pool_t[i] for i in order]
    assert sum(frames) == total
    rw = 32 if total >= 65536 else 16 if total >= 32768 else 8 if total >= 16384 else 4
    assert rw == (form or 4) and (form == 0) == (total < 8192)
    if form == 0:
        assert sum(_ceil(frames, 16)) >= 512  # the 16-row tiles, not the 4-row ones
    # long and short clips alternate: no stretch of the batch is all of one kind
    if k_long:
        is_long = np.asarray(frames) == RAGGED_LONG_T
        assert 0 < is_long[: len(frames) // 2].sum() < k_long
    _check_plan_at_scale(L, h, lengths, frames, rw)


@pytest.mark.parametrize("case,total,rw", [("t16", 8191, 4), ("t16", 8192, 4), ("rw4", 16383, 4), ("rw4", 16384, 8),
                                           ("rw8", 32767, 8), ("rw8", 32768, 16), ("rw16", 65535, 16),
                                           ("rw16", 65536, 32)])
def test_plan_at_class_boundaries(handle, case, total, rw):
    """The last total of a row class and the first of the next, reached by adding 1-frame clips
    (384 samples) to one of the compositions above."""
    from _parity import RAGGED_CASES, RAGGED_LONG_T, RAGGED_SHORT_T, ragged_case_order, ragged_pool_lengths

    L, h = handle
    pool_n, pool_t = ragged_pool_lengths(), RAGGED_SHORT_T + [RAGGED_LONG_T]
    order = ragged_case_order(case)
    extra = total - RAGGED_CASES[case][2]
    assert extra > 0
    lengths = [pool_n[i] for i in order] + [384] * extra
    frames = [pool_t[i] for i in order] + [1] * extra
    assert sum(frames) == total
    plan = _check_plan_at_scale(L, h, lengths, frames, rw)
    assert int(L.dcx_ragged_workspace_size(h, len(lengths), total)) > 0
    assert plan.shape[0] == int(L.dcx_ragged_plan_size(len(lengths)))


def test_plan_validation(handle):
    from distilcodec_nabeel_amd import _native

    L, h = handle
    rc, *_ = _plan(L, h, [5000, 383, 9000])
    assert rc == _native.DCX_ERR_INVALID_ARG
    msg = L.dcx_last_error(h).decode()
    assert "clip 1" in msg and "383" in msg, msg
    assert _plan(L, h, [384])[0] == 0  # the shortest clip the reflect pad accepts: one frame
    assert _plan(L, h, [384])[3] == 1
    # batch = 0
    assert L.dcx_ragged_plan_size(0) == 0
    buf = np.zeros(64, np.int32)
    ts, tf = ctypes.c_int64(), ctypes.c_int64()
    n = np.zeros(1, np.int64)
    assert L.dcx_ragged_plan(h, n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 0, buf.ctypes.data_as(ctypes.c_void_p),
                             64, ctypes.byref(ts), ctypes.byref(tf)) == _native.DCX_ERR_INVALID_ARG
    # a table one word short
    size = int(L.dcx_ragged_plan_size(3))
    assert size > 0
    assert _plan(L, h, [5000, 6000, 7000], words=size - 1)[0] == _native.DCX_ERR_INVALID_ARG
    assert _plan(L, h, [5000, 6000, 7000], words=size)[0] == 0
    # totals beyond what the kernels index (2^20 frames: 2^28 samples and more)
    rc, *_ = _plan(L, h, [1 << 27, 1 << 27, 1 << 27])
    assert rc == _native.DCX_ERR_INVALID_ARG and "clip 2" in L.dcx_last_error(h).decode()


def test_tokenize_before_finalize_and_workspace_size(handle):
    from distilcodec_nabeel_amd import _native

    L, h = handle
    assert L.dcx_tokenize_ragged(h, None, None, None, 1, 400, 1, None, None, None, None, 0, None) == _native.DCX_ERR_STATE
    w1 = int(L.dcx_ragged_workspace_size(h, 6, 176))
    w2 = int(L.dcx_ragged_workspace_size(h, 24, 8684))
    assert 0 < w1 < w2
    assert L.dcx_ragged_workspace_size(h, 0, 176) == 0
    assert L.dcx_ragged_workspace_size(h, 6, 5) == 0  # fewer frames than clips
