"""Host side of the ragged decode (dcx_generate_ragged / dcx_decode_ragged): the helper that pads and
validates code lists and lengths, and the argument checks the two symbols make before any HIP call.
No GPU: the handle is created and never finalized."""
import ctypes

import numpy as np
import pytest

from distilcodec_nabeel_amd import ragged


# ---------------------------------------------------------------- padding and validation helper
def test_pad_code_lists_pads_with_minus_one():
    codes, lengths = ragged.pad_code_lists([[5, 6, 7], [], [9]])
    assert codes.dtype == np.int32 and lengths.dtype == np.int32
    assert codes.flags["C_CONTIGUOUS"] and lengths.flags["C_CONTIGUOUS"]
    assert lengths.tolist() == [3, 0, 1]
    assert codes.tolist() == [[5, 6, 7], [-1, -1, -1], [9, -1, -1]]


def test_pad_code_lists_all_empty_keeps_one_frame():
    codes, lengths = ragged.pad_code_lists([[], []])
    assert codes.shape == (2, 1) and lengths.tolist() == [0, 0]
    assert (codes == ragged.PAD_CODE).all()


def test_pad_code_lists_rejects_empty_batch_and_wide_codes():
    with pytest.raises(ValueError, match="at least one clip"):
        ragged.pad_code_lists([])
    with pytest.raises(ValueError, match="32 bits"):
        ragged.pad_code_lists([[1 << 40]])


def test_check_lengths_accepts_the_edges():
    out = ragged.check_lengths([0, 40, 17], 3, 40)
    assert out.dtype == np.int32 and out.tolist() == [0, 40, 17]
    assert ragged.check_lengths(np.array([2.0, 3.0]), 2, 3).tolist() == [2, 3]


@pytest.mark.parametrize("lengths, batch, t_max, text", [
    ([], 0, 4, "non-empty"),
    ([[1, 2]], 1, 4, "non-empty 1-D"),
    ([1, 2], 3, 4, "2 lengths for a batch of 3"),
    ([1, -1], 2, 4, "clip 1 has length -1"),
    ([5, 1], 2, 4, "clip 0 has length 5"),
    ([1.5, 1], 2, 4, "integers"),
    ([1], 1, 0, "frames_max"),
])
def test_check_lengths_rejects(lengths, batch, t_max, text):
    with pytest.raises(ValueError, match=text):
        ragged.check_lengths(lengths, batch, t_max)


def test_check_codes_looks_inside_the_lengths_only():
    codes = np.array([[1, 99999, -99999], [3, 4, 5]], dtype=np.int32)
    ragged.check_codes_in_lengths(codes, np.array([1, 3]), 16384)  # the bad entries are padding
    ragged.check_codes_in_lengths(np.array([[-16384, 16383]], dtype=np.int32), np.array([2]), 16384)
    with pytest.raises(IndexError, match=r"clip 0, frame 1"):
        ragged.check_codes_in_lengths(codes, np.array([2, 3]), 16384)
    with pytest.raises(IndexError, match=r"-16385 \(clip 1, frame 2\)"):
        ragged.check_codes_in_lengths(np.array([[1, 2, 3], [3, 4, -16385]], dtype=np.int32), np.array([3, 3]), 16384)


# ---------------------------------------------------------------- the C ABI's argument checks
@pytest.fixture()
def handle(cfg):
    from distilcodec_nabeel_amd import _native

    L = _native.lib()
    c = _native.config_from_dict(cfg)
    h = ctypes.c_void_p()
    assert L.dcx_create(ctypes.byref(c), ctypes.byref(h)) == 0
    yield L, h
    L.dcx_destroy(h)


def _host_buffers():
    """Non-null arguments for a call that must fail before it touches any of them."""
    keep = [np.zeros(16, np.float32), np.zeros(4, np.int32), np.zeros(1024, np.float32), np.zeros(4, np.int32)]
    return keep, [ctypes.c_void_p(a.ctypes.data) for a in keep]


def test_signatures_are_bound():
    from distilcodec_nabeel_amd import _native

    assert "dcx_generate_ragged" in _native.SIGNATURES and "dcx_decode_ragged" in _native.SIGNATURES
    L = _native.lib()
    assert L.dcx_abi_version() == 4
    assert L.dcx_generate_ragged.restype is ctypes.c_int and len(L.dcx_generate_ragged.argtypes) == 9
    assert L.dcx_decode_ragged.restype is ctypes.c_int and len(L.dcx_decode_ragged.argtypes) == 10


def test_state_error_before_finalize(handle):
    from distilcodec_nabeel_amd import _native

    L, h = handle
    keep, (x, lens, wav, codes) = _host_buffers()
    assert L.dcx_generate_ragged(h, x, lens, 1, 4, wav, None, 0, None) == _native.DCX_ERR_STATE
    assert b"dcx_finalize" in L.dcx_last_error(h)
    assert L.dcx_decode_ragged(h, codes, lens, 1, 4, wav, None, None, 0, None) == _native.DCX_ERR_STATE
    assert b"dcx_finalize" in L.dcx_last_error(h)


def test_invalid_arg_for_null_handle_or_lengths(handle):
    from distilcodec_nabeel_amd import _native

    L, h = handle
    keep, (x, lens, wav, codes) = _host_buffers()
    assert L.dcx_generate_ragged(None, x, lens, 1, 4, wav, None, 0, None) == _native.DCX_ERR_INVALID_ARG
    assert L.dcx_decode_ragged(None, codes, lens, 1, 4, wav, None, None, 0, None) == _native.DCX_ERR_INVALID_ARG
    assert L.dcx_generate_ragged(h, x, None, 1, 4, wav, None, 0, None) == _native.DCX_ERR_INVALID_ARG
    assert b"null" in L.dcx_last_error(h)
    assert L.dcx_decode_ragged(h, codes, None, 1, 4, wav, None, None, 0, None) == _native.DCX_ERR_INVALID_ARG
    assert b"null" in L.dcx_last_error(h)
