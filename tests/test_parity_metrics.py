"""The per-clip / per-row error metrics of tests/_parity.py (CPU only).

They exist because the batch-wide metrics the suite used (max|err| / max|ref| and SNR over a whole
batch) are carried by the loudest clip: a near-silent clip that is entirely wrong beside a loud one
leaves them unchanged.  tests/test_gpu_mixed_scale.py scores every clip and every row on its own."""
import numpy as np

from _parity import rel_per_clip, rel_per_row, snr_db, snr_per_clip


def _batch():
    rng = np.random.default_rng(0)
    ref = rng.standard_normal((2, 8, 50))
    ref[0] *= 2.0 ** 12
    ref[1] *= 2.0 ** -12
    return ref


def test_batch_wide_error_hides_a_wrong_quiet_clip():
    ref = _batch()
    y = ref.copy()
    y[1] = 0.0  # the quiet clip entirely wrong
    batch_wide = np.abs(y - ref).max() / np.abs(ref).max()
    assert batch_wide < 1e-6  # the old metric passes any fp32 bound
    assert snr_db(y, ref) > 120
    per_clip = rel_per_clip(y, ref)
    assert per_clip.shape == (2,)
    assert per_clip[0] == 0.0 and per_clip[1] == 1.0
    s = snr_per_clip(y, ref)
    assert s[0] > 200 and abs(s[1]) < 1e-9  # 0 dB: the error is as large as the clip


def test_per_row_sees_one_wrong_row():
    ref = _batch()
    y = ref.copy()
    y[1, :, 7] *= 1.5
    r = rel_per_row(y, ref)
    assert r.shape == (2, 50)
    assert r[1, 7] == 0.5
    r[1, 7] = 0.0
    assert not r.any()
    # channels-last views give the same numbers
    rl = rel_per_row(y.transpose(0, 2, 1), ref.transpose(0, 2, 1), channel_axis=2)
    assert rl[1, 7] == 0.5


def test_zero_reference_is_finite():
    ref = np.zeros((1, 4, 3))
    y = np.zeros((1, 4, 3))
    assert rel_per_clip(y, ref)[0] == 0.0 and not rel_per_row(y, ref).any()
    assert np.isfinite(snr_per_clip(y, ref)).all()
