"""The float32-butterfly STFT tolerance, shared by the STFT test files (test_gpu_decay_stft, test_gpu_stft_dispatch)."""
import numpy as np

STFT_F32_STATS = []


def _stft_check(got, ref, floor_db=-120.0):
    """float32-butterfly tolerance against the REFERENCE's values (golden), stated on the bins SURVEY.md section 8(d) names
    -- every bin whose reference value is > floor + 20 dB:
      * max |delta| <= 4e-3 dB, and >= 99.9 % of those bins within 1e-3 dB (section 8d's figure holds for all but a few
        bins in ten thousand: a float32 transform's error is ~2e-7 of the FRAME's rms, so the weakest bins of a frame carry
        the largest dB error);
      * 1e-3 dB on every bin within 50 dB of its frame's peak;
      * linear error below 3e-6 of the frame's peak everywhere (floor-clamped bins included)."""
    assert got.shape == ref.shape and got.dtype == np.float32
    peak = ref.max(axis=0, keepdims=True)
    named = ref > floor_db + 20.0
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    STFT_F32_STATS.append((int(named.sum()), float(err[named].max()), float(np.mean(err[named] <= 1e-3))))
    assert err[named].max() <= 4e-3, err[named].max()
    assert np.mean(err[named] <= 1e-3) >= 0.999
    strong = named & (ref > peak - 50.0)
    assert np.max(err[strong]) < 1e-3
    lin_err = np.abs(10.0 ** (got.astype(np.float64) / 20) - 10.0 ** (ref.astype(np.float64) / 20))
    assert np.max(lin_err / 10.0 ** (peak.astype(np.float64) / 20)) < 3e-6
