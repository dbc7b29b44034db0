"""
Holds the diffusion restatement (tests/diffusion_ref.py) to NumPy and to the oracle, and shows that the inputs the GPU tests
share with it test what they claim -- on a machine without a GPU.
"""
import functools

import numpy as np
import pytest

import diffusion_ref as R
from oracle import ira_oracle as O

SUM_LENGTHS = [4, 7, 8, 9, 15, 16, 17, 23, 127, 128, 129, 136, 143, 255, 256, 257, 1000, 2400, 2401, 4099, 8191, 8192]


# ------------------------------------------------------------------------------------------------ the float32 pairwise sum
@pytest.mark.parametrize("n", SUM_LENGTHS)
def test_pairwise_sum_is_numpys_bit_for_bit(n):
    rng = np.random.default_rng(n)
    for draw, level in enumerate((1e-3, 1.0, 1e3)):
        a = (level * (rng.standard_normal(n) + 0.37 * (draw + 1))).astype(np.float32)
        got, want = R.np_pairwise_sum_f32(a), np.add.reduce(a)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (n, level, got, want)
        assert R.mean_f32(a).tobytes() == np.mean(a).tobytes(), (n, level)
        sq = a * a
        assert R.mean_f32(sq).tobytes() == np.mean(sq).tobytes(), (n, level)


def test_pairwise_plan_fits_the_kernels_capacity():
    """The kernel's plan holds 8192 / 64 + 2 = 130 leaves; every accepted window length needs at most that many, and the
    leaves tile the window with no leaf above 128 values."""
    @functools.lru_cache(maxsize=None)
    def leaves(n):
        if n <= 128:
            return 1
        n2 = n // 2 - (n // 2) % 8
        return leaves(n2) + leaves(n - n2)
    assert max(leaves(n) for n in range(4, 8193)) <= 130
    assert leaves(8192) == 64
    for n in R.PLAN_WINS:
        lv = R.pairwise_leaves(n)
        assert len(lv) == leaves(n) and lv[0][0] == 0 and sum(l for _, l in lv) == n
        assert all(s1 == s0 + l0 for (s0, l0), (s1, _) in zip(lv, lv[1:])) and max(l for _, l in lv) <= 128


# ------------------------------------------------------------------------------------------------ against the oracle
ORACLE_ATOL = 2e-5          # float32 BLAS sums (oracle) against long-double ones: the bar of test_gpu_gd_diffusion.py


def _oracle_windows():
    from audio_analysis_amd.synth import synth_ir
    x = synth_ir(400, 0, 9000, rt60_seconds=0.25)
    y = synth_ir(401, 1, 9000, rt60_seconds=0.30)
    out = []
    for win, max_lag, start in [(16, 48, 300), (100, 48, 640), (1440, 240, 700), (2400, 480, 760), (2401, 480, 5000)]:
        out.append((x[start : start + win].astype(np.float32), y[start : start + win].astype(np.float32), max_lag))
    z = np.zeros(64, dtype=np.float32)
    out.append((z, x[700:764].astype(np.float32), 10))                                   # silence on one side
    out.append((x[700:703].astype(np.float32), y[700:703].astype(np.float32), 10))       # fewer than 4 samples
    return out


def _same(got, want, what):
    got, want = float(got), float(want)
    assert np.isnan(got) == np.isnan(want), (what, got, want)
    if not np.isnan(want):
        assert abs(got - want) <= ORACLE_ATOL, (what, got, want)


def test_restatement_agrees_with_the_oracle():
    for a, b, max_lag in _oracle_windows():
        what = (a.size, max_lag)
        for w in (a, b):
            _same(R.window_autocorr(w, max_lag)[0], O.window_max_abs_autocorr(w, max_lag), what)
            for thr, norm in [(1.0, True), (0.5, True), (2.0, False), (8.0, True), (7.0, True)]:
                got = R.window_echo_density(w, thr, norm)
                want = np.float32(O.window_echo_density(w, thr, norm))
                assert got.dtype == np.float32
                np.testing.assert_array_equal(got, want, err_msg=str((what, thr, norm)))     # bit-equal, NaN included
        _same(R.window_corr0(a, b), O.window_corr0(a, b), what)
        _same(R.window_iacc(a, b, max_lag), O.window_iacc_max(a, b, max_lag), what)
        _same(R.window_iacc(b, a, max_lag), O.window_iacc_max(b, a, max_lag), what)
    assert R.gaussian_exceedance(1.0) == O.gaussian_exceedance(1.0)
    assert R.gaussian_exceedance(8.0) <= 1e-12 < R.gaussian_exceedance(7.0)


def test_series_loop_over_frames():
    x = R.decaying_noise(400, 11)
    y = R.decaying_noise(400, 12, dc=-0.2)
    ac, ed = R.series_mono(x, 3, 4, 100, 7, 20)
    c0, ia = R.series_stereo(x, y, 3, 4, 100, 7, 20)
    assert all(v.dtype == np.float32 and v.shape == (4,) for v in (ac, ed, c0, ia))
    assert ac[2] == np.float32(R.window_autocorr(x[17:117], 20)[0]) and ed[2] == R.window_echo_density(x[17:117], 1.0, True)
    assert ia[3] == np.float32(R.window_iacc(x[24:124], y[24:124], 20)) and c0[3] == np.float32(R.window_corr0(x[24:124], y[24:124]))
    exact = R.series_mono(x, 3, 4, 100, 7, 20, exact=True)[0]
    assert exact.dtype == np.longdouble and np.all(np.abs(exact - ac) <= 2.0 ** -24 * exact)


# ------------------------------------------------------------------------------------------------ planted inputs
MARGIN = 0.3


def _planted(w, d, max_lag):
    peak, lag, runner = R.window_autocorr(w, max_lag)
    assert lag == d and peak - runner > MARGIN, (d, max_lag, float(peak), lag, float(runner))
    return float(peak), float(runner)


def test_every_lag_windows_plant_their_lag():
    cases = R.every_lag_windows()
    assert [d for d, _ in cases] == list(range(1, 63))
    for d, w in cases:
        _planted(w, d, 62)


def test_boundary_windows_plant_their_lag():
    for d, w in R.boundary_windows():
        lags = R.lag_sums(R.remove_mean(w), R.remove_mean(w), 0, R.BOUNDARY_N - 2)
        r = np.abs(lags[1:] / lags[0])                                                   # r[k]: lag k + 1
        assert int(np.argmax(r)) + 1 == d and 0.4 < r[d - 1] < 0.5 and np.delete(r, d - 1).max() <= 0.04
        for max_lag in R.BOUNDARY_MAX_LAGS:
            peak = R.window_autocorr(w, max_lag)[0]
            if d <= max_lag:
                assert peak == r[d - 1]
            else:                                                                        # planted past the range: absent
                assert peak == r[:max_lag].max() and peak < 0.05


def test_clip_window_peak_leaves_with_its_lag():
    w = R.clip_window()
    _planted(w, R.CLIP_D, R.CLIP_D)
    _planted(w, R.CLIP_D, 4096)
    assert R.window_autocorr(w, R.CLIP_D - 1)[0] < 0.1
    assert R.window_autocorr(w, 62) == R.window_autocorr(w, 63) == R.window_autocorr(w, 4096)   # clipped to n - 2


def test_subrange_windows_plant_their_lag():
    for d in (9, 10):
        for i, w in R.subrange_windows(d):
            assert w[i] > 0.9 and w[i + d] > 0.9
            _planted(w, d, d)


def test_stereo_pairs_plant_their_signed_lag():
    for d, a, b in R.direction_pairs():
        peak, lag, runner = R.window_iacc(a, b, 62, detail=True)
        assert lag == d and peak > 0.9 and peak - runner > MARGIN, (d, float(peak), lag, float(runner))
        peak, lag, _ = R.window_iacc(b, a, 62, detail=True)                              # swapped: the lag changes sign
        assert lag == -d and peak > 0.9
    for d, a, b in R.direction_pairs([R.CLIP_D, -R.CLIP_D]):
        assert R.window_iacc(a, b, R.CLIP_D, detail=True)[1] == d
        assert R.window_iacc(a, b, R.CLIP_D - 1) < 0.2                                   # absent
    for d, a, b in R.long_stereo_pairs():
        peak, lag, runner = R.window_iacc(a, b, 2400, detail=True)
        assert lag == d and peak - runner > MARGIN, (d, float(peak), lag, float(runner))


# ------------------------------------------------------------------------------------------------ threshold inputs
def _energy_and_rms(w):
    w0, rms = R.echo_density_parts(w)
    return float(np.dot(w0.astype(np.longdouble), w0.astype(np.longdouble))), float(rms)


def test_silence_inputs_keep_their_distance_from_the_threshold():
    """Finite means 10 x above 1e-20, NaN means 10 x below (exact zeros aside): no case sits where float64 against long
    double could decide it."""
    for name, (w, ac_finite, ed_finite) in R.nan_rule_windows().items():
        energy, rms = _energy_and_rms(w)
        assert (energy >= 1e-19) if ac_finite else (energy == 0.0 or energy <= 1e-21), (name, energy)
        assert (rms >= 1e-19) if ed_finite else (rms == 0.0 or rms <= 1e-21), (name, rms)
        assert np.isfinite(float(R.window_autocorr(w, 48)[0])) == ac_finite, name
        assert np.isfinite(R.window_echo_density(w, 1.0, True)) == ed_finite, name
    w0 = R.remove_mean(R.nan_rule_windows()["const_0.1"][0])
    assert np.all(w0 == w0[0]) and abs(float(w0[0])) == 2.0 ** -27                       # the float32 mean's residue: one ulp
    assert not R.remove_mean(R.nan_rule_windows()["const_0.5"][0]).any()
    for name, (a, b, c0_finite, ia_finite) in R.degenerate_pairs().items():
        (aa, _), (bb, _) = _energy_and_rms(a), _energy_and_rms(b)
        den = float(np.sqrt(np.longdouble(aa) * np.longdouble(bb)))
        for e in (aa, bb):
            assert e >= 1e-19 or e == 0.0 or e <= 1e-21, (name, e)
        assert (min(aa, bb) >= 1e-19) == c0_finite and (den >= 1e-19 if ia_finite else den == 0.0), (name, aa, bb, den)
        assert np.isfinite(float(R.window_corr0(a, b))) == c0_finite, name
        assert np.isfinite(float(R.window_iacc(a, b, 62))) == ia_finite, name
    d = R.degenerate_pairs()
    assert np.float32(R.window_corr0(*d["identical"][:2])) == 1.0 and np.float32(R.window_iacc(*d["identical"][:2], 62)) == 1.0
    assert np.float32(R.window_corr0(*d["negated"][:2])) == -1.0 and np.float32(R.window_iacc(*d["negated"][:2], 62)) == 1.0


def test_alternating_window_sits_exactly_on_the_threshold():
    w = R.alternating(64)
    w0, rms = R.echo_density_parts(w)
    assert R.mean_f32(w) == 0.0 and np.array_equal(w0, w) and rms == 1.0
    assert R.window_echo_density(w, 1.0, False) == 0.0 and R.window_echo_density(w, 1.0, True) == 0.0
    assert R.window_echo_density(w, 0.999999, False) == 1.0
    assert R.window_echo_density(w, 0.999999, True) == np.float32(1.0 / R.gaussian_exceedance(0.999999))


# ------------------------------------------------------------------------------------------------ the LDS limit, host side
#             max_lag:      1     480    4096      (by hand from the kernel file's diff_lds_bytes, limit 150 KiB)
LIMIT_TABLE = {False: {1: 8192, 480: 8192, 4096: 4597},
               True: {1: 6750, 480: 6367, 4096: 1116}}


def test_largest_window_per_kernel_and_lag():
    from audio_analysis_amd.analyse import diffusion as dm
    for stereo, row in LIMIT_TABLE.items():
        for max_lag, win in row.items():
            assert dm.max_window_samples(max_lag, stereo) == win, (stereo, max_lag)
            assert dm.diffusion_lds_bytes(win, max_lag, stereo) <= 150 * 1024
            if win < 8192:
                assert dm.diffusion_lds_bytes(win + 1, max_lag, stereo) > 150 * 1024


def test_window_geometry_refuses_per_kernel_before_device_work():
    from audio_analysis_amd.analyse import diffusion as dm
    sr = 48000
    st = dm.DiffusionAnalysisSettings(window_seconds=6367 / sr, max_lag_milliseconds=10.0)
    assert dm.window_geometry(sr, st) == dm.window_geometry(sr, st, stereo=True) == (6367, 480, 480)
    st = dm.DiffusionAnalysisSettings(window_seconds=6368 / sr, max_lag_milliseconds=10.0)
    assert dm.window_geometry(sr, st) == (6368, 480, 480)                                # the mono kernel takes it
    with pytest.raises(ValueError, match=r"diffusion windows are limited to 6367 samples .* 480 samples"):
        dm.window_geometry(sr, st, stereo=True)
    with pytest.raises(ValueError, match=r"diffusion windows are limited to 6367 "):
        dm.stereo_series(np.zeros(9000, np.float32), np.zeros(9000, np.float32), sr, st)  # no engine is ever asked for
    st = dm.DiffusionAnalysisSettings(window_seconds=4598 / sr, max_lag_milliseconds=4096e3 / sr)
    with pytest.raises(ValueError, match=r"diffusion windows are limited to 4597 samples .* 4096 samples"):
        dm.window_geometry(sr, st)
    with pytest.raises(ValueError, match=r"diffusion windows are limited to 1116 "):
        dm.window_geometry(sr, st, stereo=True)
    with pytest.raises(ValueError, match=r"diffusion windows are limited to 8192 "):
        dm.window_geometry(sr, dm.DiffusionAnalysisSettings(window_seconds=8193 / sr))
    with pytest.raises(ValueError, match=r"lags are limited to 4096"):
        dm.window_geometry(sr, dm.DiffusionAnalysisSettings(max_lag_milliseconds=4097e3 / sr))


def test_stereo_file_with_an_overlong_window_fails_before_the_mono_pass(tmp_path, monkeypatch):
    from scipy.io import wavfile
    from audio_analysis_amd.analyse import diffusion as dm
    sr = 48000
    rng = np.random.default_rng(5)
    wav = tmp_path / "s.wav"
    wavfile.write(str(wav), sr, (rng.standard_normal((12000, 2)) * 3000).astype(np.int16))

    def no_device(*a, **k):
        raise AssertionError("device work before the geometry check")
    monkeypatch.setattr(dm, "get_engine", no_device)
    with pytest.raises(ValueError, match=r"diffusion windows are limited to 6367 "):
        dm.analyse_diffusion_from_wav_file(wav, dm.DiffusionAnalysisSettings(window_seconds=0.14))
