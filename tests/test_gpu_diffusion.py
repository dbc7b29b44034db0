"""
The diffusion kernels (ira_diffusion.hip through Engine.diffusion / Engine.diffusion_stereo) against the restatement of
tests/diffusion_ref.py, at the edges of the pairwise-sum plan, the lag groups, the row sub-ranges and the LDS limit.

Bars (derived, see diffusion_ref.bound):
  max |autocorr|, corr0, IACC   |got - ref| <= 2^-24 |ref| + 4 win 2^-53 against LONG-DOUBLE sums of the same float32
                                mean-removed window: one float32 rounding of the output plus float64 accumulation;
  echo density                  bit-equal, NaN pattern included (a count over float32 values restated step by step).
Every case is one launch of a handful of workgroups.  tests/test_diffusion_ref_cpu.py shows that each planted input has its
peak where this file assumes it, with a margin of 0.3 over every other lag: a kernel that drops that lag misses the bar.
"""
import numpy as np
import pytest

import diffusion_ref as R

pytestmark = pytest.mark.gpu

SR = 48000


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def _gauss(thr_rms, normalise):
    from audio_analysis_amd.analyse.diffusion import _expected_gaussian_abs_exceedance
    return _expected_gaussian_abs_exceedance(thr_rms) if normalise else -1.0


def _in_range(lengths, starts, frames, win, hop):
    """No window of the job tables reaches past its channel (the kernel trusts them)."""
    for n, s, f in zip(lengths, starts, frames):
        assert s >= 0 and (f == 0 or s + (f - 1) * hop + win <= n), (n, s, f, win, hop)


def run_mono(chans, starts, frames, win, hop, max_lag, thr_rms=1.0, normalise=True):
    """One launch: [(ac, ed)] per channel and the output offsets the engine computed."""
    eng = _eng()
    chans = [np.asarray(c, dtype=np.float32) for c in chans]
    starts, frames = np.asarray(starts, dtype=np.int64), np.asarray(frames, dtype=np.int32)
    _in_range([c.size for c in chans], starts, frames, win, hop)
    b = eng.upload(chans)
    ac, ed, off = eng.diffusion(b.x, b.off + starts, frames, win, hop, max_lag, float(thr_rms), _gauss(thr_rms, normalise))
    ac, ed = ac.cpu().numpy(), ed.cpu().numpy()
    assert ac.dtype == np.float32 and ed.dtype == np.float32
    return [(ac[o : o + f].copy(), ed[o : o + f].copy()) for o, f in zip(off, frames)], off


def run_stereo(pairs, starts, frames, win, hop, max_lag):
    """One launch over (left, right) pairs: [(corr0, iacc)] per pair."""
    eng = _eng()
    chans = [np.asarray(c, dtype=np.float32) for p in pairs for c in p]
    starts, frames = np.asarray(starts, dtype=np.int64), np.asarray(frames, dtype=np.int32)
    _in_range([c.size for c in chans[0::2]], starts, frames, win, hop)
    _in_range([c.size for c in chans[1::2]], starts, frames, win, hop)
    b = eng.upload(chans)
    li = 2 * np.arange(len(pairs))
    c0, ia, off = eng.diffusion_stereo(b.x, b.off[li] + starts, b.off[li + 1] + starts, frames, win, hop, max_lag)
    c0, ia = c0.cpu().numpy(), ia.cpu().numpy()
    assert c0.dtype == np.float32 and ia.dtype == np.float32
    return [(c0[o : o + f].copy(), ia[o : o + f].copy()) for o, f in zip(off, frames)]


def close(got, ref, win, quantity, what):
    """got (float32, device) against ref (long double) under the derived bar; NaN patterns equal."""
    got, ref = np.atleast_1d(got), np.atleast_1d(np.asarray(ref, dtype=np.longdouble))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (quantity, what, got, ref)
    ok = ~np.isnan(ref)
    if ok.any():
        err = np.abs(got[ok].astype(np.longdouble) - ref[ok]).astype(np.float64)
        bar = R.bound(ref[ok], win)
        k = int(np.argmax(err / bar))
        print(f"DIFF-ERR {quantity} {what}: |got - ref| {err[k]:.3e} bound {bar[k]:.3e} (ref {float(ref[ok][k]):.6f})")
        assert np.all(err <= bar), (quantity, what, got[ok], ref[ok].astype(np.float64), err, bar)


def check_mono(chans, starts, frames, win, hop, max_lag, what, thr_rms=1.0, normalise=True):
    got, _ = run_mono(chans, starts, frames, win, hop, max_lag, thr_rms, normalise)
    for i, (x, s, f) in enumerate(zip(chans, starts, frames)):
        ac, ed = R.series_mono(np.asarray(x, dtype=np.float32), int(s), int(f), win, hop, max_lag, thr_rms, normalise, exact=True)
        close(got[i][0], ac, win, "autocorr", f"{what} ch{i}")
        np.testing.assert_array_equal(got[i][1], ed, err_msg=f"echo density, {what} ch{i}")
    return got


def check_stereo(pairs, starts, frames, win, hop, max_lag, what):
    got = run_stereo(pairs, starts, frames, win, hop, max_lag)
    for i, ((a, b), s, f) in enumerate(zip(pairs, starts, frames)):
        c0, ia = R.series_stereo(np.asarray(a, np.float32), np.asarray(b, np.float32), int(s), int(f), win, hop, max_lag, exact=True)
        close(got[i][0], c0, win, "corr0", f"{what} pair{i}")
        close(got[i][1], ia, win, "iacc", f"{what} pair{i}")
    return got


# ================================================================================================== mono
@pytest.mark.parametrize("win", R.PLAN_WINS)
def test_01_pairwise_plan(win):
    """Every branch of the float32 pairwise sum: in order (< 8), tails, one leaf against two (128 / 129), odd splits, the
    largest window.  The DC offset makes the mean matter; the echo density is only right if the sum is NumPy's."""
    x = R.decaying_noise(win + 2 * 7, 100 + win)
    check_mono([x], [0], [3], win, 7, 48, f"plan win {win}")


def test_02_every_lag_once():
    """62 one-frame channels, channel d with its peak at lag d: no lag, lag group or partial group can go missing."""
    cases = R.every_lag_windows()
    check_mono([w for _, w in cases], [0] * len(cases), [1] * len(cases), 64, 1, 62, "every lag")


@pytest.mark.parametrize("max_lag", R.BOUNDARY_MAX_LAGS)
def test_03_lag_group_and_split_boundaries(max_lag):
    """2400 lags (nsub == 1), 2295 lags (255 groups, nsub == 1 by division) and 1148 lags (128 groups, two row halves), with
    peaks at the first lag, around the group edges 9 | 10 and 2295 | 2296 | 2297, at 2304 and at the last two lags."""
    cases = R.boundary_windows()
    got = check_mono([w for _, w in cases], [0] * len(cases), [1] * len(cases), R.BOUNDARY_N, 1, max_lag, f"max_lag {max_lag}")
    for (d, _), (ac, _) in zip(cases, got):
        assert (ac[0] > 0.4) == (d <= max_lag), (d, max_lag, ac)                 # beyond the range the peak is absent


def test_04_clipping():
    """max_lag beyond win - 2 is clipped to it: identical outputs from 62 upward; lag 40 is there at 40 and gone at 39."""
    cases = R.every_lag_windows()
    chans = [cases[0][1], cases[39][1], cases[60][1], cases[61][1], R.clip_window()]      # d = 1, 40, 61, 62 and 40 again
    out = {}
    for max_lag in (1, 39, 40, 61, 62, 63, 64, 500, 4096):
        out[max_lag] = check_mono(chans, [0] * 5, [1] * 5, 64, 1, max_lag, f"clip max_lag {max_lag}")
    for max_lag in (63, 64, 500, 4096):
        for (ac, ed), (ac62, ed62) in zip(out[max_lag], out[62]):
            np.testing.assert_array_equal(ac, ac62)
            np.testing.assert_array_equal(ed, ed62)
    assert out[40][4][0][0] > 0.4 > 0.1 > out[39][4][0][0]
    assert out[62][3][0][0] > 0.4 > 0.1 > out[61][3][0][0]


@pytest.mark.parametrize("max_lag", [9, 10])
def test_05_row_sub_ranges(max_lag):
    """One lag group over 256 row sub-ranges of 10 (max_lag 9), two groups over 128 of 19 (max_lag 10): the planted product
    pairs straddle the sub-range edges and sit in the last rows."""
    cases = R.subrange_windows(max_lag)
    got = check_mono([w for _, w in cases], [0] * len(cases), [1] * len(cases), R.SUBRANGE_N, 1, max_lag, f"rows max_lag {max_lag}")
    assert all(ac[0] > 0.4 for ac, _ in got)


def test_06_echo_density_semantics():
    from audio_analysis_amd.analyse.diffusion import _expected_gaussian_abs_exceedance as exceedance
    alt = R.alternating(64)
    (_, ed), = check_mono([alt], [0], [1], 64, 1, 48, "alternating thr 1.0", thr_rms=1.0)
    assert ed[0] == 0.0                                                                    # |w0| == thr: strict >
    (_, ed), = check_mono([alt], [0], [1], 64, 1, 48, "alternating thr 0.999999", thr_rms=0.999999)
    assert ed[0] == np.float32(1.0 / exceedance(0.999999))
    (_, ed), = check_mono([alt], [0], [1], 64, 1, 48, "alternating raw", thr_rms=0.999999, normalise=False)
    assert ed[0] == 1.0
    noise = R.decaying_noise(1000 + 4 * 7, 61, dc=0.0)
    for thr in (0.5, 2.0):
        (_, ed), = check_mono([noise], [0], [5], 1000, 7, 48, f"noise thr {thr}", thr_rms=thr)
        (_, raw), = check_mono([noise], [0], [5], 1000, 7, 48, f"noise thr {thr} raw", thr_rms=thr, normalise=False)
        count = np.rint(raw.astype(np.float64) * 1000.0)                                   # the raw fraction is count / win
        assert np.all((count > 0) & (count < 1000)) and np.array_equal(raw, (count / 1000.0).astype(np.float32))
        np.testing.assert_array_equal(ed, (count / 1000.0 / exceedance(thr)).astype(np.float32))
    assert exceedance(8.0) <= 1e-12 < exceedance(7.0)
    (ac, ed), = check_mono([noise], [0], [5], 1000, 7, 48, "thr 8.0", thr_rms=8.0)
    assert np.all(np.isnan(ed)) and np.all(np.isfinite(ac))                                # exceedance <= 1e-12: NaN
    (_, ed), = check_mono([noise], [0], [5], 1000, 7, 48, "thr 7.0", thr_rms=7.0)
    assert np.all(np.isfinite(ed))                                                         # 2.6e-12 > 1e-12: finite
    (_, ed), = check_mono([noise], [0], [5], 1000, 7, 48, "thr 8.0 raw", thr_rms=8.0, normalise=False)
    assert np.all(np.isfinite(ed))                                                         # no exceedance to divide by


def test_07_nan_rules_fire_independently():
    """den <= 1e-20 and rms <= 1e-20 are separate rules; silent windows do not disturb their neighbours in the channel."""
    w = R.nan_rule_windows()
    n = R.NAN_RULE_N
    order = [["zeros", "const_0.5", "const_0.1"], ["noise_1e-12", "noise", "zeros"], ["const_0.1", "noise_1e-12", "const_0.5"]]
    chans = [np.concatenate([w[k][0] for k in names]) for names in order]
    got = check_mono(chans, [0] * 3, [3] * 3, n, n, 48, "nan rules")
    for names, (ac, ed) in zip(order, got):
        assert [bool(np.isfinite(v)) for v in ac] == [w[k][1] for k in names], (names, ac)
        assert [bool(np.isfinite(v)) for v in ed] == [w[k][2] for k in names], (names, ed)


def test_08_batch_plumbing():
    """Five channels, frame counts (1, 5, 0, 3, 2), odd offsets: each live channel equals itself launched alone, bit for bit."""
    win, hop, max_lag = 100, 13, 48
    frames, starts = [1, 5, 0, 3, 2], [1, 3, 5, 7, 11]
    chans = [R.decaying_noise(s + max(f - 1, 0) * hop + win + 3, 80 + i) for i, (s, f) in enumerate(zip(starts, frames))]
    got, off = run_mono(chans, starts, frames, win, hop, max_lag)
    np.testing.assert_array_equal(off, [0, 1, 6, 6, 9])
    check_mono(chans, starts, frames, win, hop, max_lag, "batch")
    for i, f in enumerate(frames):
        assert got[i][0].size == f and got[i][1].size == f
        if f:
            (ac, ed), = run_mono([chans[i]], [starts[i]], [f], win, hop, max_lag)[0]
            np.testing.assert_array_equal(got[i][0], ac)
            np.testing.assert_array_equal(got[i][1], ed)


def test_09_largest_window():
    x = R.decaying_noise(8192 + 480, 9)
    check_mono([x], [0], [2], 8192, 480, 480, "win 8192")


# ================================================================================================== stereo
@pytest.mark.parametrize("win", [w for w in R.PLAN_WINS if w <= 4099])
def test_10_stereo_plan_and_lag_edges(win):
    a = R.decaying_noise(win + 2 * 7, 300 + win, dc=0.3)
    b = (0.6 * a + R.decaying_noise(win + 2 * 7, 700 + win, dc=-0.15)).astype(np.float32)   # correlated, other mean
    check_stereo([(a, b)], [0], [3], win, 7, 48, f"stereo plan win {win}")


def test_11_direction_and_lag_zero():
    """Peaks planted at +d and -d (a kernel that scans one direction only loses half of them), lag 0 counted once."""
    cases = R.direction_pairs()
    pairs = [(a, b) for _, a, b in cases]
    one = [1] * len(pairs)
    got = check_stereo(pairs, [0] * len(pairs), one, 64, 1, 62, "direction")
    assert all(ia[0] > 0.9 for _, ia in got)
    swapped = check_stereo([(b, a) for a, b in pairs], [0] * len(pairs), one, 64, 1, 62, "direction swapped")
    for (c0, ia), (c0s, ias), (d, a, b) in zip(got, swapped, cases):
        np.testing.assert_array_equal(c0, c0s)                                             # corr0: the same products
        ref = R.window_iacc(a, b, 62)
        close(ias, [ref], 64, "iacc", f"swapped against unswapped d {d}")
    far = R.direction_pairs([R.CLIP_D, -R.CLIP_D])
    far_pairs = [(a, b) for _, a, b in far]
    there = check_stereo(far_pairs, [0, 0], [1, 1], 64, 1, R.CLIP_D, "direction d 40 max_lag 40")
    gone = check_stereo(far_pairs, [0, 0], [1, 1], 64, 1, R.CLIP_D - 1, "direction d 40 max_lag 39")
    assert all(ia[0] > 0.9 for _, ia in there) and all(ia[0] < 0.2 for _, ia in gone)


def test_12_long_lag_range():
    """2401 and 2400 lags in the two passes (nsub == 1 in both), peaks at the 255 | 256 group edge and at the last lag."""
    cases = R.long_stereo_pairs()
    got = check_stereo([(a, b) for _, a, b in cases], [0] * len(cases), [1] * len(cases), R.BOUNDARY_N, 1, 2400, "long lags")
    assert all(ia[0] > 0.4 for _, ia in got)


def test_13_degenerate_pairs():
    d = R.degenerate_pairs()
    names = list(d)
    got = dict(zip(names, check_stereo([d[k][:2] for k in names], [0] * len(names), [1] * len(names), R.NAN_RULE_N, 1, 62, "degenerate")))
    assert got["identical"][0][0] == 1.0 and got["identical"][1][0] == 1.0
    assert got["negated"][0][0] == -1.0 and got["negated"][1][0] == 1.0
    assert np.isnan(got["right_zeros"][0][0]) and np.isnan(got["right_zeros"][1][0])
    assert np.isnan(got["left_1e-12"][0][0]) and np.isfinite(got["left_1e-12"][1][0])     # the two rules are separate


def test_14_many_files_one_launch():
    """stereo_series_device on a split batch of four files against stereo_series per file and against the restatement."""
    from audio_analysis_amd.analyse import diffusion as dm
    eng = _eng()
    sr = 8000
    st = dm.DiffusionAnalysisSettings(window_seconds=0.008, hop_seconds=0.002, max_lag_milliseconds=1.0)
    win, hop, max_lag = dm.window_geometry(sr, st, stereo=True)
    assert (win, hop, max_lag) == (64, 16, 8)
    rng = np.random.default_rng(14)
    files = []
    for n, peak_at in [(200, 30), (70, 20), (333, 150), (129, 65)]:                       # the second: shorter than a window
        l, r = R.decaying_noise(n, int(rng.integers(1 << 30)), dc=0.1), R.decaying_noise(n, int(rng.integers(1 << 30)), dc=-0.2)
        l[peak_at] += 40.0                                                                  # the mean peaks here, although
        r[peak_at] += 40.0
        r[peak_at - 5] -= 60.0                                                              # the right channel alone peaks earlier
        files.append((l, r))
    split = eng.upload([c for f in files for c in f])
    peaks = [int(np.argmax(np.abs(((l.astype(np.float64) + r.astype(np.float64)) * 0.5).astype(np.float32)))) for l, r in files]
    assert peaks == [30, 20, 150, 65]
    series = dm.stereo_series_device(eng, split, [0, 2, 4, 6], peaks, sr, st)
    for j, ((l, r), p) in enumerate(zip(files, peaks)):
        frames = max(0, 1 + (l.size - p - win) // hop) if l.size - p >= win else 0
        c0, ia = dm.stereo_series(l, r, sr, st)
        np.testing.assert_array_equal(series[j][0], c0)
        np.testing.assert_array_equal(series[j][1], ia)
        assert c0.size == frames == ia.size
        rc0, ria = R.series_stereo(l, r, p, frames, win, hop, max_lag, exact=True)
        close(c0, rc0, win, "corr0", f"file {j}")
        close(ia, ria, win, "iacc", f"file {j}")
    assert [s[0].size for s in series] == [7, 0, 8, 1]
    late = dm.DiffusionAnalysisSettings(window_seconds=0.008, hop_seconds=0.002, max_lag_milliseconds=1.0, ignore_leading_seconds=10.0)
    assert all(dm.trim_start(l.size, p, sr, late) == l.size for (l, _), p in zip(files, peaks))   # clamped to the remainder
    assert all(a.size == 0 and b.size == 0 for a, b in dm.stereo_series_device(eng, split, [0, 2, 4, 6], peaks, sr, late))
    assert dm.stereo_series(files[0][0], files[0][1], sr, late)[0].size == 0
    part = dm.DiffusionAnalysisSettings(window_seconds=0.008, hop_seconds=0.002, max_lag_milliseconds=1.0, ignore_leading_seconds=0.005)
    series = dm.stereo_series_device(eng, split, [0, 2, 4, 6], peaks, sr, part)             # 40 samples further in
    for j, ((l, r), p) in enumerate(zip(files, peaks)):
        frames = 1 + (l.size - p - 40 - win) // hop if l.size - p - 40 >= win else 0
        rc0, ria = R.series_stereo(l, r, p + 40, frames, win, hop, max_lag, exact=True)
        close(series[j][0], rc0, win, "corr0", f"file {j} ignore 5 ms")
        close(series[j][1], ria, win, "iacc", f"file {j} ignore 5 ms")


# ================================================================================================== the LDS limit
def test_15_lds_limit():
    """The largest window each kernel stages (by hand from the kernel file's LDS formula against 150 KiB) runs and is right;
    one sample more is refused by the library before anything is launched, and by window_geometry before that."""
    from audio_analysis_amd._lib import IraError
    from audio_analysis_amd.analyse import diffusion as dm
    assert [dm.max_window_samples(m, False) for m in (1, 480, 4096)] == [8192, 8192, 4597]
    assert [dm.max_window_samples(m, True) for m in (1, 480, 4096)] == [6750, 6367, 1116]
    eng = _eng()
    x = R.decaying_noise(6367 + 1 + 5, 15)
    y = R.decaying_noise(6367 + 1 + 5, 16, dc=-0.1)
    check_mono([x[: 4597 + 5]], [0], [2], 4597, 5, 4096, "mono limit")
    check_stereo([(x, y)], [0], [2], 6367, 5, 480, "stereo limit")
    b = eng.upload([x, y])
    one = np.array([1], dtype=np.int32)
    with pytest.raises(IraError):
        eng.diffusion(b.x, b.off[:1], one, 4598, 5, 4096, 1.0, -1.0)
    with pytest.raises(IraError):
        eng.diffusion_stereo(b.x, b.off[:1], b.off[1:], one, 6368, 5, 480)
    eng.diffusion(b.x, b.off[:1], one, 6368, 5, 480, 1.0, -1.0)                             # the mono kernel takes that one
    eng.sync()
    for stereo, win, max_lag in [(False, 4598, 4096), (True, 6368, 480), (True, 6751, 1), (True, 1117, 4096)]:
        st = dm.DiffusionAnalysisSettings(window_seconds=win / SR, max_lag_milliseconds=max_lag * 1e3 / SR)
        with pytest.raises(ValueError, match=f"diffusion windows are limited to {win - 1} samples"):
            dm.window_geometry(SR, st, stereo=stereo)
