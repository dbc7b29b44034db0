"""
Harmonic distortion on the device (ira_harmonic_windows, ira_harmonic_band_powers, audio_analysis_amd.analyse.harmonics)
against the float64 restatement in harmonics_ref.py and the analytic distortion of a synthetic sweep.

Bounds, all derived, none measured.
  Segments: bit for bit (one float64 product, one rounding to float32 on both sides).
  Band powers on given spectra: relative error <= (cnt + 4) 2^-53.  The terms are non-negative; each is rounded at most
    three times (two squares, their sum), the cnt - 1 additions and the division add one rounding each along any order of
    summation, and the restatement's own long-double arithmetic adds less than one more.
  Band powers end to end: the segments are the restatement's to the bit, so the spectra differ by the forward transform's
    error alone, which tests/test_gpu_longfft.py holds to d = 1e-13 of the row's largest bin magnitude M.  A bin S + e with
    |e| <= d M changes |S|^2 by at most 2 |S| d M + (d M)^2; the mean over a band of 2 |S| d M is at most
    2 sqrt(E_ref) d M (Cauchy-Schwarz).  Hence 2 sqrt(E_ref) d M + (d M)^2 + (cnt + 4) 2^-53 E_ref.
  HD2, HD3 of the synthetic sweep: within 1 % of c2, c3 on the grid points from 800 Hz to 0.8 f2 / (k 2^(1/(2P))), the
    condition and range of tests/test_harmonics_cpu.py.
Every test prints its measured maximum before it asserts.
"""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import harmonics_ref as R

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
FS, T, F1, F2, AMP, TAIL = 48000, 0.5, 100.0, 20000.0, 0.5, 0.1
PAIRS = ((0.03, 0.01), (0.05, 0.002))                     # (c2, c3) of the two channels of the stereo recording
U = 2.0 ** -53
D_FFT = 1e-13


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def _settings(**kw):
    from audio_analysis_amd.analyse.harmonics import HarmonicDistortionSettings
    base = dict(sweep_seconds=T, start_frequency_hz=F1, end_frequency_hz=F2, max_harmonic=3, points_per_octave=3)
    base.update(kw)
    return HarmonicDistortionSettings(**base)


@pytest.fixture(scope="module")
def signals():
    """sweep, the two muted recordings (PAIRS) and the unmuted recording of PAIRS[0]; built once, never changed."""
    x, y0 = R.test_signal(FS, T, F1, F2, AMP, TAIL, *PAIRS[0])
    _, y1 = R.test_signal(FS, T, F1, F2, AMP, TAIL, *PAIRS[1])
    _, yu = R.test_signal(FS, T, F1, F2, AMP, TAIL, *PAIRS[0], mute=False)
    for a in (x, y0, y1, yu):
        a.setflags(write=False)
    return dict(x=x, y=(y0, y1), unmuted=yu)


def _check_hd(result, pair, what):
    f = np.array(result.frequencies_hz)
    for k, c in zip((2, 3), pair):
        m = R.flat_range(f, k, F2, 3)
        err = np.abs(np.array(result.hd[k - 2])[m] / c - 1.0)
        print(f"{what}: HD{k} on {int(m.sum())} points, largest relative error {err.max():.2e}")
        assert m.sum() >= 8 and err.max() <= 0.01, (what, k, err)


# ------------------------------------------------------------------------------------------------ 1: windows, bit for bit
@pytest.mark.parametrize("guard,w_len", [(5, 203), (64, 2100)])          # seg 208: no multiple of 64; seg 2164: three tiles
def test_windows_bit_for_bit(guard, w_len):
    eng = _eng()
    rng = np.random.default_rng(11)
    n_fft = np.array([4096, 8192, 4096], dtype=np.int32)
    n_search = np.array([4001, 6000, 4001], dtype=np.int64)
    spikes = [2, 4096, 4000]                                  # sample 2, mid-buffer, n_search - 1
    # lags: none; one that puts the rows of the peak at sample 2 wholly at the buffer's end; one longer than the short
    # buffers, so that their start index wraps twice
    lags = np.array([0, 700, 4096 + 100], dtype=np.int64)
    chans = [rng.standard_normal(int(n)).astype(np.float32) for n in n_fft]
    for c, (h, p) in enumerate(zip(chans, spikes)):
        h[p] = 50.0 if c != 1 else -50.0
    chans[2][4001] = 80.0                                     # larger, but outside the search: the peak pick must not see it
    off = np.array([1, 1 + 4096, 1 + 4096 + 8192], dtype=np.int64)       # odd offsets
    flat = np.full(int(off[-1]) + 4096 + 9, 0.25, np.float32)            # the gaps are not zero: a read outside would show
    for o, h in zip(off, chans):
        flat[o : o + h.size] = h
    h_dev = eng.to_dev(flat)
    pk, pa = eng.harmonic_peaks(h_dev, off, n_search)
    assert list(pk.cpu().numpy()) == spikes and list(pa.cpu().numpy()) == [50.0, 50.0, 50.0]
    w = R.window(guard, w_len, 0.25)
    seg = guard + w_len
    rows = eng.harmonic_windows(h_dev, off, n_fft, pk, lags, guard, w).cpu().numpy()
    assert rows.shape == (9, seg) and rows.dtype == np.float32
    wraps = 0
    for c, (h, p) in enumerate(zip(chans, spikes)):
        want = R.segments(h, p, lags, guard, w)
        for k in range(3):
            start = (p - int(lags[k]) - guard) % h.size
            wraps += start + seg > h.size
            assert np.array_equal(rows[3 * c + k], want[k]), (c, k, start)
    assert wraps >= 3                                         # rows that run over the buffer's end are among them
    assert rows[0][guard] == np.float32(50.0) and w[guard] == 1.0      # the peak sits right behind the guard samples


# ------------------------------------------------------------------------------------------------ 2: band powers
def _random_spectra(rng, nrow, nbins):
    mag = np.exp(rng.uniform(-6.0, 6.0, (nrow, nbins)))      # 100 dB of dynamic range inside a band
    return mag * rng.standard_normal((nrow, nbins)) + 1j * mag * rng.standard_normal((nrow, nbins))


def _device_powers(eng, spec, lo, cnt, lead=3):
    nrow, nbins = spec.shape
    flat = np.full((lead + nrow * nbins + 5, 2), 7.0)        # the gaps are not zero
    off = lead + np.arange(nrow, dtype=np.int64) * nbins
    for r in range(nrow):
        flat[off[r] : off[r] + nbins, 0], flat[off[r] : off[r] + nbins, 1] = spec[r].real, spec[r].imag
    return eng.harmonic_band_powers(eng.to_dev(flat.reshape(-1)), off, lo, cnt, nbins).cpu().numpy()


@pytest.mark.parametrize("n_h", [256, 4096])
def test_band_powers_against_the_restatement(n_h):
    eng = _eng()
    rng = np.random.default_rng(n_h)
    nbins = n_h // 2 + 1
    if n_h == 256:
        bands = [(0, 1), (3, 63), (5, 64), (64, 65), (100, 29), (7, 0), (128, 1), (0, 129)]
    else:
        bands = [(17, 1), (1, 63), (900, 64), (33, 65), (100, 1500), (0, 0), (2048 - 1024, 1025), (5, 255), (6, 256),
                 (7, 257), (2048, 1), (0, 2049), (300, 320), (41, 191)]
    assert any(a + c == nbins for a, c in bands)              # a band that ends at bin n_h / 2
    lo = np.array([[a for a, _ in bands], [a for a, _ in reversed(bands)]], dtype=np.int32)
    cnt = np.array([[c for _, c in bands], [c for _, c in reversed(bands)]], dtype=np.int32)
    nch, k = 3, 2
    spec = _random_spectra(rng, nch * k, nbins)
    got = _device_powers(eng, spec, lo, cnt)
    assert got.shape == (nch, k, len(bands))
    worst = 0.0
    for c in range(nch):
        want = R.band_powers(spec[k * c : k * c + k], lo, cnt)
        assert np.all(got[c][cnt == 0] == 0.0) and np.all(want[cnt == 0] == 0.0)
        rel = np.abs(got[c] - want)[cnt > 0] / want[cnt > 0]
        worst = max(worst, float(np.max(rel / ((cnt[cnt > 0] + 4) * U))))
        assert np.all(rel <= (cnt[cnt > 0] + 4) * U), (c, rel)
    print(f"n_h {n_h}: largest error {worst:.3f} of the bound (cnt + 4) 2^-53")
    # the same rows elsewhere in a larger batch: identical results
    order = [2, 0, 1, 0, 2]
    big = np.concatenate([spec[k * c : k * c + k] for c in order])
    again = _device_powers(eng, big, lo, cnt, lead=11)
    for i, c in enumerate(order):
        assert np.array_equal(again[i], got[c]), (i, c)


# ------------------------------------------------------------------------------------------------ 3: end to end
def test_end_to_end_against_the_restatement_and_the_analytic_values(signals):
    from audio_analysis_amd.analyse import harmonics as H
    from audio_analysis_amd.analyse.deconvolve import DeconvolveSettings, deconvolve_device
    eng = _eng()
    st = _settings()
    rec = eng.upload(list(signals["y"]))
    sw = eng.upload([signals["x"]])
    resp = deconvolve_device(eng, rec, [0, 0], sw, [0, 0], FS,
                             DeconvolveSettings(regularization_relative=st.regularization_relative, normalise_peak=False,
                                                remove_dc=False, output_length_mode="full_fft"))
    assert list(resp["n_fft"]) == [32768, 32768]
    res = H.harmonic_distortion_device(eng, rec, [0, 0], sw, [0, 0], FS, st, response=resp)
    h = resp["h"].cpu().numpy()
    results = H.harmonic_distortion_results(res, FS, ["left", "right"], st)
    worst = 0.0
    for c in range(2):
        hc = h[int(resp["off"][c]) : int(resp["off"][c]) + 32768]
        r = R.analyse(hc, FS, T, F1, F2, 3, 3)
        assert r["status"] == 0 and results[c].status == 0
        assert (results[c].peak_sample, results[c].window_samples, results[c].fft_size) == (r["p"], r["W"], r["n_h"])
        assert np.array_equal(res.plan.cnt > 0, r["cnt"] > 0) and np.array_equal(res.plan.lo, r["lo"])
        assert np.array_equal(np.isnan(np.array(results[c].hd)), np.isnan(r["hd"]))
        assert np.array_equal(np.isnan(np.array(results[c].thd)), np.isnan(r["thd"]))
        assert results[c].harmonics_counted == tuple(int(v) for v in r["counted"])
        e_ref, cnt = r["E"], r["cnt"]
        m = np.max(np.abs(r["spec"]), axis=1)[:, None]
        tol = 2.0 * np.sqrt(e_ref) * D_FFT * m + (D_FFT * m) ** 2 + (cnt + 4) * U * e_ref
        diff = np.abs(res.powers[c] - e_ref)
        assert np.all(res.powers[c][cnt == 0] == 0.0)
        worst = max(worst, float(np.max(diff[cnt > 0] / tol[cnt > 0])))
        assert np.all(diff[cnt > 0] <= tol[cnt > 0]), (c, diff / tol)
        _check_hd(results[c], PAIRS[c], f"channel {c}")
    print(f"band powers: largest error {worst:.3e} of the tolerance")
    # the default path (its own deconvolution) gives the same masks, peaks and, to the analytic condition, the same ratios
    own = H.analyse_harmonic_distortion_batch(list(signals["y"]), signals["x"], FS, ["left", "right"], st)
    for c in range(2):
        assert (own[c].status, own[c].peak_sample, own[c].fft_size) == (0, results[c].peak_sample, results[c].fft_size)
        _check_hd(own[c], PAIRS[c], f"channel {c}, own deconvolution")


# ------------------------------------------------------------------------------------------------ 4: the unmuted signal
def test_unmuted_signal_linear_peak_is_still_found(signals):
    from audio_analysis_amd.analyse import harmonics as H
    muted, unmuted = H.analyse_harmonic_distortion_batch([signals["y"][0], signals["unmuted"]], signals["x"], FS,
                                                         ["muted", "unmuted"], _settings())
    assert muted.status == 0 and unmuted.status == 0
    assert unmuted.peak_sample == muted.peak_sample == 0
    # without the restricted search the pick would have gone wrong: the restatement's response has its largest sample there
    h = R.deconvolve(signals["unmuted"], signals["x"]).astype(np.float32)
    assert int(np.argmax(np.abs(h))) >= R.search_length(32768, T, F1, F2, FS, 3, 64)
    _check_hd(unmuted, PAIRS[0], "unmuted")


# ------------------------------------------------------------------------------------------------ 5: degenerate inputs
def test_degenerate_inputs(signals):
    from audio_analysis_amd.analyse import harmonics as H
    silent, good = H.analyse_harmonic_distortion_batch([np.zeros(28800, np.float32), signals["y"][1]], signals["x"], FS,
                                                       ["silent", "good"], _settings())
    assert silent.status == H.STATUS_SILENT and good.status == 0
    assert all(math.isnan(v) for row in silent.hd for v in row) and all(math.isnan(v) for v in silent.thd)
    assert all(math.isnan(v) for v in silent.fundamental_db)
    _check_hd(good, PAIRS[1], "beside a silent channel")
    # a sweep declared four times slower: L fs ln 11 = 43447 samples do not fit the 32768-sample buffer, L fs ln 4 does
    short, = H.analyse_harmonic_distortion_batch([signals["y"][0]], signals["x"], FS, ["short"],
                                                 _settings(sweep_seconds=2.0, max_harmonic=10))
    assert short.status == H.STATUS_TOO_SHORT and len(short.hd) == 9 and all(math.isnan(v) for v in short.thd)
    fits, = H.analyse_harmonic_distortion_batch([signals["y"][0]], signals["x"], FS, ["fits"], _settings(sweep_seconds=2.0))
    assert fits.status == 0
    # a transform of more than 2^21 points: refused before anything is launched
    eng = _eng()
    eng.sync()
    eng.events = []
    try:
        with pytest.raises(ValueError, match=r"2\^21"):
            H.analyse_harmonic_distortion_batch([np.zeros((1 << 21) + 1, np.float32)], signals["x"], FS, ["long"], _settings())
        assert eng.events == []
    finally:
        eng.events = None


# ------------------------------------------------------------------------------------------------ 6: the command line
def test_command_line_matches_the_summariser_and_json_round_trips(signals, tmp_path):
    from scipy.io import wavfile
    from audio_analysis_amd.analyse import harmonics as H
    sweep, rec, out = tmp_path / "sweep.wav", tmp_path / "rec.wav", tmp_path / "out.json"
    wavfile.write(str(sweep), FS, signals["x"])
    wavfile.write(str(rec), FS, np.stack(signals["y"], axis=1))
    want = H.analyse_harmonic_distortion_from_wav_files([rec], sweep, _settings(), FS)
    assert [r.channel_name for r in want] == ["rec.wav:left", "rec.wav:right"] and all(r.status == 0 for r in want)
    for r, pair in zip(want, PAIRS):
        _check_hd(r, pair, r.channel_name)
    env = dict(os.environ, PYTHONPATH=str(REPO))
    run = subprocess.run([sys.executable, "-m", "analyse.harmonics", "--recorded", str(rec), "--sweep", str(sweep),
                          "--sweep-seconds", str(T), "--f1", str(F1), "--f2", str(F2), "--harmonics", "3", "--json", str(out)],
                         capture_output=True, text=True, cwd=str(REPO), env=env, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    assert run.stdout == H.summarise_harmonic_distortion_text(want)
    back = H.harmonic_results_from_json(json.loads(out.read_text()))
    assert H.summarise_harmonic_distortion_text(back) == run.stdout
    assert np.array_equal(np.array(back[0].hd), np.array(want[0].hd), equal_nan=True)
    assert np.array_equal(np.array(back[1].thd), np.array(want[1].thd), equal_nan=True)
    assert back[0].harmonics_counted == want[0].harmonics_counted
