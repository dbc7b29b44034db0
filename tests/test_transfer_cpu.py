"""
CPU-only tests of the dual-channel transfer function (audio_analysis_amd.analyse.transfer): the NumPy restatement against
SciPy, frame counts, settings validation, the text / Markdown / JSON formats on hand-built results, the command line's
parser, the host side of the device function on the recording engine, the argument checks of the two C entry points
(they return before touching a device) and the ABI version.
"""
import ctypes
import json
import math
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import transfer_ref as R

REPO = Path(__file__).resolve().parent.parent


def test_reference_agrees_with_scipy_welch():
    """White noise through a short FIR plus independent noise: coherence and H1 of the restatement against
    scipy.signal.coherence and csd / welch with the same window array, noverlap and no detrending, to 1e-10 relative."""
    try:
        from scipy import signal
    except Exception as e:                                              # pragma: no cover
        pytest.skip(f"scipy.signal does not import: {e}")
    rng = np.random.default_rng(11)
    for n_fft, overlap, name in ((1024, 0.5, "hann"), (256, 0.75, "rect"), (512, 0.0, "hann")):
        hop = R.hop_of(n_fft, overlap)
        x = rng.standard_normal(20 * n_fft + 123).astype(np.float32)
        y = (np.convolve(x, [0.5, 0.3, -0.2, 0.1])[: x.size] + 0.3 * rng.standard_normal(x.size)).astype(np.float32)
        win = R.window(n_fft, name)
        X, Y, _ = R.frame_spectra(x, y, 0, n_fft, hop, win)
        sxx, syy, sxy = R.sums(X, Y)
        rows = dict(zip(R.ROWS, R.derived(sxx, syy, sxy.real, sxy.imag)))
        kw = dict(fs=1.0, window=win, nperseg=n_fft, noverlap=n_fft - hop, nfft=n_fft, detrend=False)
        _, coh = signal.coherence(x.astype(np.float64), y.astype(np.float64), **kw)
        _, pxy = signal.csd(x.astype(np.float64), y.astype(np.float64), **kw)
        _, pxx = signal.welch(x.astype(np.float64), **kw)
        h1 = pxy / pxx
        got = rows["h1_re"] + 1j * rows["h1_im"]
        e_h = float(np.max(np.abs(got - h1) / np.abs(h1)))
        e_c = float(np.max(np.abs(rows["coherence"] - coh) / coh))
        print(f"n_fft {n_fft} {name} hop {hop}: K {X.shape[0]}, H1 {e_h:.2e}, coherence {e_c:.2e} (bound 1e-10)")
        assert X.shape[0] == 1 + (x.size - n_fft) // hop
        assert e_h <= 1e-10 and e_c <= 1e-10


def test_counts_for_every_sign_of_the_delay():
    from audio_analysis_amd.analyse import transfer as T
    from audio_analysis_amd.engine import xspec_frames
    assert [T.TransferSettings(n_fft=n, overlap=o).hop for n, o in
            ((4096, 0.5), (1024, 0.75), (256, 0.0), (256, 0.999), (1024, 0.3), (8192, 0.5))] == [2048, 256, 256, 1, 717, 4096]
    for n, o in ((4096, 0.5), (1024, 0.3), (256, 0.999)):
        assert T.TransferSettings(n_fft=n, overlap=o).hop == R.hop_of(n, o) == max(1, n - math.floor(o * n + 0.5))
    # (Lx, Ly, d) -> (x skip, y skip, N)
    for (lx, ly, d), want in (((1000, 900, 0), (0, 0, 900)), ((1000, 900, 5), (0, 5, 895)), ((1000, 900, -7), (7, 0, 900)),
                              ((1000, 2000, -7), (7, 0, 993)), ((1000, 1000, 300), (0, 300, 700)),
                              ((10, 10, 50), (0, 50, 0)), ((10, 10, -50), (50, 0, 0))):
        assert tuple(int(v) for v in T.pair_geometry(lx, ly, d)) == want == R.geometry(lx, ly, d)
    n_fft, hop = 256, 37
    for n, k in ((256, 1), (255, 0), (0, 0), (256 + 36, 1), (256 + 37, 2), (256 + 15 * 37, 16), (256 + 16 * 37 - 1, 16)):
        assert int(T.frame_count(n, n_fft, hop)) == k == R.frames(n, n_fft, hop) == int(xspec_frames(np.array([n]), n_fft, hop)[0])
    assert list(T.frame_count([4096, 4095, 4096 + 2048, 3 * 4096], 4096, 2048)) == [1, 0, 2, 5]


def test_settings_defaults_and_validation():
    from audio_analysis_amd.analyse.transfer import TransferSettings
    s = TransferSettings()
    assert (s.n_fft, s.overlap, s.window, s.delay, s.band_hz, s.coherence_threshold, s.points_per_octave,
            s.use_mono_downmix_for_stereo, s.hop, s.use_hann) == (4096, 0.5, "hann", "auto", (20.0, 20000.0), 0.5, 3, False, 2048, True)
    assert TransferSettings(delay=-7, band_hz=[100, 200], window="rect").band_hz == (100.0, 200.0)
    assert TransferSettings(delay=np.int64(5)).delay == 5 and not TransferSettings(window="rect").use_hann
    for bad, what in [(dict(n_fft=128), "n_fft"), (dict(n_fft=16384), "n_fft"), (dict(n_fft=3000), "n_fft"),
                      (dict(n_fft=4096.0), "n_fft"), (dict(overlap=1.0), "overlap"), (dict(overlap=-0.1), "overlap"),
                      (dict(overlap=float("nan")), "overlap"), (dict(overlap="half"), "overlap"),
                      (dict(window="hamming"), "window"), (dict(delay="none"), "delay"), (dict(delay=1.5), "delay"),
                      (dict(delay=True), "delay"), (dict(band_hz=(200.0, 100.0)), "band_hz"), (dict(band_hz=100.0), "band_hz"),
                      (dict(band_hz=(-1.0, 100.0)), "band_hz"), (dict(coherence_threshold=1.5), "coherence_threshold"),
                      (dict(coherence_threshold=float("nan")), "coherence_threshold"),
                      (dict(points_per_octave=0), "points_per_octave"), (dict(points_per_octave=49), "points_per_octave"),
                      (dict(points_per_octave=2.5), "points_per_octave")]:
        with pytest.raises(ValueError, match=what):
            TransferSettings(**bad)


def test_octave_grid_and_band_rows_from_sums():
    from audio_analysis_amd.analyse import transfer as T
    grid = T.octave_grid((20.0, 20000.0), 3)
    assert len(grid) == 29 and grid[16][0] == 1000.0 and abs(grid[0][0] - 24.803) < 1e-3 and abs(grid[-1][0] - 16000.0) < 1e-9
    assert all(abs(b / a - 2.0 ** (1.0 / 3.0)) < 1e-12 for _, a, b in grid)
    assert [c for c, _, _ in T.octave_grid((500.0, 2000.0), 1)] == [500.0, 1000.0, 2000.0]
    # hand-built sums: H = 0.5 exp(i pi/2) everywhere, coherence 0.64, one pair too short, one silent, one non-finite
    n_fft, nb = 256, 129
    sxx = np.full(nb, 4.0)
    out = np.zeros((4, 11, nb))
    out[0] = R.derived(sxx, np.full(nb, 1.5625), np.zeros(nb), np.full(nb, 2.0))
    out[2] = R.derived(np.zeros(nb), np.ones(nb), np.zeros(nb), np.zeros(nb))
    out[3] = out[0]
    out[3, 1, 7] = np.inf
    res = T.TransferSums(n_fft=n_fft, hop=128, window="hann", delay=np.array([3, 0, 0, -2]), samples=np.array([1000, 255, 900, 900]),
                         frames=np.array([6, 0, 6, 6]), out=out)
    st = T.TransferSettings(n_fft=n_fft, band_hz=(1000.0, 8000.0), points_per_octave=1, coherence_threshold=0.6)
    r = T.transfer_results(res, 48000, ["a", "b", "c", "d"], st)
    assert [x.status for x in r] == [0, T.STATUS_TOO_SHORT, T.STATUS_SILENT_REFERENCE, T.STATUS_NON_FINITE]
    assert r[0].mean_coherence == pytest.approx(0.64, abs=1e-15) and r[0].coherent_fraction == 1.0
    assert [b.centre_hz for b in r[0].rows] == [1000.0, 2000.0, 4000.0, 8000.0]
    for b in r[0].rows:
        assert b.bins == np.count_nonzero((r[0].frequency_hz >= b.low_edge_hz) & (r[0].frequency_hz < b.high_edge_hz))
        assert b.mag_db == pytest.approx(20.0 * math.log10(0.5), abs=1e-12) and b.phase_rad == pytest.approx(math.pi / 2)
        assert b.coherence == pytest.approx(0.64, abs=1e-15)
    assert r[0].arrays["h1_im"][5] == 0.5 and r[0].arrays["mag_db"][5] == pytest.approx(20.0 * math.log10(0.5), abs=1e-13)
    assert (r[0].delay_samples, r[0].samples, r[0].frames, r[3].delay_samples) == (3, 1000, 6, -2)
    for x in r[1:]:
        assert math.isnan(x.mean_coherence) and math.isnan(x.coherent_fraction)
        assert all(np.all(np.isnan(x.arrays[k])) for k in T.ARRAYS)
        assert all(math.isnan(b.mag_db) and math.isnan(b.coherence) for b in x.rows) and len(x.rows) == 4
    assert T.TransferSettings(coherence_threshold=0.7).coherence_threshold == 0.7
    r7 = T.transfer_results(res, 48000, ["a"], T.TransferSettings(n_fft=n_fft, coherence_threshold=0.7))
    assert r7[0].coherent_fraction == 0.0


def _hand_built():
    from audio_analysis_amd.analyse import transfer as T
    nan = float("nan")
    nb = 129
    arrays = {k: np.linspace(0.0, 1.0, nb) * (i + 1) for i, k in enumerate(T.ARRAYS)}
    arrays["h2_re"] = arrays["h2_re"].copy()
    arrays["h2_re"][0] = nan
    arrays["mag_db"] = arrays["mag_db"].copy()
    arrays["mag_db"][0] = -math.inf
    ok = T.TransferPairResult(
        pair_name="a.wav:left", sample_rate_hz=48000, n_fft=256, hop=128, window="hann", delay_samples=-300, samples=96000,
        frames=749, status=0, band_hz=(20.0, 20000.0), coherence_threshold=0.5, mean_coherence=0.98765, coherent_fraction=0.75,
        rows=(T.TransferBandRow(1000.0, 890.9, 1122.5, 2, -12.0412, math.pi / 4, 0.9994), T.TransferBandRow(31.25, 27.8, 35.1, 0, nan, nan, nan)),
        arrays=arrays)
    bad = T.TransferPairResult(
        pair_name="b.wav:mono", sample_rate_hz=48000, n_fft=256, hop=256, window="rect", delay_samples=0, samples=255, frames=0,
        status=2, band_hz=(20.0, 20000.0), coherence_threshold=0.5, mean_coherence=nan, coherent_fraction=nan, rows=(),
        arrays={k: np.full(nb, nan) for k in T.ARRAYS})
    return [ok, bad]


def test_summary_text_and_markdown_formats_are_pinned():
    from audio_analysis_amd.analyse.transfer import summarise_transfer_markdown, summarise_transfer_text
    assert summarise_transfer_text(_hand_built()) == (
        "[a.wav:left]\n"
        "Delay: -300 samples (-6.250 ms)  Frames: 749 of 256 (hann, hop 128)  Mean coherence 20-20000 Hz: 0.988  "
        "Bins at or above 0.5: 75.0 %  Status: ok\n"
        "Hz  Mag_dB  Phase_deg  Coherence  Bins\n"
        "1000.0  -12.04  45.0  0.999  2\n"
        "31.2  NA  NA  NA  0\n"
        "\n"
        "[b.wav:mono]\n"
        "Delay: 0 samples (0.000 ms)  Frames: 0 of 256 (rect, hop 256)  Mean coherence 20-20000 Hz: NA  "
        "Bins at or above 0.5: NA %  Status: 2 (too short)\n"
        "Hz  Mag_dB  Phase_deg  Coherence  Bins\n"
        "\n")
    assert summarise_transfer_text([]) == ""
    assert summarise_transfer_markdown(_hand_built()[:1]) == (
        "### a.wav:left\n"
        "\n"
        "Delay: -300 samples (-6.250 ms). Frames: 749 of 256 (hann, hop 128). Mean coherence 20-20000 Hz: 0.988. "
        "Bins at or above 0.5: 75.0 %. Status: ok.\n"
        "\n"
        "| Hz | Mag (dB) | Phase (deg) | Coherence | Bins |\n"
        "|---|---:|---:|---:|---:|\n"
        "| 1000.0 | -12.04 | 45.0 | 0.999 | 2 |\n"
        "| 31.2 | NA | NA | NA | 0 |\n"
        "\n")


def test_json_round_trip_carries_the_arrays_with_nan_as_null():
    from audio_analysis_amd.analyse import transfer as T
    res = _hand_built()
    text = json.dumps(T.transfer_results_to_json(res))
    assert "NaN" not in text and "Infinity" not in text                  # strict JSON
    doc = json.loads(text)
    rows = doc["transfer"]
    assert rows[0]["arrays"]["h2_re"][0] is None and rows[0]["arrays"]["mag_db"][0] == "-inf"
    assert rows[1]["mean_coherence"] is None and rows[1]["arrays"]["sxx"] == [None] * 129 and rows[1]["rows"] == []
    assert len(rows[0]["frequency_hz"]) == 129 and rows[0]["frequency_hz"][1] == 187.5 and rows[0]["rows"][1]["mag_db"] is None
    back = T.transfer_results_from_json(doc)
    assert T.summarise_transfer_text(back) == T.summarise_transfer_text(res)
    for b, r in zip(back, res):
        for f in ("pair_name", "sample_rate_hz", "n_fft", "hop", "window", "delay_samples", "samples", "frames", "status",
                  "band_hz", "coherence_threshold"):
            assert getattr(b, f) == getattr(r, f), f
        for k in T.ARRAYS:
            np.testing.assert_array_equal(b.arrays[k], r.arrays[k])      # NaN == NaN here, bit-exact otherwise
        assert len(b.rows) == len(r.rows)
    assert back[0].rows[0] == res[0].rows[0] and math.isnan(back[0].rows[1].coherence) and back[0].mean_coherence == 0.98765
    assert T.transfer_results_to_json(back) == T.transfer_results_to_json(res)


def test_cli_parser_defaults_and_help():
    from audio_analysis_amd.analyse import transfer as T
    p = T.build_parser()
    a = p.parse_args(["--measured", "a.wav", "b.wav", "--reference", "s.wav"])
    assert a.measured == [Path("a.wav"), Path("b.wav")] and a.reference == Path("s.wav") and a.input is None
    assert (a.mono, a.n_fft, a.overlap, a.window, a.delay, a.points_per_octave, a.coherence_threshold, a.expected_sample_rate,
            a.json, a.reference_channel) == (False, 4096, 0.5, "hann", "auto", 3, 0.5, 48000, None, None)
    assert T.settings_from_args(a) == T.TransferSettings()
    a = p.parse_args(["--input", "st.wav", "--reference-channel", "right", "--n-fft", "1024", "--overlap", "0.75", "--window",
                      "rect", "--delay", "-300", "--points-per-octave", "6", "--coherence-threshold", "0.8",
                      "--expected-sample-rate", "44100", "--json", "o.json"])
    s = T.settings_from_args(a)
    assert a.input == [Path("st.wav")] and a.reference_channel == "right" and a.expected_sample_rate == 44100 and a.json == Path("o.json")
    assert (s.n_fft, s.overlap, s.window, s.delay, s.points_per_octave, s.coherence_threshold, s.hop) == (1024, 0.75, "rect", -300, 6, 0.8, 256)
    for bad in ([], ["--measured", "a.wav", "--input", "b.wav"], ["--measured", "a.wav", "--reference", "s.wav", "--window", "kaiser"],
                ["--measured", "a.wav", "--reference", "s.wav", "--delay", "soon"],
                ["--input", "a.wav", "--reference-channel", "centre"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    for bad in (["--measured", "a.wav"], ["--input", "a.wav"], ["--input", "a.wav", "--reference", "s.wav"],
                ["--measured", "a.wav", "--reference", "s.wav", "--reference-channel", "left"],
                ["--measured", "a.wav", "--reference", "s.wav", "--n-fft", "1000"],
                ["--measured", "a.wav", "--reference", "s.wav", "--overlap", "1"]):
        with pytest.raises(SystemExit):                                   # a source without its partner, invalid settings
            T.main(bad)
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.transfer", "--help"], capture_output=True, text=True, cwd=str(REPO),
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--measured", "--reference", "--mono", "--input", "--reference-channel", "--n-fft", "--overlap", "--window",
                 "--delay", "--points-per-octave", "--coherence-threshold", "--expected-sample-rate", "--json"):
        assert flag in r.stdout


def test_shim_re_exports_the_module():
    import analyse.transfer as shim
    from audio_analysis_amd.analyse import transfer
    assert shim is transfer


def test_transfer_device_is_one_accumulate_and_one_finish_per_batch():
    """The host side of transfer_device on the recording engine: a ragged batch of three pairs that share one reference
    row, with per-pair delays of every sign."""
    from host_engine import HostEngine
    from audio_analysis_amd.analyse import transfer as T
    eng = HostEngine()
    rng = np.random.default_rng(3)
    lens = [5000, 4000, 5200, 1030]
    batch = eng.upload([rng.standard_normal(n).astype(np.float32) for n in lens])
    st = T.TransferSettings(n_fft=1024, overlap=0.5, window="rect", delay=0)
    res = T.transfer_device(eng, batch, [0, 0, 0], [1, 2, 3], 48000, st, delays=[5, -7, 0])
    acc, fin = eng.calls("ira_xspec_accumulate"), eng.calls("ira_xspec_finish")
    assert len(acc) == 1 and len(fin) == 1 and acc[0][0] == "ira_xspec_accumulate[1024]"
    x, xo, yo, n, npairs, max_frames, n_fft, hop, win, tw, partial, stream = acc[0][1]
    # N = min(Lx - max(0, -d), Ly - max(0, d)): 3995, 4993, 1030;  K = 1 + (N - 1024) // 512: 6, 8, 1
    assert (npairs, max_frames, n_fft, hop) == (3, 8, 1024, 512)
    assert list(eng.table(n)[:3]) == [3995, 4993, 1030] and list(res.samples) == [3995, 4993, 1030] and list(res.frames) == [6, 8, 1]
    assert list(eng.table(xo)[:3]) == [0, 7, 0] and list(eng.table(yo)[:3]) == [5000 + 5, 9000, 14200]
    assert x[:3] == ("up", "<f4", (sum(lens),)) and win[:3] == ("up", "<f8", (1024,)) and tw[:3] == ("up", "<f8", (512, 2))
    assert np.all(eng.table(win)[:1024] == 1.0)
    assert partial[:2] == ("empty", 3 * 1 * 4 * 513)                       # ceil(8 / 16) = 1 chunk of the longest pair
    p2, n2, npairs2, max_frames2, n_fft2, hop2, out, _ = fin[0][1]
    assert p2 == partial and n2 == n and (npairs2, max_frames2, n_fft2, hop2) == (3, 8, 1024, 512)
    assert out[:2] == ("empty", 3 * 11 * 513) and res.out.shape == (3, 11, 513) and list(res.delay) == [5, -7, 0]
    # more frames than one chunk; the Hann table; an integer delay from the settings
    st = T.TransferSettings(n_fft=256, overlap=0.75, delay=2)
    res = T.transfer_device(eng, batch, [0, 1], [1, 0], 48000, st)
    args = eng.calls("ira_xspec_accumulate")[1][1]
    assert args[4:8] == (2, 1 + (4000 - 256) // 64, 256, 64) and args[10][:2] == ("empty", 2 * 4 * 4 * 129)   # 59 frames: 4 chunks
    assert np.array_equal(eng.table(args[8])[:256], np.hanning(256)) and list(eng.table(args[3])[:2]) == [3998, 4000]
    assert len(eng.calls("ira_xspec_finish")) == 2
    # an empty batch launches nothing
    res = T.transfer_device(eng, batch, [], [], 48000, st)
    assert res.out.shape == (0, 11, 129) and len(eng.calls("ira_xspec_accumulate")) == 2
    with pytest.raises(ValueError, match="index the batch"):
        T.transfer_device(eng, batch, [0], [4], 48000, st)
    with pytest.raises(ValueError, match="one delay per pair"):
        T.transfer_device(eng, batch, [0], [1], 48000, st, delays=[1, 2])
    with pytest.raises(ValueError, match="inside x_dev"):
        eng.cross_spectra(batch.x, np.array([0]), np.array([sum(lens) - 10]), np.array([300]), 256, 64, True)
    with pytest.raises(ValueError, match="n_fft"):
        eng.cross_spectra(batch.x, np.array([0]), np.array([0]), np.array([300]), 300, 64, True)
    with pytest.raises(ValueError, match="hop"):
        eng.cross_spectra(batch.x, np.array([0]), np.array([0]), np.array([300]), 256, 257, True)


def test_auto_delay_is_deconvolution_and_a_peak_pick_on_the_recording_engine():
    from host_engine import HostEngine
    from audio_analysis_amd.analyse import transfer as T
    eng = HostEngine()
    rng = np.random.default_rng(4)
    batch = eng.upload([rng.standard_normal(n).astype(np.float32) for n in (3000, 2500, 4100)])
    d = T.find_delay_device(eng, batch, [0, 0], [1, 2], 48000)
    assert d.shape == (2,) and d.dtype == np.int64
    assert len(eng.calls("ira_deconv_divide")) == 1 and len(eng.calls("ira_peak_index")) == 1
    fin = eng.calls("ira_deconv_finish")[0][1]
    assert fin[7:9] == (0, 0)                                              # no DC removal, no peak normalisation
    pk = eng.calls("ira_peak_index")[0][1]
    assert list(eng.table(pk[2])[:2]) == [4096, 8192] and pk[3] == 2       # the full transforms
    big = eng.upload([np.zeros(8, np.float32), np.zeros((1 << 21) + 1, np.float32)])
    with pytest.raises(ValueError, match="2\\^21"):
        T.find_delay_device(eng, big, [0], [1], 48000)


def test_xspec_entry_points_validate_arguments_without_gpu():
    from audio_analysis_amd import _lib
    lib = _lib.load()
    E_NULL, E_SIZE = -1, -2

    def acc(**kw):
        a = dict(x=1, xo=1, yo=1, n=1, npairs=0, max_frames=10, n_fft=4096, hop=2048, win=1, tw=1, partial=1)
        a.update(kw)
        return lib.ira_xspec_accumulate(a["x"], a["xo"], a["yo"], a["n"], a["npairs"], a["max_frames"], a["n_fft"], a["hop"],
                                        a["win"], a["tw"], a["partial"], 0)

    def fin(**kw):
        a = dict(partial=1, n=1, npairs=0, max_frames=10, n_fft=4096, hop=2048, out=1)
        a.update(kw)
        return lib.ira_xspec_finish(a["partial"], a["n"], a["npairs"], a["max_frames"], a["n_fft"], a["hop"], a["out"], 0)

    for name in ("x", "xo", "yo", "n", "win", "tw", "partial"):
        assert acc(**{name: 0}) == E_NULL, name
        assert acc(**{name: 0, "npairs": 1}) == E_NULL, name
    for name in ("partial", "n", "out"):
        assert fin(**{name: 0}) == E_NULL, name
    for call in (acc, fin):
        assert call() == 0                                               # an empty batch: nothing to do
        for n_fft in (256, 512, 1024, 2048, 4096, 8192):
            assert call(n_fft=n_fft, hop=1) == 0 and call(n_fft=n_fft, hop=n_fft) == 0
            assert call(n_fft=n_fft, hop=n_fft + 1) == E_SIZE
        for n_fft in (0, -4096, 128, 16384, 4095, 4097, 3 * 1024):
            assert call(n_fft=n_fft, hop=1) == E_SIZE, n_fft
        for kw in (dict(hop=0), dict(hop=-1), dict(npairs=-1), dict(npairs=65536), dict(max_frames=-1)):
            assert call(**kw) == E_SIZE, kw
        assert call(max_frames=0) == 0
    assert acc(npairs=1, n_fft=100) == E_SIZE and acc(npairs=1, hop=0) == E_SIZE     # refused before any launch
    assert acc(npairs=1, max_frames=0) == 0                               # no frames anywhere: nothing to accumulate


def test_abi_version_is_15_everywhere():
    from audio_analysis_amd import _lib, engine
    hdr = (REPO / "include" / "ira.h").read_text()
    assert re.search(r"#define IRA_ABI_VERSION 15\b", hdr)
    assert _lib.ABI_VERSION == 15 and _lib.load().ira_abi_version() == 15
    assert f"#define IRA_XSPEC_FRAMES {engine.XSPEC_FRAMES}" in hdr and f"#define IRA_XSPEC_ROWS {engine.XSPEC_ROWS}" in hdr
    assert engine.XSPEC_FRAMES == R.FRAMES_PER_CHUNK and engine.XSPEC_ROWS == len(R.ROWS)
    for name in ("ira_xspec_accumulate", "ira_xspec_finish"):
        assert name in _lib.PROTOTYPES and re.search(rf"int32_t {name}\(", hdr)
    assert hdr.count("replace no reference function") >= 2
    src = (REPO / "audio_analysis_amd" / "build.py").read_text()
    assert '"ira_xspec.hip"' in src
