"""
CPU-only tests of the frequency-dependent-window response (audio_analysis_amd.analyse.fdw): the restatement of
tests/fdw_ref.py against a float64 emulation and against closed forms, the grid builder at its edges, settings validation,
the host arithmetic on hand-built fields, the fixed text / Markdown / JSON formats, the command line, the host side of the
engine method on the recording engine, the argument checks of both C entry points (they return before touching a device),
the scratch size against its formula, and the header's constants.
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

import fdw_ref as R

REPO = Path(__file__).resolve().parent.parent
LD = np.longdouble


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("window", R.WINDOWS)
def test_float64_arithmetic_lies_inside_the_three_bounds(window):
    """The bounds are float64 arithmetic's own: the emulation (another order of the sums, NumPy's sine and cosine) stays
    inside all three, at five points from 20 Hz to 20 kHz of the default grid, whole windows and clipped ones (the last
    centre leaves three end terms, where the per-term share of the bound is all there is)."""
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(48000) * np.exp(-np.arange(48000) / 6000.0)).astype(np.float32)
    worst = 0.0
    for f, half in ((20.0, 10000), (200.0, 1800), (2000.0, 180), (9000.0, 40), (20000.0, 18)):
        for p in (24000, 5, 47990, -3, 48000 + half - 2):
            ref = R.reference(x, p, f / 48000.0, half, window)
            got = R.emulate64(x, p, f / 48000.0, half, window)
            assert ref["n"] == got[5] > 0
            worst = max(worst, R.worst_ratio(got, ref))
    print(f"float64 emulation, {window}: worst error / bound {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("window", R.WINDOWS)
def test_unit_impulse_closed_form(window):
    """x = delta at p + d: S0 = w(d) e^{-2 pi i rho d}, S1 = d S0, A = w(d), so the group delay is d samples."""
    n, p = 4100, 2050
    for half, rho in ((1, 0.5), (33, 0.1234567), (700, 1e-5), (700, 0.1234567), (1999, 0.31)):
        for d in (0, 1, -1, half, -half, half // 2):
            x = np.zeros(n, np.float32)
            x[p + d] = 1.0
            ref = R.reference(x, p, rho, half, window)
            # the weight as written, in long double: right to that format's ABSOLUTE rounding, which is all the literal form
            # keeps at the window's ends; the relative checks below take the restatement's own A = w(d)
            literal = R.literal_hann(d, half) if window == "hann" else LD(1)
            assert abs(ref["a"] - literal) <= LD(2.0) ** -61
            w = float(ref["a"])
            assert w > 0.0 and ref["n"] == 2 * half + 1
            want = w * np.exp(-2j * np.pi * ((rho * d) % 1.0))
            assert abs(complex(ref["re0"], ref["im0"]) - want) <= 1e-12 * w
            assert abs(complex(ref["re1"], ref["im1"]) - d * want) <= 1e-12 * w * max(abs(d), 1)
            assert abs(float(ref["a1"]) - abs(d) * w) <= 1e-15 * abs(d) * w
            delay = float((ref["re1"] * ref["re0"] + ref["im1"] * ref["im0"]) / (ref["re0"] ** 2 + ref["im0"] ** 2))
            assert abs(delay - d) <= 1e-9 * max(abs(d), 1)
            assert R.worst_ratio(R.emulate64(x, p, rho, half, window), ref) <= 1.0
    x = np.zeros(n, np.float32)
    x[p + 40] = 1.0                                            # outside the window: nothing
    ref = R.reference(x, p, 0.1, 39, window)
    assert ref["a"] == 0 and ref["re0"] == 0 and ref["n"] == 79


def test_rect_window_over_the_whole_channel_is_the_rfft():
    """rect, every sample inside the window, rho = m / n: S0 = rfft(x)[m] e^{+2 pi i m p / n}."""
    rng = np.random.default_rng(5)
    for n, p in ((256, 0), (256, 100), (1000, 999), (375, 17)):
        x = rng.standard_normal(n).astype(np.float32)
        spec = np.fft.rfft(x.astype(np.float64))
        scale = float(np.sum(np.abs(x)))
        for m in (1, 2, n // 5, n // 2):
            ref = R.reference(x, p, m / n, n, "rect")          # half = n reaches every sample from any centre
            assert ref["n"] == n
            want = spec[m] * np.exp(2j * np.pi * ((m * p) % n) / n)
            assert abs(complex(ref["re0"], ref["im0"]) - want) <= 1e-13 * scale
            assert R.worst_ratio(R.emulate64(x, p, m / n, n, "rect"), ref) <= 1.0


def test_restatement_edges():
    x = np.arange(1, 11, dtype=np.float32)
    for p, half, n in ((0, 3, 4), (9, 3, 4), (10, 3, 3), (10 + 3 + 3, 3, 0), (-2, 3, 2), (-4, 3, 0), (5, 100, 10)):
        ref = R.reference(x, p, 0.25, half, "hann")
        assert ref["n"] == n and R.emulate64(x, p, 0.25, half, "hann")[5] == n
        if n == 0:
            assert all(ref[q] == 0 for q in ("re0", "im0", "re1", "im1", "a", "a1"))
            assert not R.emulate64(x, p, 0.25, half, "hann").any()
    assert R.reference(np.zeros(0, np.float32), 0, 0.25, 5, "rect")["n"] == 0
    # a NaN inside the window makes the point non-finite, outside it is not read
    y = x.copy()
    y[7] = np.nan
    assert not np.isfinite(float(R.reference(y, 5, 0.1, 2, "hann")["re0"]))
    assert np.isfinite(float(R.reference(y, 4, 0.1, 2, "hann")["re0"]))
    assert R.worst_ratio(np.array([0.0, 0.0, 0.0, 0.0, 0.0, 3.0]), R.reference(np.zeros(3, np.float32), 1, 0.1, 1, "rect")) == 0.0
    assert R.worst_ratio(np.array([1e-300, 0.0, 0.0, 0.0, 0.0, 3.0]), R.reference(np.zeros(3, np.float32), 1, 0.1, 1, "rect")) == math.inf


# ------------------------------------------------------------------------------------------------ grid and settings
def test_default_grid_and_its_edges():
    from audio_analysis_amd.analyse import fdw as D
    f, rho, half = D.fdw_grid(D.FdwSettings(), 48000)
    assert f.size == 479 and f[0] == 20.0 and f[-1] <= 20000.0 < f[-1] * 2.0 ** (1 / 48)
    assert half.dtype == np.int32 and half[0] == 18000 and half[-1] == 18 and np.all(np.diff(half) <= 0)
    assert rho.dtype == np.float64 and np.array_equal(rho, f / 48000.0) and rho.max() <= 0.5
    assert np.array_equal(f, 20.0 * 2.0 ** (np.arange(479) / 48.0))
    assert np.array_equal(half, np.rint(15.0 * 48000 / (2.0 * f)).astype(np.int32))
    assert int(np.sum(2 * half.astype(np.int64) + 1)) == 2509009            # the terms of a channel at the defaults
    # f_max above Nyquist: the grid ends at fs / 2
    f, rho, half = D.fdw_grid(D.FdwSettings(f_max_hz=30000.0), 44100)
    assert f[-1] <= 22050.0 < f[-1] * 2.0 ** (1 / 48) and rho[-1] <= 0.5 and f.size == 486
    f, _, _ = D.fdw_grid(D.FdwSettings(f_min_hz=1000.0, f_max_hz=16000.0, points_per_octave=1), 32000)
    assert list(f) == [1000.0, 2000.0, 4000.0, 8000.0, 16000.0]                  # Nyquist itself is a point: rho = 0.5
    f, _, half = D.fdw_grid(D.FdwSettings(points_per_octave=1), 48000)
    assert list(f) == [20.0 * 2 ** j for j in range(10)] and list(half) == [18000, 9000, 4500, 2250, 1125, 562, 281, 141, 70, 35]
    # the clips bound the half width in samples
    _, _, half = D.fdw_grid(D.FdwSettings(min_window_ms=1.0, max_window_ms=100.0), 48000)
    assert half.max() == 4800 and half.min() == 48 and half[0] == 4800 and half[-1] == 48
    _, _, half = D.fdw_grid(D.FdwSettings(cycles=0.01), 48000)
    assert half.min() == 1 and half.max() == 12                                  # at least one sample to either side
    _, _, half = D.fdw_grid(D.FdwSettings(cycles=0.5, max_window_ms=0.001), 48000)
    assert np.all(half == 1)
    f, _, _ = D.fdw_grid(D.FdwSettings(f_min_hz=20.0, f_max_hz=20.0), 48000)
    assert list(f) == [20.0]
    for kw, fs, what in ((dict(f_min_hz=30000.0, f_max_hz=40000.0), 48000, "no frequency point"),
                         (dict(points_per_octave=500), 48000, "at most 4096"),
                         (dict(cycles=1000.0, f_min_hz=1.0, max_window_ms=1e6), 48000, "half width"),
                         (dict(), 0, "sample rate")):
        with pytest.raises(ValueError, match=what):
            D.fdw_grid(D.FdwSettings(**kw), fs)


def test_settings_defaults_and_validation():
    from audio_analysis_amd.analyse import fdw as D
    s = D.FdwSettings()
    assert (s.cycles, s.points_per_octave, s.f_min_hz, s.f_max_hz, s.window, s.min_window_ms, s.max_window_ms, s.centre,
            s.onset_db, s.magnitude_floor_db, s.use_mono_downmix_for_stereo) == \
        (15.0, 48, 20.0, 20000.0, "hann", 0.0, 500.0, "peak", -20.0, -120.0, False)
    assert s.rel_energy == 10.0 ** (-20.0 / 10.0)
    assert D.FdwSettings(cycles=3, window="rect", centre="onset", min_window_ms=2, max_window_ms=2).cycles == 3.0
    nan, inf = float("nan"), float("inf")
    bad = [(dict(cycles=0.0), "cycles"), (dict(cycles=-1.0), "cycles"), (dict(cycles=nan), "cycles"), (dict(cycles=inf), "cycles"),
           (dict(cycles="many"), "cycles"), (dict(points_per_octave=0), "points_per_octave"),
           (dict(points_per_octave=2.5), "points_per_octave"), (dict(points_per_octave=True), "points_per_octave"),
           (dict(f_min_hz=0.0), "f_min_hz"), (dict(f_min_hz=nan), "f_min_hz"), (dict(f_max_hz=inf), "f_max_hz"),
           (dict(f_min_hz=100.0, f_max_hz=50.0), "f_max_hz"), (dict(window="hamming"), "window must"),
           (dict(min_window_ms=-1.0), "min_window_ms"), (dict(min_window_ms=10.0, max_window_ms=5.0), "min_window_ms"),
           (dict(max_window_ms=0.0), "max_window_ms"), (dict(max_window_ms=nan), "max_window_ms"),
           (dict(centre="middle"), "centre must"), (dict(onset_db=1.0), "onset_db"), (dict(onset_db=nan), "onset_db"),
           (dict(magnitude_floor_db=inf), "magnitude_floor_db")]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            D.FdwSettings(**kw)


# ------------------------------------------------------------------------------------------------ host arithmetic
def test_host_arithmetic_on_hand_built_fields():
    from audio_analysis_amd.analyse import fdw as D
    nan, inf = float("nan"), float("inf")
    half = np.array([2, 2, 2, 2, 2, 2, 2])
    sums = np.array([[3.0, 4.0, 6.0, 8.0, 10.0, 5.0],          # |S0| = 5, S1 = 2 S0: two samples late
                     [0.0, -2.0, 0.0, 1.0, 2.0, 4.0],          # -90 degrees, half a sample early, clipped
                     [0.0, 0.0, 0.0, 0.0, 0.0, 5.0],           # S0 == 0
                     [nan, 1.0, 1.0, 1.0, 1.0, 5.0],           # non-finite
                     [1.0, 1.0, 1.0, 1.0, inf, 5.0],           # a non-finite A alone
                     [-1.0, -1e-9, 0.0, 0.0, 4.0, 5.0],        # just past -180 degrees: unwraps upwards
                     [-1e-9, 2e-10, 0.0, 0.0, 1.0, 0.0]])      # below the floor, near +169 degrees
    c = D.fdw_arithmetic(sums, half, 1000.0, -120.0)
    assert c["level_db"][0] == 10.0 * np.log10(25.0) and c["phase_deg"][0] == np.degrees(np.arctan2(4.0, 3.0))
    assert c["group_delay_seconds"][0] == (6.0 * 3.0 + 8.0 * 4.0) / 25.0 / 1000.0 == 0.002 and c["cancellation"][0] == 0.5
    assert c["phase_deg"][1] == -90.0 and c["group_delay_seconds"][1] == -0.0005 and c["cancellation"][1] == 1.0
    for name in ("level_db", "phase_deg", "unwrapped_phase_deg", "group_delay_seconds", "cancellation"):
        assert np.array_equal(np.isnan(c[name]), [False, False, True, True, True, False, False]), name
    assert list(c["clipped"]) == [False, True, False, False, False, False, True]
    assert np.all(c["window_ms"] == 5.0)
    assert c["level_db"][6] == -120.0 and c["level_db"][5] == 10.0 * np.log10(1.0 + 1e-18)
    # unwrapped along the points that have a value: 53.1, -90, -180 (just past it: +180 as a phase), then +169 continues as -191
    assert c["unwrapped_phase_deg"][0] == c["phase_deg"][0] and c["unwrapped_phase_deg"][1] == -90.0
    assert abs(c["unwrapped_phase_deg"][5] + 180.0) < 1e-6
    assert c["phase_deg"][6] == np.degrees(np.arctan2(2e-10, -1e-9)) and 168.0 < c["phase_deg"][6] < 169.0
    assert abs(c["unwrapped_phase_deg"][6] - (c["phase_deg"][6] - 360.0)) < 1e-9
    # records -> results, with and without the curves
    st = D.FdwSettings(points_per_octave=3)
    rec = D.FdwRecords(settings=st, frequencies_hz=np.arange(1.0, 8.0), rho=np.arange(1.0, 8.0) / 1000.0,
                       half=half.astype(np.int32), length=np.array([100, 0]), centre=np.array([7, 0]),
                       sums=np.stack([sums, np.zeros_like(sums)]))
    a, b = D.fdw_results(rec, 1000, ["a", "b"])
    assert (a.centre_samples, a.centre_seconds, a.centre, a.cycles, a.window, a.points_per_octave) == (7, 0.007, "peak", 15.0, "hann", 3)
    assert np.array_equal(a.level_db, c["level_db"], equal_nan=True) and a.half_samples.dtype == np.int64
    assert np.all(np.isnan(b.level_db)) and np.all(b.clipped) and b.centre_samples == 0
    assert D.fdw_results(rec, 1000, ["a", "b"], keep_curve=False)[0].level_db is None


def _hand_built():
    from audio_analysis_amd.analyse.fdw import FdwChannelResult
    nan = float("nan")
    ok = FdwChannelResult(
        channel_name="left", sample_rate_hz=48000, centre="peak", centre_samples=240, centre_seconds=0.005, cycles=15.0,
        window="hann", points_per_octave=2, frequencies_hz=np.array([20.0, 28.284, 40.0, 56.568, 80.0]),
        half_samples=np.array([18000, 12728, 9000, 6364, 4500]), window_ms=np.array([750.02083, 530.35417, 375.02083, 265.1875, 187.52083]),
        level_db=np.array([-3.25, -2.0, nan, -1.0, 0.125]), phase_deg=np.array([12.34, 0.0, nan, -170.0, 179.96]),
        unwrapped_phase_deg=np.array([12.34, 0.0, nan, -170.0, -180.04]),
        group_delay_seconds=np.array([0.0012345, 0.0, nan, -0.0001, 0.00005]),
        cancellation=np.array([0.91234, 0.5, nan, 0.25, 1.0]), clipped=np.array([True, True, True, False, False]))
    bare = FdwChannelResult(channel_name="right", sample_rate_hz=44100, centre="onset", centre_samples=0, centre_seconds=0.0,
                            cycles=7.5, window="rect", points_per_octave=48)
    return [ok, bare]


def test_summary_text_format_is_pinned():
    from audio_analysis_amd.analyse.fdw import summarise_fdw_text
    assert summarise_fdw_text(_hand_built()) == (
        "[left]\n"
        "Centre: peak at 240 samples (5.000 ms)  Window: hann 15 cycles  Points: 5 (2 per octave)\n"
        "freq_Hz  window_ms  level_dB  phase_deg  group_delay_ms  cancellation  clipped\n"
        "20.0  750.021  -3.25  12.3  1.234  0.9123  yes\n"
        "40.0  375.021  NA  NA  NA  NA  yes\n"
        "80.0  187.521  0.12  180.0  0.050  1.0000  no\n"
        "clipped points: 3, without a value: 1\n"
        "\n"
        "[right]\n"
        "Centre: onset at 0 samples (0.000 ms)  Window: rect 7.5 cycles  Points: NA (48 per octave)\n"
        "freq_Hz  window_ms  level_dB  phase_deg  group_delay_ms  cancellation  clipped\n"
        "\n")
    assert summarise_fdw_text([]) == ""


def test_summary_markdown_format_is_pinned():
    from audio_analysis_amd.analyse.fdw import summarise_fdw_markdown
    assert summarise_fdw_markdown(_hand_built()[:1]) == (
        "### left\n"
        "\n"
        "Centre: peak at 240 samples (5.000 ms). Window: hann 15 cycles. Points: 5 (2 per octave).\n"
        "\n"
        "| freq (Hz) | window (ms) | level (dB) | phase (deg) | group delay (ms) | cancellation | clipped |\n"
        "|---|---:|---:|---:|---:|---:|---:|\n"
        "| 20.0 | 750.021 | -3.25 | 12.3 | 1.234 | 0.9123 | yes |\n"
        "| 40.0 | 375.021 | NA | NA | NA | NA | yes |\n"
        "| 80.0 | 187.521 | 0.12 | 180.0 | 0.050 | 1.0000 | no |\n"
        "\n"
        "clipped points: 3, without a value: 1.\n"
        "\n")


def test_json_round_trip_keeps_nan_and_drops_the_curve_on_request():
    from audio_analysis_amd.analyse.fdw import fdw_results_from_json, fdw_results_to_json, summarise_fdw_text
    res = _hand_built()
    text = json.dumps(fdw_results_to_json(res), allow_nan=False)               # strict JSON: no NaN tokens
    doc = json.loads(text)
    rows = doc["fdw"]
    assert rows[0]["level_db"] == [-3.25, -2.0, None, -1.0, 0.125] and rows[0]["clipped"] == [True, True, True, False, False]
    assert rows[0]["half_samples"] == [18000, 12728, 9000, 6364, 4500]
    assert set(rows[0]) == {"channel_name", "sample_rate_hz", "centre", "centre_samples", "centre_seconds", "cycles", "window",
                            "points_per_octave", "frequencies_hz", "half_samples", "window_ms", "level_db", "phase_deg",
                            "unwrapped_phase_deg", "group_delay_seconds", "cancellation", "clipped"}
    assert set(rows[1]) == {"channel_name", "sample_rate_hz", "centre", "centre_samples", "centre_seconds", "cycles", "window",
                            "points_per_octave"}
    back = fdw_results_from_json(doc)
    assert summarise_fdw_text(back) == summarise_fdw_text(res) and fdw_results_to_json(back) == doc
    assert back[0].clipped.dtype == bool and back[0].half_samples.dtype == np.int64 and back[0].level_db.dtype == np.float64
    assert np.array_equal(back[0].group_delay_seconds, res[0].group_delay_seconds, equal_nan=True)
    assert back[1].level_db is None and back[1].centre == "onset" and back[1].cycles == 7.5
    slim = fdw_results_to_json(res, with_curve=False)
    assert all("level_db" not in r for r in slim["fdw"])
    assert fdw_results_from_json(json.loads(json.dumps(slim)))[0].frequencies_hz is None


def test_cli_parser_defaults_and_help_through_the_shim():
    import analyse.fdw as shim
    from audio_analysis_amd.analyse import fdw as D
    assert shim is D
    p = D.build_parser()
    a = p.parse_args(["--input", "a.wav", "b.wav"])
    assert a.input == [Path("a.wav"), Path("b.wav")] and a.bundle is None and a.mono is False and a.no_curve is False
    assert (a.expected_sample_rate, a.json) == (48000, None)
    assert D.settings_from_args(a) == D.FdwSettings()
    a = p.parse_args(["--bundle", "d", "--mono", "--cycles", "6", "--points-per-octave", "12", "--f-min", "50", "--f-max",
                      "10000", "--window", "rect", "--min-window-ms", "0.5", "--max-window-ms", "100", "--centre", "onset",
                      "--onset-db", "-30", "--no-curve", "--expected-sample-rate", "44100", "--json", "o.json"])
    assert D.settings_from_args(a) == D.FdwSettings(
        cycles=6.0, points_per_octave=12, f_min_hz=50.0, f_max_hz=10000.0, window="rect", min_window_ms=0.5,
        max_window_ms=100.0, centre="onset", onset_db=-30.0, use_mono_downmix_for_stereo=True)
    assert a.bundle == Path("d") and a.no_curve and a.expected_sample_rate == 44100 and a.json == Path("o.json")
    for bad in ([], ["--input", "a.wav", "--bundle", "d"], ["--input", "a.wav", "--window", "hamming"],
                ["--input", "a.wav", "--centre", "middle"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit):                                       # invalid settings end as a usage error
        D.main(["--input", "a.wav", "--cycles", "0"])
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.fdw", "--help"], capture_output=True, text=True, cwd=str(REPO), env=env,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--input", "--bundle", "--mono", "--cycles", "--points-per-octave", "--f-min", "--f-max", "--window",
                 "--min-window-ms", "--max-window-ms", "--centre", "--onset-db", "--no-curve", "--expected-sample-rate", "--json"):
        assert flag in r.stdout


# ------------------------------------------------------------------------------------------------ library and engine
def test_header_constants_symbols_and_abi_version():
    from audio_analysis_amd import _lib, build, engine
    from audio_analysis_amd.analyse import fdw as D
    hdr = (REPO / "include" / "ira.h").read_text()
    for name in ("FIELDS", "SUMS", "MAX_POINTS", "CHUNK", "NARROW_HALF"):
        assert re.search(rf"#define IRA_FDW_{name} {getattr(engine, 'FDW_' + name)}\b", hdr), name
    assert "#define IRA_FDW_MAX_HALF (1 << 20)" in hdr and engine.FDW_MAX_HALF == 1 << 20
    assert (engine.FDW_FIELDS, engine.FDW_SUMS, engine.FDW_MAX_POINTS, engine.FDW_CHUNK, engine.FDW_NARROW_HALF) == \
        (6, 5, 4096, 4096, 127)
    assert (D.MAX_POINTS, D.MAX_HALF_SAMPLES, D.WINDOWS, D.CENTRES) == (4096, 1 << 20, ("hann", "rect"), ("peak", "onset"))
    assert build.SOURCES["ira_fdw.hip"] == ["-ffp-contract=off"]
    assert "#define IRA_ABI_VERSION 15 " in hdr and _lib.ABI_VERSION == 15
    for name in ("ira_fdw_scratch_doubles", "ira_fdw_response"):
        assert name in _lib.PROTOTYPES and re.search(rf"int(32|64)_t {name}\(", hdr)
    lib = _lib.load()
    assert lib.ira_abi_version() == 15 and lib.ira_fdw_response is not None and lib.ira_fdw_scratch_doubles is not None


def _i32(values):
    return (ctypes.c_int32 * max(1, len(values)))(*values)


def _f64(values):
    return (ctypes.c_double * max(1, len(values)))(*values)


def test_scratch_size_follows_its_formula():
    from audio_analysis_amd import _lib, engine
    from audio_analysis_amd.analyse import fdw as D
    lib = _lib.load()
    C = engine.FDW_CHUNK
    assert list(engine.fdw_chunks([1, 127, 128, 1023, 1024, C // 2 - 1, C // 2, C + C // 2 + 5, 3 * C, 1 << 20])) == \
        [0, 0, 1, 1, 1, 1, 2, 4, 7, 513]
    for nch, half in ((1, [1]), (3, [127, 128]), (256, list(D.fdw_grid(D.FdwSettings(), 48000)[2])), (0, [5000]),
                      (2, [C // 2 - 1, C // 2, 3 * C, 1 << 20]), (65535, [4096] * 7), (5, [])):
        chunks = [0 if h <= 127 else -(-(2 * h + 1) // C) for h in half]
        total, narrow = sum(chunks), sum(1 for c in chunks if c == 0)
        want = nch * total * 5 + (len(half) + 1 + total + narrow + 1) // 2
        assert lib.ira_fdw_scratch_doubles(nch, _i32(half), len(half)) == want == engine.fdw_scratch_doubles(nch, half), (nch, half)
    half = list(D.fdw_grid(D.FdwSettings(), 48000)[2])
    assert sum(1 for h in half if h <= 127) == 136 and int(engine.fdw_chunks(half).sum()) == 817
    E_NULL, E_SIZE = -1, -2
    none = ctypes.POINTER(ctypes.c_int32)()
    assert lib.ira_fdw_scratch_doubles(1, none, 1) == E_NULL and lib.ira_fdw_scratch_doubles(1, none, 0) == 1
    for nch, half, npts in ((-1, [5], 1), (65536, [5], 1), (1, [5], -1), (1, [5] * 4097, 4097), (1, [0], 1),
                            (1, [(1 << 20) + 1], 1), (1, [5, -3], 2)):
        assert lib.ira_fdw_scratch_doubles(nch, _i32(half), npts) == E_SIZE, (nch, half[:2], npts)
    assert lib.ira_fdw_scratch_doubles(65535, _i32([1 << 20] * 4096), 4096) == 65535 * 4096 * 513 * 5 + (4097 + 4096 * 513 + 1) // 2


def test_entry_point_validates_arguments_without_gpu():
    from audio_analysis_amd import _lib
    lib = _lib.load()
    E_NULL, E_SIZE = -1, -2
    nan, inf = float("nan"), float("inf")

    def call(rho=(0.1, 0.5), half=(5, 4000), **kw):
        a = dict(x=1, off=1, len=1, centre=1, nch=0, rho_dev=1, half_dev=1, npts=len(half), window=0, scratch=1,
                 scratch_doubles=None, out=1, rho_null=False, half_null=False)
        a.update(kw)
        c_rho = ctypes.POINTER(ctypes.c_double)() if a["rho_null"] else _f64(rho)
        c_half = ctypes.POINTER(ctypes.c_int32)() if a["half_null"] else _i32(half)
        need = lib.ira_fdw_scratch_doubles(max(0, min(a["nch"], 65535)), _i32(half), len(half))
        size = need if a["scratch_doubles"] is None else a["scratch_doubles"]
        return lib.ira_fdw_response(a["x"], a["off"], a["len"], a["centre"], a["nch"], c_rho, c_half, a["rho_dev"],
                                    a["half_dev"], a["npts"], a["window"], a["scratch"], size, a["out"], 0)

    assert call() == 0 and call(window=1) == 0                             # nch == 0: nothing to do
    assert call(nch=3, npts=0, rho=(), half=()) == 0                       # no point: nothing to do
    for name in ("x", "off", "len", "centre", "rho_dev", "half_dev", "scratch", "out"):
        assert call(**{name: 0}) == E_NULL, name
    assert call(rho_null=True) == E_NULL and call(half_null=True) == E_NULL
    for kw in (dict(nch=-1), dict(nch=65536), dict(npts=-1), dict(window=2), dict(window=-1),
               dict(half=(0, 4000)), dict(half=(5, (1 << 20) + 1)), dict(half=(5, -1)),
               dict(rho=(0.0, 0.5)), dict(rho=(0.1, 0.5000001)), dict(rho=(-0.1, 0.5)), dict(rho=(nan, 0.5)),
               dict(rho=(0.1, inf)), dict(rho=[0.1] * 4097, half=[5] * 4097)):
        assert call(**kw) == E_SIZE, kw
    assert call(half=(1, 1 << 20)) == 0 and call(rho=(5e-324, 0.5)) == 0 and call(rho=[0.1] * 4096, half=[5] * 4096) == 0
    # the scratch is checked before any launch, and everything is refused before any launch with channels present
    need = lib.ira_fdw_scratch_doubles(2, _i32([5, 4000]), 2)
    assert need == 2 * 2 * 5 + (3 + 2 + 1 + 1) // 2
    assert call(nch=2, scratch_doubles=need - 1) == E_SIZE and call(nch=0, scratch_doubles=0) == E_SIZE
    assert call(nch=2, half=(0, 4000)) == E_SIZE and call(nch=2, x=0) == E_NULL and call(nch=2, window=3) == E_SIZE
    assert call(nch=2, rho=(0.1, 0.6)) == E_SIZE


def test_fdw_device_is_one_launch_over_every_channel():
    """The host side of fdw_device and Engine.fdw_response on the recording engine: one ira_fdw_response call whose tables
    hold the channels' offsets and lengths and the grid, the peak or the onset as the centre, the scratch size."""
    from host_engine import HostEngine
    from audio_analysis_amd import engine
    from audio_analysis_amd.analyse import fdw as D
    from audio_analysis_amd.synth import synth_ir
    eng = HostEngine()
    lens = [6000, 500, 0, 7001]
    batch = eng.upload([synth_ir(i, 0, n, 48000) if n else np.zeros(0, np.float32) for i, n in enumerate(lens)])
    res = D.fdw_device(eng, batch, 48000, D.FdwSettings())
    f, rho, half = D.fdw_grid(D.FdwSettings(), 48000)
    assert len(eng.calls("ira_onset_index")) == 1
    calls = eng.calls("ira_fdw_response")
    assert len(calls) == 1 and calls[0][0] == "ira_fdw_response[hann]"
    (x, off, ln, centre, nch, c_rho, c_half, rho_dev, half_dev, npts, window, scratch, scratch_doubles, out, stream) = calls[0][1]
    assert (nch, npts, window, stream) == (4, 479, 0, None)
    assert c_rho == tuple(rho) and c_half == tuple(int(h) for h in half)
    assert list(eng.table(off)[:4]) == list(batch.off) and list(eng.table(ln)[:4]) == lens
    assert np.array_equal(eng.table(rho_dev)[:479], rho) and np.array_equal(eng.table(half_dev)[:479], half)
    assert rho_dev[1] == "<f8" and half_dev[1] == "<i4"
    assert scratch_doubles == engine.fdw_scratch_doubles(4, half) == 4 * 817 * 5 + (480 + 817 + 136 + 1) // 2
    assert scratch[:3] == ("empty", scratch_doubles, "torch.float64") and out[:3] == ("empty", 4 * 479 * 6, "torch.float64")
    onset_args = eng.calls("ira_onset_index")[0][1]
    assert centre == onset_args[5] and centre[0] == "empty" and x[0] == "up"   # centre peak: the peak index of the onset call
    assert res.sums.shape == (4, 479, 6) and list(res.length) == lens and res.centre.shape == (4,) and np.array_equal(res.half, half)
    res = D.fdw_device(eng, batch, 48000, D.FdwSettings(centre="onset", window="rect", points_per_octave=3, f_max_hz=1000.0))
    name, args = eng.calls("ira_fdw_response")[1]
    assert name == "ira_fdw_response[rect]" and args[10] == 1 and args[9] == 17 and args[3] == eng.calls("ira_onset_index")[1][1][8]
    assert res.sums.shape == (4, 17, 6)
    # an empty batch launches nothing
    n_before = len(eng.calls("ira_fdw_response"))
    res = D.fdw_device(eng, eng.upload([]), 48000, D.FdwSettings())
    assert len(eng.calls("ira_fdw_response")) == n_before and res.sums.shape == (0, 479, 6)
    assert eng.fdw_response(batch.x, batch.off, batch.length, batch.off_dev, [], [], "hann").shape == (4, 0, 6)
    good = dict(rho=[0.1, 0.2], half=[3, 300], window="hann")
    for bad, what in ((dict(window="hamming"), "window"), (dict(rho=[0.1]), "rho and half"), (dict(rho=[0.1, 0.0]), "rho"),
                      (dict(rho=[0.1, 0.51]), "rho"), (dict(rho=[0.1, float("nan")]), "rho"), (dict(half=[3, 0]), "half"),
                      (dict(half=[3, 2.5]), "half"), (dict(half=[3, (1 << 20) + 1]), "half"),
                      (dict(rho=[0.1] * 4097, half=[3] * 4097), "at most 4096")):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError, match=what):
            eng.fdw_response(batch.x, batch.off, batch.length, batch.off_dev, **kw)
    with pytest.raises(ValueError, match="off and length"):
        eng.fdw_response(batch.x, batch.off, batch.length[:2], batch.off_dev, **good)
