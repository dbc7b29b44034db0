"""
CPU-only tests of the burst-decay map (audio_analysis_amd.analyse.burstdecay): the grid and the step table against
hand-computed values, settings validation, the host arithmetic on hand-built sums, the text and JSON formats, the command
line's parser, the host side of the device function on the recording engine, the argument checks of the C entry points
(they return before touching a device), the header's constants, and a float64 emulation of the table form against the
long-double restatement (tests/burstdecay_ref.py, tests/fdw_ref.py) within the bounds the device is held to.
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

import burstdecay_ref as B
import fdw_ref as R

REPO = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------ grid, axis, settings
def test_default_grid_and_steps_at_three_sample_rates():
    from audio_analysis_amd.analyse import burstdecay as D
    st = D.BurstDecaySettings()
    f, rho, half, t, delta = D.burst_grid(st, 48000)
    assert f.size == 240 and f[0] == 20.0 and np.array_equal(f, 20.0 * 2.0 ** (np.arange(240) / 24.0))
    assert half.dtype == np.int32 and half[0] == 9600 and half[-1] == 10 and half[24] == 4800
    assert np.array_equal(rho, f / 48000.0) and int(np.sum(2 * half.astype(np.int64) + 1)) == 674024
    assert t.size == 61 and t[0] == 0.0 and t[1] == 0.5 and t[-1] == 30.0
    assert delta.dtype == np.int32 and delta.shape == (240, 61) and not delta[:, 0].any()
    assert list(delta[0, :4]) == [0, 1200, 2400, 3600] and delta[0, -1] == 72000 == np.abs(delta).max()
    assert list(delta[24, :3]) == [0, 600, 1200]                           # 40 Hz
    assert list(delta[-1, :4]) == [0, 1, 2, 4]                             # 19893.7 Hz: 1.206, 2.413, 3.619 samples
    assert int(np.sum((2 * half.astype(np.int64) + 1) * 61)) == 41115464   # the terms of a channel at the defaults
    assert np.all(np.diff(delta.astype(np.int64), axis=1) >= 0)
    # 44.1 kHz: 0.5 periods of 20 Hz are 1102.5 samples, 1.5 periods 3307.5: rint goes to the even neighbour
    f, rho, half, t, delta = D.burst_grid(st, 44100)
    assert f.size == 240 and half[0] == 8820 and list(delta[0, :4]) == [0, 1102, 2205, 3308] and delta[0, -1] == 66150
    f, rho, half, t, delta = D.burst_grid(st, 96000)
    assert f.size == 240 and half[0] == 19200 and half[-1] == 19 and delta[0, 1] == 2400 and delta[0, -1] == 144000
    # the ms axis: the same steps for every point
    ms = D.BurstDecaySettings(axis="ms")
    f, rho, half, t, delta = D.burst_grid(ms, 48000)
    assert t.size == 151 and t[-1] == 300.0 and np.array_equal(delta, np.broadcast_to(96 * np.arange(151), (240, 151)))
    f, rho, half, t, delta = D.burst_grid(ms, 44100)
    assert list(delta[7, :6]) == [0, 88, 176, 265, 353, 441] and delta[0, -1] == 13230
    # a negative start: pre-ringing
    f, rho, half, t, delta = D.burst_grid(D.BurstDecaySettings(start=-2.0, stop=1.0, step=0.25, points_per_octave=1), 48000)
    assert t.size == 13 and t[0] == -2.0 and list(delta[0, :3]) == [-4800, -4200, -3600] and delta[0, 8] == 0
    with pytest.raises(ValueError, match="samples from the centre"):
        D.burst_grid(D.BurstDecaySettings(stop=4000.0, step=1.0, f_min_hz=1.0, max_window_ms=10.0), 192000)


def test_step_count_where_the_step_does_not_divide_the_span():
    from audio_analysis_amd.analyse import burstdecay as D
    for kw, m in ((dict(), 61), (dict(axis="ms"), 151), (dict(start=0.0, stop=1.0, step=0.3), 4),
                  (dict(start=0.0, stop=0.3 * 3, step=0.3), 4),           # 0.8999999999999999 / 0.3: the 1e-9 keeps the step
                  (dict(start=-2.0, stop=10.0, step=0.1), 121), (dict(start=0.0, stop=0.0), 1),
                  (dict(start=1.0, stop=2.0, step=5.0), 1), (dict(axis="ms", stop=10.0, step=3.0), 4),
                  (dict(start=0.0, stop=4095.0, step=1.0), 4096)):
        st = D.BurstDecaySettings(**kw)
        assert st.steps == m, kw
        start, stop, step = st.axis_range
        t = D.burst_grid(D.BurstDecaySettings(points_per_octave=1, f_min_hz=1000.0, **kw), 48000)[3]
        assert t.size == m and t[0] == start and t[-1] <= stop + 1e-9 * step < t[-1] + step * (1 + 1e-9)


def test_settings_defaults_and_validation():
    from audio_analysis_amd.analyse import burstdecay as D
    s = D.BurstDecaySettings()
    assert (s.cycles, s.points_per_octave, s.f_min_hz, s.f_max_hz, s.window, s.min_window_ms, s.max_window_ms, s.centre,
            s.onset_db, s.axis, s.start, s.stop, s.step, s.decay_db, s.magnitude_floor_db, s.use_mono_downmix_for_stereo) == \
        (8.0, 24, 20.0, 20000.0, "hann", 0.0, 500.0, "peak", -20.0, "periods", None, None, None, 30.0, -120.0, False)
    assert s.axis_range == (0.0, 30.0, 0.5) and D.BurstDecaySettings(axis="ms", step=1).axis_range == (0.0, 300.0, 1.0)
    assert s.rel_energy == 10.0 ** (-20.0 / 10.0) and D.BurstDecaySettings(cycles=3, start=-1).start == -1.0
    nan, inf = float("nan"), float("inf")
    bad = [(dict(cycles=0.0), "cycles"), (dict(cycles=nan), "cycles"), (dict(cycles="many"), "cycles"),
           (dict(points_per_octave=0), "points_per_octave"), (dict(points_per_octave=2.5), "points_per_octave"),
           (dict(f_min_hz=0.0), "f_min_hz"), (dict(f_min_hz=100.0, f_max_hz=50.0), "f_max_hz"),
           (dict(window="hamming"), "window must"), (dict(min_window_ms=-1.0), "min_window_ms"),
           (dict(max_window_ms=0.0), "max_window_ms"), (dict(centre="middle"), "centre must"), (dict(onset_db=1.0), "onset_db"),
           (dict(axis="cycles"), "axis must"), (dict(step=0.0), "step"), (dict(step=-1.0), "step"), (dict(step=nan), "step"),
           (dict(start=inf), "start"), (dict(stop="late"), "stop"), (dict(start=5.0, stop=4.0), "stop must"),
           (dict(stop=5000.0, step=1.0), "at most 4096"), (dict(decay_db=0.0), "decay_db"), (dict(decay_db=nan), "decay_db"),
           (dict(magnitude_floor_db=inf), "magnitude_floor_db")]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            D.BurstDecaySettings(**kw)


# ------------------------------------------------------------------------------------------------ host arithmetic
def _level(db):
    return 10.0 ** (db / 20.0)


def test_host_arithmetic_decay_crossing_and_nan_rules():
    from audio_analysis_amd.analyse import burstdecay as D
    nan, inf = float("nan"), float("inf")
    t = np.array([0.0, 0.5, 1.0, 1.5, 2.0])
    f = np.array([100.0, 200.0, 400.0, 800.0, 1600.0, 3200.0])
    half = np.array([4, 4, 4, 4, 4, 4])
    delta = np.broadcast_to(np.array([0, 5, 10, 15, 20]), (6, 5))
    s = np.zeros((6, 5, 2))
    s[0, :, 0] = [_level(-10), _level(0), _level(-20), _level(-40), _level(-50)]   # maximum at 0.5, -30 dB between 1.0 and 1.5
    s[1, :, 1] = [_level(0), _level(-5), _level(-10), _level(-15), _level(-29.99)]  # never 30 dB down
    s[2, :, 0] = [_level(-50), _level(-40), _level(-30), _level(-20), _level(-3)]   # the maximum at the last step
    s[3, :, 0] = [1.0, nan, 0.0, _level(-60), 1e-9]                                 # a non-finite cell, a silent one, the floor
    s[3, 1, 1] = 1.0
    s[4, :, 0] = [inf, 0.0, nan, 0.0, 0.0]                                          # no cell has a value
    s[5, :, 0] = [-1.0, 0.0, 0.0, 0.0, 0.0]
    s[5, :, 1] = [0.0, -_level(-30), 0.0, 0.0, 0.0]                                 # exactly 30 dB down at the next step
    v = D.burst_arithmetic(s, half, delta, f, t, "periods", 10, 30, decay_db=30.0, magnitude_floor_db=-120.0)
    lv = v["level_db"]
    assert lv.shape == (6, 5) and abs(lv[0, 1]) < 1e-12 and abs(lv[0, 3] + 40.0) < 1e-12
    assert lv[0, 0] == 10.0 * np.log10(max(s[0, 0, 0] ** 2 + 0.0, 1e-12))
    assert np.array_equal(np.isnan(lv), np.isnan(v["phase_deg"])) and np.array_equal(np.isnan(lv), np.isnan(v["relative_db"]))
    assert list(np.isnan(lv[3])) == [False, True, True, False, False] and np.isnan(lv[4]).all()
    assert list(np.isnan(lv[5])) == [False, False, True, True, True]
    assert lv[3, 4] == -120.0 and abs(lv[3, 3] + 60.0) < 1e-12                      # the floor holds the level, not the cell
    assert v["phase_deg"][1, 0] == 90.0 and v["phase_deg"][5, 0] == 180.0 and v["phase_deg"][5, 1] == -90.0
    top = np.nanmax(lv)
    assert np.array_equal(v["relative_db"], lv - top, equal_nan=True) and np.nanmax(v["relative_db"]) == 0.0
    # decay: row 0 crosses -30 dB between t = 1.0 (-20 dB) and t = 1.5 (-40 dB): halfway
    assert abs(v["decay_periods"][0] - 1.25) < 1e-12 and abs(v["decay_seconds"][0] - 1.25 / 100.0) < 1e-15
    assert v["peak_position"][0] == 0.5 and abs(v["peak_level_db"][0]) < 1e-12
    assert math.isnan(v["decay_periods"][1]) and math.isnan(v["decay_seconds"][1]) and v["peak_position"][1] == 0.0
    assert math.isnan(v["decay_periods"][2]) and v["peak_position"][2] == 2.0 and abs(v["peak_level_db"][2] + 3.0) < 1e-12
    # row 3: 0 dB at t = 0, the next cell WITH A VALUE is t = 1.5 at -60 dB: -30 dB halfway between them
    assert abs(v["decay_periods"][3] - 0.75) < 1e-12
    assert math.isnan(v["decay_periods"][4]) and math.isnan(v["peak_level_db"][4]) and math.isnan(v["peak_position"][4])
    assert abs(v["decay_periods"][5] - 0.5) < 1e-9
    # clipped: c = 10 + delta, H = 4, L = 30: 6 .. 14 | .. | 26 .. 34 is cut at the end
    assert np.array_equal(v["clipped"], np.broadcast_to([False, False, False, False, True], (6, 5)))
    assert np.array_equal(D.terms_inside(10, delta[:1], half[:1], 30), [[9, 9, 9, 9, 4]])
    assert np.array_equal(D.terms_inside(-3, [[0, 2, 40]], [4], 30), [[2, 4, 0]])
    assert np.array_equal(D.terms_inside(0, [[0]], [4], 0), [[0]])
    # the ms axis reports the same crossing in seconds, periods through f
    w = D.burst_arithmetic(s, half, delta, f, t, "ms", 10, 30)
    assert abs(w["decay_seconds"][0] - 1.25e-3) < 1e-18 and abs(w["decay_periods"][0] - 1.25e-3 * 100.0) < 1e-15
    assert np.array_equal(w["level_db"], lv, equal_nan=True)
    with pytest.raises(ValueError, match="axis"):
        D.burst_arithmetic(s, half, delta, f, t, "cycles", 10, 30)


def _hand_built():
    from audio_analysis_amd.analyse.burstdecay import BurstDecayChannelResult
    nan = float("nan")
    full = BurstDecayChannelResult(
        channel_name="left", sample_rate_hz=48000, centre="peak", centre_samples=240, centre_seconds=0.005, cycles=8.0,
        window="hann", points_per_octave=2, axis="periods", decay_db=30.0, axis_values=np.array([0.0, 0.5, 1.0]),
        frequencies_hz=np.array([20.0, 28.284, 40.0]), half_samples=np.array([9600, 6788, 4800]),
        peak_level_db=np.array([-3.25, nan, 0.125]), peak_position=np.array([0.5, nan, 0.0]),
        decay_periods=np.array([12.345, nan, 7.0]), decay_seconds=np.array([0.61725, nan, 0.175]),
        level_db=np.array([[-5.0, -3.25, -9.0], [nan, nan, nan], [0.125, -1.0, nan]]),
        relative_db=np.array([[-5.125, -3.375, -9.125], [nan, nan, nan], [0.0, -1.125, nan]]),
        phase_deg=np.array([[0.0, 90.0, -179.5], [nan, nan, nan], [12.5, -3.0, nan]]),
        clipped=np.array([[True, True, False], [True, False, False], [False, False, False]]))
    bare = BurstDecayChannelResult(
        channel_name="right", sample_rate_hz=44100, centre="onset", centre_samples=0, centre_seconds=0.0, cycles=6.5,
        window="rect", points_per_octave=1, axis="ms", decay_db=20.0, axis_values=np.array([-2.0, 0.0]),
        frequencies_hz=np.array([1000.0]), half_samples=np.array([143]), peak_level_db=np.array([-0.5]),
        peak_position=np.array([0.0]), decay_periods=np.array([nan]), decay_seconds=np.array([nan]))
    return [full, bare]


def test_summary_text_format_is_pinned():
    from audio_analysis_amd.analyse.burstdecay import summarise_burst_decay_text
    assert summarise_burst_decay_text(_hand_built()) == (
        "[left]\n"
        "Centre: peak at 240 samples (5.000 ms)  Window: hann 8 cycles  Points: 3 (2 per octave)  Axis: periods 0 .. 1, 3 steps  Decay: -30 dB\n"
        "freq_Hz  window_ms  peak_dB  peak_at  decay_periods  decay_ms  clipped_cells\n"
        "20.0  400.021  -3.25  0.50  12.35  617.250  2\n"
        "40.0  200.021  0.12  0.00  7.00  175.000  0\n"
        "points that reach the decay: 2 of 3\n"
        "\n"
        "[right]\n"
        "Centre: onset at 0 samples (0.000 ms)  Window: rect 6.5 cycles  Points: 1 (1 per octave)  Axis: ms -2 .. 0, 2 steps  Decay: -20 dB\n"
        "freq_Hz  window_ms  peak_dB  peak_at  decay_periods  decay_ms  clipped_cells\n"
        "1000.0  6.508  -0.50  0.00  NA  NA  NA\n"
        "points that reach the decay: 0 of 1\n"
        "\n")
    assert summarise_burst_decay_text([]) == ""


def test_json_round_trip_keeps_nan_and_drops_the_map_on_request():
    from audio_analysis_amd.analyse.burstdecay import (burst_decay_results_from_json, burst_decay_results_to_json,
                                                       summarise_burst_decay_text)
    res = _hand_built()
    doc = json.loads(json.dumps(burst_decay_results_to_json(res), allow_nan=False))   # strict JSON: no NaN tokens
    rows = doc["burst_decay"]
    assert rows[0]["level_db"][1] == [None, None, None] and rows[0]["clipped"][0] == [True, True, False]
    assert rows[0]["decay_periods"] == [12.345, None, 7.0] and rows[0]["half_samples"] == [9600, 6788, 4800]
    point = {"channel_name", "sample_rate_hz", "centre", "centre_samples", "centre_seconds", "cycles", "window",
             "points_per_octave", "axis", "decay_db", "axis_values", "frequencies_hz", "half_samples", "peak_level_db",
             "peak_position", "decay_periods", "decay_seconds"}
    assert set(rows[0]) == point | {"level_db", "relative_db", "phase_deg", "clipped"} and set(rows[1]) == point
    back = burst_decay_results_from_json(doc)
    assert summarise_burst_decay_text(back) == summarise_burst_decay_text(res) and burst_decay_results_to_json(back) == doc
    assert back[0].clipped.dtype == bool and back[0].clipped.shape == (3, 3) and back[0].half_samples.dtype == np.int64
    assert np.array_equal(back[0].phase_deg, res[0].phase_deg, equal_nan=True) and back[1].level_db is None
    assert back[1].axis == "ms" and back[1].decay_db == 20.0 and list(back[1].axis_values) == [-2.0, 0.0]
    slim = burst_decay_results_to_json(res, with_map=False)
    assert all("level_db" not in r and "decay_seconds" in r for r in slim["burst_decay"])
    assert burst_decay_results_from_json(json.loads(json.dumps(slim)))[0].level_db is None


def test_cli_parser_defaults_no_map_and_help_through_the_shim():
    import analyse.burstdecay as shim
    from audio_analysis_amd.analyse import burstdecay as D
    assert shim is D
    p = D.build_parser()
    a = p.parse_args(["--input", "a.wav", "b.wav"])
    assert a.input == [Path("a.wav"), Path("b.wav")] and a.bundle is None and a.mono is False and a.no_map is False
    assert (a.expected_sample_rate, a.json, a.start, a.stop, a.step) == (48000, None, None, None, None)
    assert D.settings_from_args(a) == D.BurstDecaySettings()
    a = p.parse_args(["--bundle", "d", "--mono", "--cycles", "6", "--points-per-octave", "12", "--f-min", "50", "--f-max",
                      "10000", "--window", "rect", "--min-window-ms", "0.5", "--max-window-ms", "100", "--axis", "ms",
                      "--start", "-5", "--stop", "50", "--step", "0.5", "--centre", "onset", "--onset-db", "-30",
                      "--decay-db", "20", "--no-map", "--expected-sample-rate", "44100", "--json", "o.json"])
    assert D.settings_from_args(a) == D.BurstDecaySettings(
        cycles=6.0, points_per_octave=12, f_min_hz=50.0, f_max_hz=10000.0, window="rect", min_window_ms=0.5,
        max_window_ms=100.0, centre="onset", onset_db=-30.0, axis="ms", start=-5.0, stop=50.0, step=0.5, decay_db=20.0,
        use_mono_downmix_for_stereo=True)
    assert a.bundle == Path("d") and a.no_map and a.expected_sample_rate == 44100 and a.json == Path("o.json")
    for bad in ([], ["--input", "a.wav", "--bundle", "d"], ["--input", "a.wav", "--window", "hamming"],
                ["--input", "a.wav", "--axis", "cycles"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit):                                       # invalid settings end as a usage error
        D.main(["--input", "a.wav", "--step", "0"])
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.burstdecay", "--help"], capture_output=True, text=True, cwd=str(REPO),
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--input", "--bundle", "--mono", "--cycles", "--points-per-octave", "--f-min", "--f-max", "--window",
                 "--min-window-ms", "--max-window-ms", "--axis", "--start", "--stop", "--step", "--centre", "--onset-db",
                 "--decay-db", "--no-map", "--expected-sample-rate", "--json"):
        assert flag in r.stdout


# ------------------------------------------------------------------------------------------------ library and engine
def test_header_constants_symbols_and_abi_version():
    from audio_analysis_amd import _lib, build, engine
    from audio_analysis_amd.analyse import burstdecay as D
    hdr = (REPO / "include" / "ira.h").read_text()
    for name in ("STEPS", "LANES", "CHANNELS", "MAX_STEPS"):
        assert re.search(rf"#define IRA_BURST_{name} {getattr(engine, 'BURST_' + name)}\b", hdr), name
    assert "#define IRA_BURST_MAX_DELTA (1 << 24)" in hdr and engine.BURST_MAX_DELTA == 1 << 24 >= 72000
    assert (engine.BURST_STEPS, engine.BURST_LANES, engine.BURST_CHANNELS, engine.BURST_MAX_STEPS) == (8, 64, 4, 4096)
    assert (D.MAX_STEPS, D.MAX_DELTA_SAMPLES, D.AXES) == (4096, 1 << 24, ("periods", "ms"))
    assert build.SOURCES["ira_burstdecay.hip"] == ["-ffp-contract=off"]
    assert "#define IRA_ABI_VERSION 15 " in hdr and _lib.ABI_VERSION == 15
    for name in ("ira_burst_table_doubles", "ira_burst_table", "ira_burst_decay"):
        assert name in _lib.PROTOTYPES and re.search(rf"int(32|64)_t {name}\(", hdr)
    declared = set(re.findall(r"\b(ira_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_lib.PROTOTYPES)
    lib = _lib.load()
    assert lib.ira_abi_version() == 15 and lib.ira_burst_table is not None and lib.ira_burst_decay is not None


def _i32(values):
    return (ctypes.c_int32 * max(1, len(values)))(*values)


def _f64(values):
    return (ctypes.c_double * max(1, len(values)))(*values)


def test_table_size_follows_its_formula():
    from audio_analysis_amd import _lib, engine
    from audio_analysis_amd.analyse import burstdecay as D
    lib = _lib.load()
    default = list(D.burst_grid(D.BurstDecaySettings(), 48000)[2])
    for half in ([1], [127, 128], default, [1 << 20] * 4096, []):
        want = 2 * sum(2 * h + 1 for h in half)
        assert lib.ira_burst_table_doubles(_i32(half), len(half)) == want == engine.burst_table_doubles(half), half[:3]
    assert engine.burst_table_doubles(default) == 2 * 674024
    assert list(engine.burst_table_offsets([1, 2, 3, 10])) == [0, 3, 8, 15] and engine.burst_table_offsets([]).size == 0
    assert engine.burst_channels_per_call(240, 61) == (256 << 20) // (16 * 240 * 61) == 1145
    assert engine.burst_channels_per_call(4096, 4096) == 1 and engine.burst_channels_per_call(1, 1) == 65535
    E_NULL, E_SIZE = -1, -2
    none = ctypes.POINTER(ctypes.c_int32)()
    assert lib.ira_burst_table_doubles(none, 1) == E_NULL and lib.ira_burst_table_doubles(none, 0) == 0
    for half, npts in (([5], -1), ([5] * 4097, 4097), ([0], 1), ([(1 << 20) + 1], 1), ([5, -3], 2)):
        assert lib.ira_burst_table_doubles(_i32(half), npts) == E_SIZE, (half[:2], npts)


def test_entry_points_validate_arguments_without_gpu():
    from audio_analysis_amd import _lib
    lib = _lib.load()
    E_NULL, E_SIZE = -1, -2
    nan, inf = float("nan"), float("inf")

    def table(rho=(0.1, 0.5), half=(5, 4000), **kw):
        a = dict(rho_dev=1, half_dev=1, tab_off=1, npts=len(half), window=0, table=1, doubles=None, rho_null=False,
                 half_null=False)
        a.update(kw)
        c_rho = ctypes.POINTER(ctypes.c_double)() if a["rho_null"] else _f64(rho)
        c_half = ctypes.POINTER(ctypes.c_int32)() if a["half_null"] else _i32(half)
        need = 2 * sum(2 * h + 1 for h in half)
        return lib.ira_burst_table(c_rho, c_half, a["rho_dev"], a["half_dev"], a["tab_off"], a["npts"], a["window"],
                                   a["table"], need if a["doubles"] is None else a["doubles"], 0)

    assert table(npts=0) == 0 and table(npts=0, window=1) == 0              # no point: nothing to do
    for name in ("rho_dev", "half_dev", "tab_off", "table"):
        assert table(**{name: 0}) == E_NULL, name
    assert table(rho_null=True) == E_NULL and table(half_null=True) == E_NULL
    for kw in (dict(npts=-1), dict(window=2), dict(window=-1), dict(half=(0, 4000)), dict(half=(5, (1 << 20) + 1)),
               dict(rho=(0.0, 0.5)), dict(rho=(0.1, 0.5000001)), dict(rho=(nan, 0.5)), dict(rho=(0.1, inf)),
               dict(rho=[0.1] * 4097, half=[5] * 4097), dict(doubles=2 * (11 + 8001) - 1), dict(doubles=0)):
        assert table(**kw) == E_SIZE, kw

    def decay(half=(5, 4000), delta=((0, 0, 3), (-7, 2, 9)), **kw):
        nsteps = len(delta[0]) if len(delta) else 0
        a = dict(x=1, off=1, len=1, centre=1, nch=0, half_dev=1, tab_off=1, table=1, doubles=None, delta_dev=1,
                 npts=len(half), nsteps=nsteps, out=1, half_null=False, delta_null=False)
        a.update(kw)
        c_half = ctypes.POINTER(ctypes.c_int32)() if a["half_null"] else _i32(half)
        c_delta = ctypes.POINTER(ctypes.c_int32)() if a["delta_null"] else _i32([d for row in delta for d in row])
        need = 2 * sum(2 * h + 1 for h in half)
        return lib.ira_burst_decay(a["x"], a["off"], a["len"], a["centre"], a["nch"], c_half, a["half_dev"], a["tab_off"],
                                   a["table"], need if a["doubles"] is None else a["doubles"], c_delta, a["delta_dev"],
                                   a["npts"], a["nsteps"], a["out"], 0)

    assert decay() == 0                                                     # nch == 0: nothing to do
    assert decay(nch=3, npts=0, half=(), delta=()) == 0 and decay(nch=3, nsteps=0) == 0
    for name in ("x", "off", "len", "centre", "half_dev", "tab_off", "table", "delta_dev", "out"):
        assert decay(**{name: 0}) == E_NULL, name
    assert decay(half_null=True) == E_NULL and decay(delta_null=True) == E_NULL
    big = 1 << 24
    for kw in (dict(nch=-1), dict(nch=65536), dict(npts=-1), dict(nsteps=-1), dict(nsteps=4097),
               dict(half=(0, 4000)), dict(half=(5, (1 << 20) + 1)), dict(half=[5] * 4097, delta=[(0,)] * 4097),
               dict(delta=((0, 0, 3), (-7, 9, 8))), dict(delta=((1, 0, 3), (-7, 2, 9))), dict(delta=((0, 0, big + 1), (0, 0, 0))),
               dict(delta=((0, 0, 0), (-big - 1, 0, 0))), dict(doubles=2 * (11 + 8001) - 1), dict(doubles=0)):
        assert decay(**kw) == E_SIZE, kw
    assert decay(delta=((-big, 0, big), (5, 5, 5))) == 0 and decay(delta=[tuple(range(4096))] * 2) == 0
    # everything is refused before any launch with channels present
    assert decay(nch=2, half=(0, 4000)) == E_SIZE and decay(nch=2, x=0) == E_NULL and decay(nch=2, doubles=5) == E_SIZE
    assert decay(nch=2, delta=((0, 3, 2), (0, 0, 0))) == E_SIZE and decay(nch=65536) == E_SIZE


def test_burst_decay_device_is_one_table_call_and_one_map_call(monkeypatch):
    """The host side of burst_decay_device and the two Engine methods on the recording engine."""
    from host_engine import HostEngine
    from audio_analysis_amd import engine
    from audio_analysis_amd.analyse import burstdecay as D
    from audio_analysis_amd.synth import synth_ir
    eng = HostEngine()
    lens = [6000, 500, 0, 7001, 33]
    batch = eng.upload([synth_ir(i, 0, n, 48000) if n else np.zeros(0, np.float32) for i, n in enumerate(lens)])
    res = D.burst_decay_device(eng, batch, 48000, D.BurstDecaySettings())
    f, rho, half, t, delta = D.burst_grid(D.BurstDecaySettings(), 48000)
    assert len(eng.calls("ira_onset_index")) == 1
    tables, maps = eng.calls("ira_burst_table"), eng.calls("ira_burst_decay")
    assert len(tables) == 1 and len(maps) == 1 and tables[0][0] == "ira_burst_table[hann]" and maps[0][0] == "ira_burst_decay[hann]"
    (c_rho, c_half, rho_dev, half_dev, off_dev, npts, window, table, doubles, stream) = tables[0][1]
    assert (npts, window, doubles, stream) == (240, 0, 2 * 674024, None) and c_rho == tuple(rho) and c_half == tuple(int(h) for h in half)
    assert np.array_equal(eng.table(rho_dev)[:240], rho) and np.array_equal(eng.table(half_dev)[:240], half)
    assert np.array_equal(eng.table(off_dev)[:240], engine.burst_table_offsets(half)) and off_dev[1] == "<i8"
    assert table[:3] == ("empty", 2 * 674024, "torch.float64")
    (x, off, ln, centre, nch, m_half, m_half_dev, m_off_dev, m_table, m_doubles, c_delta, delta_dev, m_npts, nsteps, out,
     stream) = maps[0][1]
    assert (nch, m_npts, nsteps, m_doubles, stream) == (5, 240, 61, 2 * 674024, None)
    assert m_half == c_half and m_half_dev == half_dev and m_off_dev == off_dev and m_table == table
    assert c_delta == tuple(int(d) for d in delta.reshape(-1)) and delta_dev[1] == "<i4"
    assert np.array_equal(eng.table(delta_dev)[: delta.size], delta.reshape(-1))
    assert list(eng.table(off)[:5]) == list(batch.off) and list(eng.table(ln)[:5]) == lens
    assert out[:3] == ("empty", 5 * 240 * 61 * 2, "torch.float64") and x[0] == "up"
    assert centre == eng.calls("ira_onset_index")[0][1][5] and centre[0] == "empty"   # centre peak: the onset call's peak index
    assert res.sums.shape == (5, 240, 61, 2) and list(res.length) == lens and res.centre.shape == (5,)
    assert np.array_equal(res.delta, delta) and np.array_equal(res.axis_values, t) and np.array_equal(res.half, half)
    # a map larger than the stated constant is cut into calls of whole channels; the table is still made once
    monkeypatch.setattr(engine, "BURST_MAX_OUT_BYTES", 2 * 16 * 240 * 151 + 5)
    st = D.BurstDecaySettings(axis="ms", centre="onset", window="rect")
    res = D.burst_decay_device(eng, batch, 48000, st)
    maps = eng.calls("ira_burst_decay")[1:]
    assert len(eng.calls("ira_burst_table")) == 2 and [m[1][4] for m in maps] == [2, 2, 1] and maps[0][0] == "ira_burst_decay[rect]"
    assert [m[1][14][1] for m in maps] == [2 * 240 * 151 * 2, 2 * 240 * 151 * 2, 240 * 151 * 2]
    assert [m[1][1][-1] for m in maps] == [maps[0][1][1][-1] + 16 * i for i in range(3)]   # the offsets table from channel 0, 2, 4 on
    assert [m[1][3][-1] for m in maps] == [maps[0][1][3][-1] + 16 * i for i in range(3)]   # and the centres
    assert maps[0][1][3][:-1] == eng.calls("ira_onset_index")[1][1][8][:-1] and res.sums.shape == (5, 240, 151, 2)
    # an empty batch launches nothing
    before = len(eng.calls())
    res = D.burst_decay_device(eng, eng.upload([]), 48000, D.BurstDecaySettings())
    assert len(eng.calls("ira_burst_table")) == 2 and len(eng.calls()) == before + 2 and res.sums.shape == (0, 240, 61, 2)
    tab = eng.burst_table(rho[:2], half[:2], "hann")
    assert eng.burst_decay(batch.x, batch.off, batch.length, batch.off_dev, tab, np.zeros((2, 0)))[0].shape == (5, 2, 0, 2)
    assert eng.burst_table([], [], "hann").doubles == 0
    for bad, what in ((dict(window="hamming"), "window"), (dict(rho=[0.1]), "rho and half"), (dict(rho=[0.1, 0.0]), "rho"),
                      (dict(half=[3, 0]), "half"), (dict(half=[3, 2.5]), "half"), (dict(rho=[0.1] * 4097, half=[3] * 4097), "at most 4096")):
        kw = dict(rho=[0.1, 0.2], half=[3, 300], window="hann")
        kw.update(bad)
        with pytest.raises(ValueError, match=what):
            eng.burst_table(**kw)
    for bad, what in ((np.zeros((3, 4)), r"\(J, M\)"), (np.zeros(4), r"\(J, M\)"), (np.array([[0, 2, 1], [0, 0, 0]]), "decrease"),
                      (np.array([[0, 0.5], [0, 0]]), "whole"), (np.array([[0, (1 << 24) + 1], [0, 0]]), "whole"),
                      (np.zeros((2, 4097)), "at most 4096")):
        with pytest.raises(ValueError, match=what):
            eng.burst_decay(batch.x, batch.off, batch.length, batch.off_dev, tab, bad)
    with pytest.raises(ValueError, match="off and length"):
        eng.burst_decay(batch.x, batch.off, batch.length[:2], batch.off_dev, tab, np.zeros((2, 3)))


# ------------------------------------------------------------------------------------------------ the emulation
@pytest.mark.parametrize("window", R.WINDOWS)
def test_float64_table_form_lies_inside_both_bounds(window):
    """The bounds are float64 arithmetic's own: a NumPy emulation of the table form, (w * phasor) * x, stays inside the
    cell bound (N + 16) u A in both sum orders and its table inside 16 u w(k), from H = 1 to 12288 at three values of rho,
    with whole, clipped and empty windows."""
    rng = np.random.default_rng(21)
    x = (rng.standard_normal(30001) * np.exp(-np.arange(30001) / 4000.0)).astype(np.float32)
    worst_cell = worst_table = 0.0
    for half in (1, 2, 31, 32, 33, 64, 127, 128, 129, 1000, 2048, 12288):
        for rho in (1e-6, 0.1234567, 0.5):
            g = B.wavelet_emulate64(rho, half, window)
            worst_table = max(worst_table, B.table_ratio(g, rho, half, window))
            for c in (15000, 3, 30000 - 2, -half + 1, 30000 + half, 30001 + half, -half - 1):
                ref = R.reference(x, c, rho, half, window)
                for order in ("pairwise", "lanes"):
                    re, im = B.cell_emulate64(g, x, c, half, order)
                    if ref["n"] == 0:
                        assert re == 0.0 and im == 0.0
                    worst_cell = max(worst_cell, B.cell_ratio(re, im, ref))
    print(f"float64 table form, {window}: worst cell error / bound {worst_cell:.4f}, worst table error {16 * worst_table:.2f} u w(k)")
    assert worst_cell <= 1.0 and worst_table <= 1.0
