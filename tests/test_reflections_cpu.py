"""
CPU-only tests of the early-reflection detection (audio_analysis_amd.analyse.reflections): sample counts, settings
validation, records -> results for every status bit, the fixed text / Markdown / JSON formats on hand-built results, the
command line, the header's constants, the argument checks of ira_reflections (they return before touching a device), the
host side of the device function on the recording engine, and the restatement of tests/reflections_ref.py against itself
in float64 and long double.
"""
import json
import math
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import reflections_ref as R

REPO = Path(__file__).resolve().parent.parent
RATES = (22050, 44100, 48000, 96000)


def test_sample_counts_at_common_rates():
    from audio_analysis_amd.analyse import reflections as D
    assert [D.half_window_samples(1.0, fs) for fs in RATES] == [11, 22, 24, 48]
    assert [D.samples_of(2.5, fs) for fs in RATES] == [55, 110, 120, 240]
    assert [D.samples_of(1.0, fs) for fs in RATES] == [22, 44, 48, 96]
    assert [D.samples_of(0.5, fs) for fs in RATES] == [11, 22, 24, 48]
    assert [D.samples_of(5.0, fs) for fs in RATES] == [110, 221, 240, 480]
    assert [D.search_samples(200.0, fs) for fs in RATES] == [4410, 8820, 9600, 19200]
    assert D.search_samples(None, 48000) == D.UNBOUNDED == R.UNBOUNDED and D.search_samples(0.0, 48000) == 0
    assert D.samples_of(0.001, 8000) == 1 and D.half_window_samples(0.001, 8000) == 1
    for fs in RATES:
        for ms in (0.5, 1.0, 2.5, 5.0, 33.3):
            assert D.samples_of(ms, fs) == R.count_of(ms, fs) == max(1, math.floor(ms * fs / 1000.0 + 0.5))
            assert D.half_window_samples(ms, fs) == R.half_window(ms, fs) == max(1, math.floor(ms * fs / 2000.0 + 0.5))
            assert D.search_samples(ms, fs) == R.tn_of(ms, fs) == math.ceil(ms * fs / 1000.0)
        c = D.sample_counts(D.ReflectionSettings(), fs)
        assert (c.half, c.direct, c.direct_window, c.guard, c.separation, c.background, c.tn, c.curve_step) == \
            (D.half_window_samples(1.0, fs), D.samples_of(2.5, fs), D.samples_of(2.5, fs), D.samples_of(1.0, fs),
             D.samples_of(0.5, fs), D.samples_of(5.0, fs), D.search_samples(200.0, fs), D.samples_of(1.0, fs))


def test_settings_defaults_and_validation():
    from audio_analysis_amd.analyse import reflections as D
    s = D.ReflectionSettings()
    assert (s.smooth_ms, s.window, s.direct_search_ms, s.direct_window_ms, s.guard_ms, s.separation_ms, s.background_ms,
            s.min_level_db, s.prominence_db, s.max_time_ms, s.max_reflections, s.onset_db, s.speed_of_sound, s.curve_step_ms,
            s.use_mono_downmix_for_stereo) == (1.0, "hann", 2.5, 2.5, 1.0, 0.5, 5.0, -40.0, 6.0, 200.0, 16, -20.0, 343.0, 1.0,
                                               False)
    assert s.rel_energy == 10.0 ** (-20.0 / 10.0) and s.rel == 10.0 ** (-40.0 / 10.0) and s.prom == 10.0 ** (6.0 / 10.0)
    assert D.ReflectionSettings(max_time_ms=None, max_reflections=64, min_level_db=0, prominence_db=0).max_time_ms is None
    nan, inf = float("nan"), float("inf")
    bad = [(dict(window="hamming"), "window must"), (dict(guard_ms=0.4), "guard_ms"), (dict(background_ms=0.5), "background_ms"),
           (dict(background_ms=0.25), "background_ms"), (dict(min_level_db=1.0), "min_level_db"), (dict(min_level_db=nan), "min_level_db"),
           (dict(prominence_db=-0.1), "prominence_db"), (dict(prominence_db=inf), "prominence_db"),
           (dict(max_time_ms=-1.0), "max_time_ms"), (dict(max_time_ms=inf), "max_time_ms"),
           (dict(max_reflections=0), "max_reflections"), (dict(max_reflections=65), "max_reflections"),
           (dict(max_reflections=2.5), "max_reflections"), (dict(onset_db=1.0), "onset_db"), (dict(onset_db=nan), "onset_db")]
    for name in ("smooth_ms", "direct_search_ms", "direct_window_ms", "guard_ms", "separation_ms", "background_ms",
                 "speed_of_sound", "curve_step_ms"):
        bad += [({name: 0.0}, name), ({name: -1.0}, name), ({name: nan}, name), ({name: inf}, name)]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            D.ReflectionSettings(**kw)
    # the bounds in samples hold at the rate the settings are used at
    for kw, fs, what in ((dict(smooth_ms=21.4), 48000, "smooth_ms"), (dict(smooth_ms=10.7), 96000, "smooth_ms"),
                         (dict(direct_search_ms=21.4), 48000, "direct_search_ms"),
                         (dict(separation_ms=21.4, guard_ms=30.0, background_ms=40.0), 48000, "separation_ms"),
                         (dict(background_ms=42.7), 48000, "background_ms"), (dict(background_ms=21.4), 96000, "background_ms"),
                         (dict(separation_ms=0.5, background_ms=0.51), 1000, "background_ms")):      # B == S == 1 sample
        with pytest.raises(ValueError, match=what):
            D.sample_counts(D.ReflectionSettings(**kw), fs)
    c = D.sample_counts(D.ReflectionSettings(smooth_ms=21.33, direct_search_ms=21.33, background_ms=42.66), 48000)
    assert (c.half, c.direct, c.background) == (512, 1024, 2048)              # the bounds themselves pass


def _hand_built():
    from audio_analysis_amd.analyse.reflections import Reflection, ReflectionChannelResult
    nan, inf = float("nan"), float("inf")
    ok = ReflectionChannelResult(
        channel_name="left", sample_rate_hz=48000, onset_samples=200, onset_seconds=200 / 48000, status=0, smooth_ms=1.0,
        window="hann", window_samples=49, direct_samples=200, direct_seconds=200 / 48000, itdg_ms=3.104166, drr_db=-0.3649,
        candidates_found=3,
        reflections=(Reflection(349, 349, 3.104166, -6.0206, 12.3456, 1, 1.0647),
                     Reflection(1146, 1145, 19.708333, -13.152, inf, -1, 6.76),
                     Reflection(2000, 2000, 37.5, -20.0, 6.5, 0, 12.8625)),
        curve_step_seconds=0.001, curve=np.array([0.0, nan, -inf, -12.5], np.float32))
    bad = ReflectionChannelResult(
        channel_name="right", sample_rate_hz=48000, onset_samples=0, onset_seconds=0.0, status=3, smooth_ms=0.5,
        window="rect", window_samples=25, direct_samples=-1, direct_seconds=nan, itdg_ms=nan, drr_db=nan,
        candidates_found=0, reflections=(), curve_step_seconds=0.001, curve=None)
    return [ok, bad]


def test_summary_text_format_is_pinned():
    from audio_analysis_amd.analyse.reflections import summarise_reflections_text
    assert summarise_reflections_text(_hand_built()) == (
        "[left]\n"
        "Onset: 200 samples (4.167 ms)  Direct: 200 samples (4.167 ms)  Status: ok  Window: hann 1 ms (49 samples)\n"
        "#  delay_ms  level_dB  prominence_dB  polarity  path_m\n"
        "1  3.104  -6.02  12.35  +  1.065\n"
        "2  19.708  -13.15  +inf  -  6.760\n"
        "3  37.500  -20.00  6.50  0  12.863\n"
        "ITDG: 3.104 ms  DRR: -0.36 dB  found 3, kept 3\n"
        "\n"
        "[right]\n"
        "Onset: 0 samples (0.000 ms)  Direct: NA  Status: 3 (silent, too short)  Window: rect 0.5 ms (25 samples)\n"
        "#  delay_ms  level_dB  prominence_dB  polarity  path_m\n"
        "ITDG: NA ms  DRR: NA dB  found 0, kept 0\n"
        "\n")
    assert summarise_reflections_text([]) == ""


def test_summary_markdown_format_is_pinned():
    from audio_analysis_amd.analyse.reflections import summarise_reflections_markdown
    assert summarise_reflections_markdown(_hand_built()[:1]) == (
        "### left\n"
        "\n"
        "Onset: 200 samples (4.167 ms). Direct: 200 samples (4.167 ms). Status: ok. Window: hann 1 ms (49 samples).\n"
        "\n"
        "| # | delay (ms) | level (dB) | prominence (dB) | polarity | path (m) |\n"
        "|---|---:|---:|---:|---:|---:|\n"
        "| 1 | 3.104 | -6.02 | 12.35 | + | 1.065 |\n"
        "| 2 | 19.708 | -13.15 | +inf | - | 6.760 |\n"
        "| 3 | 37.500 | -20.00 | 6.50 | 0 | 12.863 |\n"
        "\n"
        "ITDG: 3.104 ms. DRR: -0.36 dB. found 3, kept 3.\n"
        "\n")


def test_json_round_trip_keeps_nan_and_infinities_and_drops_the_curve_on_request():
    from audio_analysis_amd.analyse.reflections import (reflections_results_from_json, reflections_results_to_json,
                                                        summarise_reflections_text)
    res = _hand_built()
    text = json.dumps(reflections_results_to_json(res), allow_nan=False)     # strict JSON: no NaN tokens
    assert "NaN" not in text
    doc = json.loads(text)
    rows = doc["reflections"]
    assert rows[0]["curve"] == [0.0, None, "-inf", -12.5] and rows[0]["reflections"][1]["prominence_db"] == "+inf"
    assert rows[0]["reflections"][0] == {"sample_index": 349, "peak_sample_index": 349, "delay_ms": 3.104166,
                                         "level_db": -6.0206, "prominence_db": 12.3456, "polarity": 1,
                                         "path_difference_m": 1.0647}
    assert "curve" not in rows[1] and rows[1]["itdg_ms"] is None and rows[1]["drr_db"] is None
    assert rows[1]["direct_seconds"] is None and rows[1]["direct_samples"] == -1 and rows[1]["reflections"] == []
    assert set(rows[0]) == {"channel_name", "sample_rate_hz", "onset_samples", "onset_seconds", "status", "smooth_ms",
                            "window", "window_samples", "direct_samples", "direct_seconds", "itdg_ms", "drr_db",
                            "candidates_found", "reflections", "curve_step_seconds", "curve"}
    back = reflections_results_from_json(doc)
    assert summarise_reflections_text(back) == summarise_reflections_text(res)
    assert reflections_results_to_json(back) == doc
    assert math.isnan(back[1].itdg_ms) and back[1].curve is None and back[1].status == 3
    assert back[0].curve.dtype == np.float32 and np.array_equal(back[0].curve, res[0].curve, equal_nan=True)
    assert back[0].reflections == res[0].reflections and back[0].reflections[1].prominence_db == float("inf")
    slim = reflections_results_to_json(res, with_curve=False)
    assert all("curve" not in r for r in slim["reflections"])
    assert reflections_results_from_json(json.loads(json.dumps(slim)))[0].curve is None


def test_results_from_records_status_bits():
    from audio_analysis_amd.analyse import reflections as D
    nan, inf = float("nan"), float("inf")
    st = D.ReflectionSettings(max_reflections=3, max_time_ms=10.0)
    c = D.sample_counts(st, 48000)                                             # R <= 120 + 480 + 240
    rec = np.array([[200.0, 2.0, 5.0, 2.0, 349.0, 1.0, 0.5, 0.0],              # fine
                    [10.0, 2.0, 0.0, 0.0, -1.0, 1.0, 0.0, 0.0],                # no candidate, nothing behind the direct window
                    [200.0, nan, 1.0, 1.0, 349.0, 1.0, 0.5, 3.0],              # three non-finite row entries
                    [0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0],                 # silence
                    [60.0, 2.0, 0.0, 0.0, -1.0, 1.0, 0.0, 0.0],                # n0 + G >= L
                    [0.0, nan, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0]])                # empty channel
    lists = np.full((6, 3, 6), nan)
    lists[:, :, (0, 3, 4)] = -1.0
    lists[0, 0] = [349.0, 0.5, 0.25, 5.0, 349.0, 0.5]                          # -6.02 dB, prominence 10 dB
    lists[0, 1] = [1146.0, 0.1, 0.0, 432.0, 1145.0, -0.22]                     # a silent background: +inf
    lists[2, 0] = lists[0, 0]
    length = np.array([3000, 2000, 3000, 2000, 108, 0])
    onset = np.array([200, 10, 200, 0, 60, 0])
    room = [int(min(n, 840)) for n in length]
    erow = np.concatenate([np.full(r, 2.0) for r in room])
    erow[0:3] = [2.0, 0.2, 0.0]
    erow[48], erow[96] = 1.0, 4.0
    res = D.ReflectionRecords(settings=st, counts=c, length=length, onset=onset, peak_abs=np.array([1, 1, 1, 0, 1, 0], np.float32),
                              records=rec, lists=lists, erow=erow, erow_off=np.concatenate([[0], np.cumsum(room)[:-1]]))
    out = D.reflection_results(res, 48000, list("abcdef"))
    assert [r.status for r in out] == [0, 0, D.STATUS_NON_FINITE, D.STATUS_SILENT, D.STATUS_TOO_SHORT,
                                       D.STATUS_SILENT | D.STATUS_TOO_SHORT]
    a = out[0]
    assert a.direct_samples == 200 and a.direct_seconds == 200 / 48000 and a.onset_samples == 200 and a.candidates_found == 5
    assert a.itdg_ms == 1000.0 * 149 / 48000 and a.drr_db == 10.0 * math.log10(2.0) and len(a.reflections) == 2
    q = a.reflections[0]
    assert (q.sample_index, q.peak_sample_index, q.polarity) == (349, 349, 1) and q.delay_ms == 1000.0 * 149 / 48000
    assert q.level_db == 10.0 * math.log10(0.25) and q.prominence_db == 10.0 * math.log10(0.5 * 5.0 / 0.25)
    assert q.path_difference_m == 343.0 * (149 / 48000)
    q = a.reflections[1]
    assert q.prominence_db == inf and q.polarity == -1 and q.peak_sample_index == 1145
    assert a.curve.dtype == np.float32 and len(a.curve) == 18 and a.curve_step_seconds == 0.001       # ceil(840 / 48)
    assert a.curve[0] == 0.0 and a.curve[1] == np.float32(10.0 * math.log10(0.5)) and a.curve[2] == np.float32(10.0 * math.log10(2.0))
    assert out[1].drr_db == inf and math.isnan(out[1].itdg_ms) and out[1].reflections == () and out[1].status == 0
    for r in out[2:]:
        assert r.direct_samples == -1 and math.isnan(r.direct_seconds) and math.isnan(r.itdg_ms) and math.isnan(r.drr_db)
        assert r.reflections == () and r.candidates_found == 0 and np.all(np.isnan(r.curve))
    assert [len(r.curve) for r in out] == [18, 18, 18, 18, 1, 0]                # R = min(L - o, Rmax) at 1 ms steps
    assert D.reflection_results(res, 48000, list("abcdef"), keep_curve=False)[0].curve is None
    assert D.status_text(0) == "ok" and D.status_text(6) == "6 (too short, non-finite)"
    text = D.summarise_reflections_text(out)
    assert "Status: 4 (non-finite)" in text and "Status: 1 (silent)" in text and "Status: 2 (too short)" in text
    assert "DRR: +inf dB" in text and "ITDG: NA ms" in text
    assert "NaN" not in json.dumps(D.reflections_results_to_json(out), allow_nan=False)


def test_cli_parser_defaults_and_help_through_the_shim():
    import analyse.reflections as shim
    from audio_analysis_amd.analyse import reflections as D
    assert shim is D
    p = D.build_parser()
    a = p.parse_args(["--input", "a.wav", "b.wav"])
    assert a.input == [Path("a.wav"), Path("b.wav")] and a.bundle is None and a.mono is False and a.no_curve is False
    assert (a.expected_sample_rate, a.json) == (48000, None)
    assert D.settings_from_args(a) == D.ReflectionSettings()
    a = p.parse_args(["--bundle", "d", "--mono", "--smooth-ms", "2", "--window", "rect", "--direct-search-ms", "3",
                      "--direct-window-ms", "4", "--guard-ms", "1.5", "--separation-ms", "0.75", "--background-ms", "8",
                      "--min-level-db", "-30", "--prominence-db", "3", "--max-time-ms", "none", "--max-reflections", "5",
                      "--onset-db", "-30", "--speed-of-sound", "340", "--curve-step-ms", "0.5", "--no-curve",
                      "--expected-sample-rate", "44100", "--json", "o.json"])
    assert D.settings_from_args(a) == D.ReflectionSettings(
        smooth_ms=2.0, window="rect", direct_search_ms=3.0, direct_window_ms=4.0, guard_ms=1.5, separation_ms=0.75,
        background_ms=8.0, min_level_db=-30.0, prominence_db=3.0, max_time_ms=None, max_reflections=5, onset_db=-30.0,
        speed_of_sound=340.0, curve_step_ms=0.5, use_mono_downmix_for_stereo=True)
    assert a.bundle == Path("d") and a.no_curve and a.expected_sample_rate == 44100 and a.json == Path("o.json")
    assert p.parse_args(["--input", "a.wav", "--max-time-ms", "80"]).max_time_ms == 80.0
    for bad in ([], ["--input", "a.wav", "--bundle", "d"], ["--input", "a.wav", "--window", "hamming"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit):                                       # invalid settings end as a usage error
        D.main(["--input", "a.wav", "--guard-ms", "0.25"])
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.reflections", "--help"], capture_output=True, text=True,
                       cwd=str(REPO), env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--input", "--bundle", "--mono", "--smooth-ms", "--window", "--direct-search-ms", "--direct-window-ms",
                 "--guard-ms", "--separation-ms", "--background-ms", "--min-level-db", "--prominence-db", "--max-time-ms",
                 "--max-reflections", "--onset-db", "--speed-of-sound", "--curve-step-ms", "--no-curve",
                 "--expected-sample-rate", "--json"):
        assert flag in r.stdout


def test_header_constants_symbol_and_abi_version():
    from audio_analysis_amd import _lib, build, engine
    from audio_analysis_amd.analyse import reflections as D
    hdr = (REPO / "include" / "ira.h").read_text()
    for name in ("DOUBLES", "FIELDS", "TILE", "MAX_HALF", "MAX_DIRECT", "MAX_BG", "MAX_KEEP"):
        assert re.search(rf"#define IRA_REFL_{name} {getattr(engine, 'REFL_' + name)}\b", hdr), name
    assert (engine.REFL_DOUBLES, engine.REFL_FIELDS, engine.REFL_TILE, engine.REFL_MAX_HALF, engine.REFL_MAX_DIRECT,
            engine.REFL_MAX_BG, engine.REFL_MAX_KEEP) == (8, 6, 1024, 512, 1024, 2048, 64)
    assert (D.MAX_HALF_SAMPLES, D.MAX_DIRECT_SAMPLES, D.MAX_BACKGROUND_SAMPLES, D.MAX_REFLECTIONS) == (512, 1024, 2048, 64)
    src = (REPO / "audio_analysis_amd" / "csrc" / "ira_reflections.hip").read_text()
    assert f"REFL_MAX_SEP = {engine.REFL_MAX_SEP};" in src and "REFL_UNBOUNDED = (int64_t)1 << 40;" in src
    assert engine.REFL_UNBOUNDED == 1 << 40
    assert build.SOURCES["ira_reflections.hip"] == ["-ffp-contract=off"]
    assert "#define IRA_ABI_VERSION 15 " in hdr and _lib.ABI_VERSION == 15
    assert "ira_reflections" in _lib.PROTOTYPES and re.search(r"int32_t ira_reflections\(", hdr)
    lib = _lib.load()
    assert lib.ira_abi_version() == 15 and lib.ira_reflections is not None
    # the candidates of a tile and the scratch: a count and 4 doubles per candidate a tile can hold
    assert [engine.refl_tile_candidates(s) for s in (1, 24, 48, 1023, 1024)] == [512, 41, 21, 1, 1]
    assert engine.refl_scratch_doubles(3, 9960, 24) == 3 * 10 * (1 + 4 * 41) and engine.refl_scratch_doubles(2, 0, 24) == 0
    assert engine.refl_scratch_doubles(1, 1024, 1) == 1 + 4 * 512 and engine.refl_scratch_doubles(1, 1025, 1) == 2 * (1 + 4 * 512)
    assert list(engine.refl_row_room([0, 5, 20000], 120, 9600, 240)) == [0, 5, 9960]
    assert list(engine.refl_row_room([0, 5, 20000], 120, 1 << 40, 240)) == [0, 5, 20000]


def test_entry_point_validates_arguments_without_gpu():
    from audio_analysis_amd import _lib
    lib = _lib.load()
    E_NULL, E_SIZE = -1, -2

    def call(**kw):
        a = dict(x=1, off=1, len=1, onset=1, nch=0, w=1, d=24, D=120, Dw=120, G=48, S=24, B=240, Tn=9600, rel=1e-4, prom=4.0,
                 keep=16, max_room=9960, erow=1, erow_off=1, scratch=1, scratch_doubles=0, lst=1, rec=1)
        a.update(kw)
        return lib.ira_reflections(a["x"], a["off"], a["len"], a["onset"], a["nch"], a["w"], a["d"], a["D"], a["Dw"], a["G"],
                                   a["S"], a["B"], a["Tn"], a["rel"], a["prom"], a["keep"], a["max_room"], a["erow"],
                                   a["erow_off"], a["scratch"], a["scratch_doubles"], a["lst"], a["rec"], 0)

    assert call() == 0                                                     # nch == 0: nothing to do
    for name in ("x", "off", "len", "onset", "w", "erow", "erow_off", "scratch", "lst", "rec"):
        assert call(**{name: 0}) == E_NULL, name
    nan, inf = float("nan"), float("inf")
    for kw in (dict(d=0), dict(d=513), dict(D=0), dict(D=1025), dict(Dw=0), dict(S=0), dict(S=1025, G=2000, B=2048),
               dict(G=23), dict(B=24), dict(B=2049), dict(Tn=-1), dict(rel=-1.0), dict(rel=nan), dict(rel=inf),
               dict(prom=0.5), dict(prom=nan), dict(prom=inf), dict(keep=0), dict(keep=65), dict(nch=-1), dict(nch=65536),
               dict(max_room=-1), dict(max_room=9961)):
        assert call(**kw) == E_SIZE, kw
    assert call(d=1) == 0 and call(d=512) == 0 and call(D=1024) == 0 and call(G=24) == 0 and call(B=25, max_room=9745) == 0
    assert call(B=2048) == 0 and call(keep=1) == 0 and call(keep=64) == 0 and call(prom=1.0) == 0 and call(rel=1.0) == 0
    assert call(Tn=1 << 40, max_room=1 << 30) == 0 and call(Tn=0, max_room=360) == 0
    # the scratch is checked against the geometry before any launch: 10 tiles of 1 + 4 * 41 doubles per channel
    assert call(nch=2, scratch_doubles=2 * 10 * 165 - 1) == E_SIZE and call(nch=1, scratch_doubles=0) == E_SIZE
    assert call(d=0, nch=1) == E_SIZE and call(x=0, nch=1) == E_NULL            # refused before any launch


def test_reflections_device_is_one_launch_over_every_channel():
    """The host side of reflections_device on the recording engine: one ira_reflections call whose tables hold the
    channels' offsets and lengths, the host-built weights, the row offsets of onset 0, the counts and the scratch size."""
    from host_engine import HostEngine
    from audio_analysis_amd.analyse import reflections as D
    from audio_analysis_amd.analyse.echodensity import window_weights
    from audio_analysis_amd.synth import synth_ir
    eng = HostEngine()
    lens = [60000, 5000, 0, 7001]
    batch = eng.upload([synth_ir(i, 0, n, 48000) if n else np.zeros(0, np.float32) for i, n in enumerate(lens)])
    res = D.reflections_device(eng, batch, 48000, D.ReflectionSettings())
    assert len(eng.calls("ira_onset_index")) == 1
    calls = eng.calls("ira_reflections")
    assert len(calls) == 1 and calls[0][0] == "ira_reflections"
    (x, off, ln, onset, nch, w, d, big_d, dw, g, s, b, tn, rel, prom, keep, max_room, erow, erow_off, scratch, scratch_doubles,
     lst, rec, stream) = calls[0][1]
    assert (nch, d, big_d, dw, g, s, b, tn, keep, stream) == (4, 24, 120, 120, 48, 24, 240, 9600, 16, None)
    assert rel == 10.0 ** (-40.0 / 10.0) and prom == 10.0 ** (6.0 / 10.0)
    assert list(eng.table(off)[:4]) == list(batch.off) and list(eng.table(ln)[:4]) == lens
    assert np.array_equal(eng.table(w)[:49], window_weights(24, "hann"))
    assert list(eng.table(erow_off)[:4]) == [0, 9960, 14960, 14960] and max_room == 9960        # min(L, 120 + 9600 + 240)
    assert erow[:3] == ("empty", 9960 + 5000 + 7001, "torch.float64")
    assert scratch_doubles == 4 * 10 * (1 + 4 * 41) and scratch[:3] == ("empty", scratch_doubles, "torch.float64")
    assert lst[:3] == ("empty", 4 * 16 * 6, "torch.float64") and rec[:3] == ("empty", 32, "torch.float64")
    assert onset[0] == "empty" and x[0] == "up"
    assert res.records.shape == (4, 8) and res.lists.shape == (4, 16, 6) and res.erow.shape == (21961,)
    assert list(res.erow_off) == [0, 9960, 14960, 14960] and list(res.length) == lens and res.counts.half == 24
    # the whole channel, rect, other counts: the rows are sized by the lengths; without the curve the rows stay behind
    st = D.ReflectionSettings(window="rect", smooth_ms=0.5, max_time_ms=None, separation_ms=1.0 / 48.0, guard_ms=0.1,
                              background_ms=2.0, max_reflections=64, min_level_db=0.0, prominence_db=0.0)
    res = D.reflections_device(eng, batch, 48000, st, keep_curve=False)
    args = eng.calls("ira_reflections")[1][1]
    assert args[4:5] + args[6:16] == (4, 12, 120, 120, 5, 1, 96, 1 << 40, 1.0, 1.0, 64) and args[16] == 60000
    assert np.array_equal(eng.table(args[5])[:25], np.ones(25)) and list(eng.table(args[18])[:4]) == [0, 60000, 65000, 65000]
    assert args[17][:2] == ("empty", 72001) and args[20] == 4 * 59 * (1 + 4 * 512) and args[21][:2] == ("empty", 4 * 64 * 6)
    assert res.erow is None and res.lists.shape == (4, 64, 6)
    # an empty batch launches nothing
    n_before = len(eng.calls("ira_reflections"))
    res = D.reflections_device(eng, eng.upload([]), 48000, st)
    assert len(eng.calls("ira_reflections")) == n_before and res.records.shape == (0, 8) and res.lists.shape == (0, 64, 6)
    with pytest.raises(ValueError, match="at most 1025"):
        D.reflections_device(eng, batch, 192000, D.ReflectionSettings(smooth_ms=6.0))
    good = dict(weights=np.ones(7), half=3, direct=10, direct_window=10, guard=4, separation=2, background=20, tn=100,
                rel=1e-4, prom=4.0, keep=16)
    for bad, what in ((dict(half=0), "half"), (dict(weights=np.ones(5)), "weights"), (dict(direct=1025), "direct"),
                      (dict(direct_window=0), "direct_window"), (dict(separation=0), "separation"), (dict(guard=1), "guard"),
                      (dict(background=2), "background"), (dict(background=2049), "background"), (dict(tn=-1), "tn"),
                      (dict(prom=0.5), "prom"), (dict(rel=float("nan")), "rel"), (dict(keep=65), "keep"), (dict(keep=0), "keep")):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError, match=what):
            eng.reflections(batch.x, batch.off, batch.length, batch.off_dev, **kw)


# ------------------------------------------------------------------------------------------------ the restatement
DEFAULTS = dict(d=24, window="hann", D=120, Dw=120, G=48, S=24, B=240, Tn=9600, rel=10.0 ** -4.0, prom=10.0 ** 0.6, keep=16)


@pytest.mark.parametrize("n,seed", [(6000, 1), (24000, 3)])
def test_restatement_finds_the_planted_reflections_in_both_precisions(n, seed):
    x = R.sparse_room(n, seed)
    o = R.onset_index(x)
    margins = []
    lo = R.detect(x, o, margins=margins, **DEFAULTS)
    hi = R.detect(x, o, dtype=np.longdouble, **DEFAULTS)
    assert R.decisions(lo) == R.decisions(hi)                                 # the same decisions in both precisions
    assert lo["n0"] == R.DIRECT_AT and lo["M"] == 5 and lo["first"] == lo["candidates"][0][0]
    found = [c[0] for c in lo["candidates"]]
    assert all(abs(a - b) <= 1 for a, b in zip(found, R.planted())), (found, R.planted())
    assert [r[5] for r in lo["kept"]] == [np.float32(g) for _, g in R.REFLECTIONS]          # the planted samples, signs included
    levels = [10.0 * math.log10(c[1] / lo["Ed"]) for c in lo["candidates"]]
    assert [round(v, 1) for v in levels[:4]] == [-6.0, -9.1, -10.5, -13.2] and -14.2 <= round(levels[4], 1) <= -13.5
    assert lo["candidates"][3][2] == 0.0 and lo["candidates"][3][3] == 432      # 19.7 ms lies in digital silence: +inf
    # float64 against long double: W non-negative terms, one rounding per product and per add
    w_len = 2 * DEFAULTS["d"] + 1
    e64, e80 = R.envelope(x, DEFAULTS["d"], "hann"), R.envelope(x, DEFAULTS["d"], "hann", np.longdouble)
    assert np.all(np.abs(e64.astype(np.longdouble) - e80) <= (w_len + 2) * np.longdouble(2.0) ** -53 * e80)
    # every comparison that decides lies far above that rounding
    assert min(margins) >= 1e-7 > 1e4 * (w_len + 2) * 2.0 ** -53, min(margins)
    assert abs(float(lo["Edir"]) - float(hi["Edir"])) <= (lo["terms"][0] + 1) * 2.0 ** -53 * float(hi["Edir"])
    assert abs(float(lo["Erest"]) - float(hi["Erest"])) <= (lo["terms"][1] + 1) * 2.0 ** -53 * float(hi["Erest"])


def test_restatement_ties_selection_and_degenerate_inputs():
    x = R.twin_pulses()
    o = R.onset_index(x)
    assert o == 100
    both = R.detect(x, o, **DEFAULTS)
    assert [c[0] for c in both["candidates"]] == [1500, 2200] and both["candidates"][0][1] == both["candidates"][1][1]
    one = R.detect(x, o, **dict(DEFAULTS, keep=1))
    assert one["M"] == 2 and [r[0] for r in one["kept"]] == [1500] and one["first"] == 1500       # the earlier of a tie
    # the strongest are kept and written in time order, whatever their order in level
    x = R.sparse_room(6000, 1)
    kept = R.detect(x, 200, **dict(DEFAULTS, keep=3))["kept"]
    assert [r[0] for r in kept] == R.planted()[:3]
    x[R.planted()[4]] = 0.6
    kept = R.detect(x, 200, **dict(DEFAULTS, keep=2))["kept"]
    assert [r[0] for r in kept] == [R.planted()[0], R.planted()[4]]
    # a constant magnitude: a plateau of equal sums has no strict maximum; the direct sound is the onset
    flat = (0.25 * np.random.default_rng(1).choice([-1.0, 1.0], 3000)).astype(np.float32)
    r = R.detect(flat, 0, **dict(DEFAULTS, window="rect", d=0 + 24))
    assert r["M"] == 0 and r["first"] == -1 and r["kept"] == []
    r = R.detect(flat, 50, **dict(DEFAULTS, window="rect"))
    assert r["n0"] == 50 and r["M"] == 0
    # min_level_db = 0: nothing reaches the direct sound
    r = R.detect(R.sparse_room(6000, 1), 200, **dict(DEFAULTS, rel=1.0))
    assert r["M"] == 0 and r["first"] == -1
    # an empty channel, one sample, a NaN inside the row
    r = R.detect(np.zeros(0, np.float32), 0, **DEFAULTS)
    assert r["row"].size == 0 and r["n0"] == 0 and math.isnan(r["Ed"]) and r["M"] == 0
    r = R.detect(np.array([0.5], np.float32), 0, **DEFAULTS)
    assert r["row"].size == 1 and r["n0"] == 0 and r["M"] == 0 and float(r["Edir"]) == 0.25 and float(r["Erest"]) == 0.0
    x = R.sparse_room(6000, 1)
    x[1000] = np.nan
    r = R.detect(x, 200, **DEFAULTS)
    assert r["nonfinite"] == 49 and r["n0"] == 200
