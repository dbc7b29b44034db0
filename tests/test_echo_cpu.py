"""
CPU-only tests of the echo criterion (audio_analysis_amd.analyse.echo): sample counts, settings validation, rating words,
the fixed text / Markdown / JSON formats on hand-built results, the command line's parser, the host side of the device
function on the recording engine, and the argument checks of the new C entry points (they return before touching a
device).
"""
import ctypes
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent


def test_sample_counts_at_common_rates():
    from audio_analysis_amd.analyse import echo as E
    assert [E.lag_samples(9.0, fs) for fs in (22050, 44100, 48000, 96000)] == [198, 397, 432, 864]
    assert [E.lag_samples(14.0, fs) for fs in (22050, 44100, 48000, 96000)] == [309, 617, 672, 1344]
    assert E.lag_samples(0.001, 8000) == 1                              # never below one sample
    for fs in (22050, 44100, 48000, 96000):
        for ms in (9.0, 14.0, 1.0, 33.3):
            assert E.lag_samples(ms, fs) == max(1, math.floor(ms * fs / 1000.0 + 0.5))
    assert E.guard_samples(50.0, 48000) == 2400 and E.guard_samples(50.0, 44100) == 2205 and E.guard_samples(0.0, 48000) == 0
    assert E.max_samples(1000.0, 48000) == 48001 and E.max_samples(None, 48000) == 1 << 31
    assert E.curve_step_samples(1.0, 48000) == 48 and E.curve_step_samples(1.0, 44100) == 44
    assert E.curve_step_samples(0.0, 48000) == 0 and E.curve_step_samples(0.001, 48000) == 1
    st = E.EchoCriterionSettings()
    assert E.criterion_params(E.SPEECH, 48000, st) == [2.0 / 3.0, 432.0, 2400.0, 48001.0, 48.0, 0.9, 1.0, 48000.0]
    assert E.criterion_params(E.MUSIC, 96000, st)[1] == 1344.0          # 14 ms at 96 kHz fits the halo
    with pytest.raises(ValueError, match="at most 2048"):
        E.criterion_params(E.EchoCriterion("slow", 1.0, 30.0, None, 1.0, 2.0), 96000, st)
    hdr = (REPO / "include" / "ira.h").read_text()
    assert f"#define IRA_ECHO_MAX_LAG {E.MAX_LAG_SAMPLES}" in hdr
    from audio_analysis_amd import engine
    for name in ("DOUBLES", "CHUNK", "MAX_LAG", "MAX_PARAMS", "PARAM_DOUBLES"):
        assert f"#define IRA_ECHO_{name} {getattr(engine, 'ECHO_' + name)}" in hdr


def test_settings_defaults_and_validation():
    from audio_analysis_amd.analyse.echo import MUSIC, SPEECH, EchoCriterion, EchoCriterionSettings
    s = EchoCriterionSettings()
    assert s.criteria == (SPEECH, MUSIC) and s.onset_db == -20.0 and s.max_tau_ms == 1000.0 and s.end_guard_ms == 50.0
    assert s.curve_step_ms == 1.0 and not s.use_mono_downmix_for_stereo and s.rel_energy == 10.0 ** (-20.0 / 10.0)
    assert (SPEECH.exponent, SPEECH.window_ms, SPEECH.band_hz, SPEECH.threshold_10, SPEECH.threshold_50) == \
        (2.0 / 3.0, 9.0, (700.0, 1400.0), 0.9, 1.0)
    assert (MUSIC.exponent, MUSIC.window_ms, MUSIC.band_hz, MUSIC.threshold_10, MUSIC.threshold_50) == \
        (1.0, 14.0, (700.0, 2800.0), 1.5, 1.8)
    assert EchoCriterionSettings(criteria=[SPEECH], max_tau_ms=None).max_tau_ms is None
    assert EchoCriterion("x", 1, 5, [100, 200], 1, 2).band_hz == (100.0, 200.0)
    ok = dict(name="x", exponent=1.0, window_ms=9.0, band_hz=None, threshold_10=1.0, threshold_50=2.0)
    for bad, what in [(dict(name=" "), "name"), (dict(exponent=0.0), "exponent"), (dict(exponent=float("inf")), "exponent"),
                      (dict(window_ms=0.0), "window_ms"), (dict(window_ms=float("nan")), "window_ms"),
                      (dict(band_hz=(1400.0, 700.0)), "band_hz"), (dict(band_hz=(0.0, 700.0)), "band_hz"),
                      (dict(band_hz=700.0), "band_hz"), (dict(threshold_10=float("nan")), "thresholds"),
                      (dict(threshold_10=2.0, threshold_50=1.0), "threshold_50")]:
        with pytest.raises(ValueError, match=what):
            EchoCriterion(**dict(ok, **bad))
    for bad, what in [(dict(criteria=()), "1 to 4"), (dict(criteria=(SPEECH,) * 5), "1 to 4"),
                      (dict(criteria=(SPEECH, SPEECH)), "unique"), (dict(criteria=("speech",)), "EchoCriterion"),
                      (dict(criteria=3), "sequence"), (dict(onset_db=1.0), "onset_db"),
                      (dict(onset_db=float("nan")), "onset_db"), (dict(max_tau_ms=0.0), "max_tau_ms"),
                      (dict(max_tau_ms=float("inf")), "max_tau_ms"), (dict(end_guard_ms=-1.0), "end_guard_ms"),
                      (dict(curve_step_ms=-1.0), "curve_step_ms"), (dict(curve_step_ms=float("nan")), "curve_step_ms")]:
        with pytest.raises(ValueError, match=what):
            EchoCriterionSettings(**bad)


def test_rating_words_at_the_thresholds():
    from audio_analysis_amd.analyse.echo import MUSIC, SPEECH
    below = math.nextafter(0.9, 0.0)
    assert [SPEECH.rating(v) for v in (0.0, below, 0.9, math.nextafter(1.0, 0.0), 1.0, 7.0)] == \
        ["inaudible", "inaudible", "marginal", "marginal", "audible", "audible"]
    assert [MUSIC.rating(v) for v in (1.49, 1.5, 1.79, 1.8)] == ["inaudible", "marginal", "marginal", "audible"]
    assert SPEECH.rating(float("nan")) == "NA"


def test_criteria_with_equal_edges_share_a_band():
    from audio_analysis_amd.analyse.echo import MUSIC, SPEECH, EchoCriterion, criterion_bands
    bands, rows = criterion_bands((SPEECH, MUSIC))
    assert rows == [1, 2] and [(b.name, b.kind, b.low_edge_hz, b.high_edge_hz) for b in bands] == \
        [("700-1400Hz", "bandpass", 700.0, 1400.0), ("700-2800Hz", "bandpass", 700.0, 2800.0)]
    assert bands[0].centre_hz == math.sqrt(700.0 * 1400.0)
    wide = EchoCriterion("wide", 1.0, 9.0, None, 1.0, 2.0)
    twin = EchoCriterion("twin", 2.0, 20.0, (700.0, 1400.0), 1.0, 2.0)
    bands, rows = criterion_bands((wide, SPEECH, twin, MUSIC))
    assert rows == [0, 1, 1, 2] and len(bands) == 2
    assert criterion_bands((wide,)) == ([], [0])


def _hand_built():
    from audio_analysis_amd.analyse.echo import MUSIC, SPEECH, EchoCriterionChannelResult, EchoCriterionValues
    nan = float("nan")
    ok = EchoCriterionChannelResult(
        channel_name="left", sample_rate_hz=48000, onset_samples=240, onset_seconds=0.005, status=0,
        criteria=(SPEECH, MUSIC), curve_step_seconds=0.001,
        values_by_name={"speech": EchoCriterionValues(1.40712, 0.1630625, 0.151, 0.1523333, "audible", 0.0712, (0.25, 1.40712, nan)),
                        "music": EchoCriterionValues(1.6, 0.163, 0.1512, nan, "marginal", 0.08, (0.5, 1.6, 0.75))})
    bad = EchoCriterionChannelResult(
        channel_name="right", sample_rate_hz=48000, onset_samples=0, onset_seconds=0.0, status=3, criteria=(SPEECH,),
        curve_step_seconds=0.0, values_by_name={"speech": EchoCriterionValues(nan, nan, nan, nan, "NA", nan, None)})
    return [ok, bad]


def test_summary_text_format_is_pinned():
    from audio_analysis_amd.analyse.echo import summarise_echo_criterion_text
    assert summarise_echo_criterion_text(_hand_built()) == (
        "[left]\n"
        "Onset: 240 samples (5.000 ms)  Status: ok\n"
        "Criterion  EK_max  tau_max_ms  tau_10_ms  tau_50_ms  Rating\n"
        "speech  1.407  163.06  151.00  152.33  audible\n"
        "music  1.600  163.00  151.20  NA  marginal\n"
        "\n"
        "[right]\n"
        "Onset: 0 samples (0.000 ms)  Status: 3 (silent, too short)\n"
        "Criterion  EK_max  tau_max_ms  tau_10_ms  tau_50_ms  Rating\n"
        "speech  NA  NA  NA  NA  NA\n"
        "\n")
    assert summarise_echo_criterion_text([]) == ""


def test_summary_markdown_format_is_pinned():
    from audio_analysis_amd.analyse.echo import summarise_echo_criterion_markdown
    assert summarise_echo_criterion_markdown(_hand_built()[:1]) == (
        "### left\n"
        "\n"
        "Onset: 240 samples (5.000 ms). Status: ok.\n"
        "\n"
        "| Criterion | EK_max | tau_max (ms) | tau_10 (ms) | tau_50 (ms) | Rating |\n"
        "|---|---:|---:|---:|---:|---:|\n"
        "| speech | 1.407 | 163.06 | 151.00 | 152.33 | audible |\n"
        "| music | 1.600 | 163.00 | 151.20 | NA | marginal |\n"
        "\n")


def test_json_round_trip_keeps_nan_and_the_curve_only_when_computed():
    from audio_analysis_amd.analyse.echo import (echo_results_from_json, echo_results_to_json,
                                                 summarise_echo_criterion_text)
    res = _hand_built()
    doc = json.loads(json.dumps(echo_results_to_json(res)))             # strict JSON: no NaN tokens
    rows = doc["echo_criterion"]
    assert rows[0]["criteria"][0]["curve"] == [0.25, 1.40712, None] and rows[0]["criteria"][1]["first_tau_50_seconds"] is None
    assert "curve" not in rows[1]["criteria"][0] and rows[1]["criteria"][0]["rating"] == "NA"
    assert rows[0]["criteria"][0]["band_hz"] == [700.0, 1400.0] and rows[0]["curve_step_seconds"] == 0.001
    back = echo_results_from_json(doc)
    assert summarise_echo_criterion_text(back) == summarise_echo_criterion_text(res)
    bm, rm = back[0].values_by_name["music"], res[0].values_by_name["music"]
    assert back[0].criteria == res[0].criteria and math.isnan(bm.first_tau_50_seconds)
    assert (bm.ek_max, bm.tau_max_seconds, bm.first_tau_10_seconds, bm.rating, bm.build_up_seconds, bm.curve) == \
        (rm.ek_max, rm.tau_max_seconds, rm.first_tau_10_seconds, rm.rating, rm.build_up_seconds, rm.curve)
    assert back[0].values_by_name["speech"].curve[:2] == (0.25, 1.40712) and math.isnan(back[0].values_by_name["speech"].curve[2])
    assert back[1].values_by_name["speech"].curve is None and back[1].status == 3


def test_results_from_records_status_bits_and_curve_length():
    from audio_analysis_amd.analyse import echo as E
    nan = float("nan")
    good = [1.2, 7000.0, 6900.0, 6950.0, 0.07, 55.0, 9600.0, 1e5]
    rec = np.array([[good, [0.4, 10.0, -1.0, -1.0, 0.05, 40.0, 9600.0, 9e4]],
                    [good, [0.4, 10.0, -1.0, -1.0, 0.05, 40.0, 672.0, 9e4]],          # M == D for music: too short
                    [[nan, -1.0, -1.0, -1.0, nan, nan, 9600.0, nan], good],           # W[M-1] not finite
                    [[0.0, 0.0, -1.0, -1.0, 0.0, 0.0, 9600.0, 0.0]] * 2,              # silence
                    [[nan, -1.0, -1.0, -1.0, nan, 0.0, -30.0, 0.0]] * 2])             # M <= 0
    curve = np.full((5, 2, 200), nan, np.float32)
    curve[:, :, :200] = 0.25
    res = E.EchoRecords(criteria=(E.SPEECH, E.MUSIC), length=np.full(5, 12000), onset=np.array([5, 0, 0, 0, 0]),
                        peak_abs=np.array([1, 1, 1, 0, 1], np.float32), records=rec, curve=curve,
                        lag=np.array([432, 672]), step=48)
    out = E.echo_criterion_results(res, 48000, list("abcde"))
    assert [r.status for r in out] == [0, E.STATUS_TOO_SHORT, E.STATUS_NON_FINITE, E.STATUS_SILENT, E.STATUS_TOO_SHORT]
    v = out[0].values_by_name
    assert v["speech"].rating == "audible" and v["music"].rating == "inaudible" and out[0].onset_seconds == 5 / 48000
    assert v["speech"].tau_max_seconds == 7000.0 / 48000 and v["speech"].first_tau_10_seconds == 6900.0 / 48000
    assert math.isnan(v["music"].first_tau_10_seconds) and v["music"].build_up_seconds == 0.05
    assert len(v["speech"].curve) == 200 and out[0].curve_step_seconds == 0.001
    for r in out[1:]:
        for val in r.values_by_name.values():
            assert val.rating == "NA" and math.isnan(val.ek_max) and math.isnan(val.build_up_seconds)
            assert all(math.isnan(c) for c in val.curve)
    assert len(out[1].values_by_name["music"].curve) == 14 and out[4].values_by_name["music"].curve == ()


def test_cli_parser_defaults_and_help():
    from audio_analysis_amd.analyse import echo
    p = echo.build_parser()
    a = p.parse_args(["--input", "a.wav", "b.wav"])
    assert a.input == [Path("a.wav"), Path("b.wav")] and a.bundle is None
    assert (a.mono, a.criteria, a.onset_db, a.max_tau_ms, a.end_guard_ms, a.curve_step_ms, a.expected_sample_rate, a.json) == \
        (False, ["speech", "music"], -20.0, 1000.0, 50.0, 1.0, 48000, None)
    assert echo.settings_from_args(a) == echo.EchoCriterionSettings()
    a = p.parse_args(["--bundle", "d", "--mono", "--criteria", "music", "--onset-db", "-30", "--max-tau-ms", "400",
                      "--end-guard-ms", "20", "--curve-step-ms", "0", "--expected-sample-rate", "44100", "--json", "o.json"])
    s = echo.settings_from_args(a)
    assert a.bundle == Path("d") and s.criteria == (echo.MUSIC,) and s.onset_db == -30.0 and s.max_tau_ms == 400.0
    assert s.end_guard_ms == 20.0 and s.curve_step_ms == 0.0 and s.use_mono_downmix_for_stereo
    assert a.expected_sample_rate == 44100 and a.json == Path("o.json")
    for bad in ([], ["--input", "a.wav", "--bundle", "d"], ["--input", "a.wav", "--criteria", "film"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit):                                       # invalid settings end as a usage error
        echo.main(["--input", "a.wav", "--max-tau-ms", "-5"])
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.echo", "--help"], capture_output=True, text=True, cwd=str(REPO),
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--input", "--bundle", "--mono", "--criteria", "--onset-db", "--max-tau-ms", "--end-guard-ms",
                 "--curve-step-ms", "--expected-sample-rate", "--json"):
        assert flag in r.stdout


def test_shim_re_exports_the_module():
    import analyse.echo as shim
    from audio_analysis_amd.analyse import echo
    assert shim is echo


def test_echo_device_is_one_launch_over_every_channel_and_criterion():
    """The host side of echo_criterion_device on the recording engine: one ira_echo_criterion call whose job tables hold,
    per channel, one segment per criterion that reads the criterion's band row (criteria with equal edges the same one)."""
    from host_engine import HostEngine
    from audio_analysis_amd.analyse import echo as E
    from audio_analysis_amd.synth import synth_ir
    eng = HostEngine()
    lens = [60000, 5000, 7001]
    batch = eng.upload([synth_ir(i, 0, n, 48000) for i, n in enumerate(lens)])
    wide = E.EchoCriterion("wide", 2.0, 9.0, None, 1.0, 2.0)
    twin = E.EchoCriterion("twin", 0.5, 14.0, (700.0, 1400.0), 1.0, 2.0)
    st = E.EchoCriterionSettings(criteria=(wide, E.SPEECH, twin, E.MUSIC), max_tau_ms=100.0)
    res = E.echo_criterion_device(eng, batch, 48000, st)
    assert len(eng.calls("ira_band_irfft")) + len(eng.calls("ira_band_irfft_smooth")) >= 1
    calls = eng.calls("ira_echo_criterion")
    assert len(calls) == 1
    x, off, ln, chan, par, onset, nseg, max_len, params, nparam, ncurve, scratch, stash, rec, curve, stream = calls[0][1]
    assert (nseg, max_len, nparam, ncurve, stash) == (12, 4801, 4, 101, None)             # 1 + ceil(100 ms), its 48-sample steps
    assert rec[:2] == ("empty", 12 * 8) and curve[:2] == ("empty", 12 * 101)
    assert list(eng.table(ln)[:12]) == [60000] * 4 + [5000] * 4 + [7001] * 4
    assert list(eng.table(chan)[:12]) == [0] * 4 + [1] * 4 + [2] * 4 and list(eng.table(par)[:12]) == [0, 1, 2, 3] * 3
    o = eng.table(off)[:12].reshape(3, 4)
    assert np.all(o[:, 1] == o[:, 2])                                      # equal edges: one band signal
    assert np.all(o[:, 3] - o[:, 1] == np.array(lens))                     # the channel's second band follows its first
    assert o[1, 0] - o[0, 0] == 60000 and o[1, 1] - o[0, 1] == 2 * 60000
    p = np.array(params[: 4 * 8]).reshape(4, 8)
    assert list(p[:, 0]) == [2.0, 2.0 / 3.0, 0.5, 1.0] and list(p[:, 1]) == [432.0, 432.0, 672.0, 672.0]
    assert np.all(p[:, 2] == 2400.0) and np.all(p[:, 3] == 4801.0) and np.all(p[:, 4] == 48.0) and np.all(p[:, 7] == 48000.0)
    assert res.records.shape == (3, 4, 8) and res.curve.shape == (3, 4, 101) and list(res.lag) == [432, 432, 672, 672]
    # no curve, no bands, the stash switch
    eng.echo_stash = True
    res = E.echo_criterion_device(eng, batch, 48000, E.EchoCriterionSettings(criteria=(wide,), curve_step_ms=0.0, max_tau_ms=None))
    name, args = eng.calls("ira_echo_criterion")[1]
    assert name == "ira_echo_criterion[stash]" and args[6:11] == (3, 60000 - 2400, (2.0, 432.0, 2400.0, float(1 << 31), 0.0, 1.0, 2.0, 48000.0), 1, 0)
    assert args[12][:2] == ("empty", 3 * 15 * 4096) and res.curve is None and res.step == 0
    with pytest.raises(ValueError, match="param_of_seg"):
        eng.echo_criterion(batch.x, batch.off, batch.length, np.zeros(3, np.int32), batch.off_dev, np.ones((1, 8)), np.array([0, 1, 0]))
    with pytest.raises(ValueError, match="params must be"):
        eng.echo_criterion(batch.x, batch.off, batch.length, np.zeros(3, np.int32), batch.off_dev, np.ones((17, 8)), np.zeros(3, np.int32))


def test_echo_entry_points_validate_arguments_without_gpu():
    from audio_analysis_amd import _lib
    lib = _lib.load()
    E_NULL, E_SIZE = -1, -2

    def call(params=(2.0 / 3.0, 432.0, 2400.0, 48001.0, 48.0, 0.9, 1.0, 48000.0), nparam=1, **kw):
        # ira_echo_criterion(x, base_off, base_len, chan, param_of_seg, onset, nseg, max_len, params, nparam, ncurve,
        #                    scratch, stash, rec, curve, stream)
        a = dict(x=1, base_off=1, base_len=1, chan=1, par=1, onset=1, nseg=1, max_len=48001, ncurve=1001, scratch=1, stash=0,
                 rec=1, curve=1)
        a.update(kw)
        arr = (ctypes.c_double * max(1, len(params)))(*params) if params is not None else None
        return lib.ira_echo_criterion(a["x"], a["base_off"], a["base_len"], a["chan"], a["par"], a["onset"], a["nseg"],
                                      a["max_len"], arr, nparam, a["ncurve"], a["scratch"], a["stash"], a["rec"],
                                      a["curve"], 0)

    ok = (2.0 / 3.0, 432.0, 2400.0, 48001.0, 48.0, 0.9, 1.0, 48000.0)
    for name in ("x", "base_off", "base_len", "chan", "par", "onset", "scratch", "rec", "curve"):
        assert call(**{name: 0}) == E_NULL, name
    assert call(params=None) == E_NULL
    assert call(curve=0, ncurve=0, nseg=0) == 0                          # no curve: the pointer may be NULL
    assert call(nseg=0) == 0                                             # empty batch: nothing to do

    def with_(i, v):
        p = list(ok)
        p[i] = v
        return tuple(p)

    nan, inf = float("nan"), float("inf")
    for i, v in ((0, 0.0), (0, -1.0), (0, nan), (0, inf),                # exponent not finite or <= 0
                 (1, 0.0), (1, 2049.0), (1, 432.5), (1, nan),            # D outside 1 .. the halo capacity (2048)
                 (2, -1.0), (2, nan), (3, -1.0), (3, float((1 << 31) + 1)), (4, -1.0), (4, 0.5),
                 (5, nan), (5, inf), (6, nan), (6, -inf),                # thresholds not finite
                 (7, 0.0), (7, nan)):
        assert call(params=with_(i, v)) == E_SIZE, (i, v)
    assert call(params=with_(1, 2048.0), nseg=0) == 0 and call(params=with_(1, 1344.0), nseg=0) == 0   # 14 ms at 96 kHz
    assert call(params=ok + with_(0, nan), nparam=2) == E_SIZE           # every set is checked
    for kw in (dict(nparam=0), dict(nparam=17), dict(nseg=-1), dict(nseg=65536), dict(max_len=-1),
               dict(max_len=(1 << 31) + 1), dict(ncurve=-1)):
        assert call(**kw) == E_SIZE, kw
    # scratch: 8 doubles per segment and 6 per (segment, 4096-sample chunk of the longest evaluation)
    assert lib.ira_echo_scratch_doubles(3, 4096 * 2 + 1) == 3 * (8 + 6 * 3)
    assert lib.ira_echo_scratch_doubles(1, 4096) == 14 and lib.ira_echo_scratch_doubles(5, 0) == 40
    assert lib.ira_echo_scratch_doubles(0, 100) == 0
    for bad in ((-1, 100), (65536, 100), (1, -1), (1, (1 << 31) + 1)):
        assert lib.ira_echo_scratch_doubles(*bad) == E_SIZE, bad
