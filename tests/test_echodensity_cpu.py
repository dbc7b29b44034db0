"""
CPU-only tests of the normalized echo density (audio_analysis_amd.analyse.echodensity): sample counts, the host-built
weights, settings validation, status words, the fixed text / Markdown / JSON formats on hand-built results, the command
line, the header's constants, the argument checks of ira_echo_density (they return before touching a device), the host
side of the device function on the recording engine, and the restatement of tests/echodensity_ref.py against itself in
float64 and long double.
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

import echodensity_ref as R

REPO = Path(__file__).resolve().parent.parent


def test_sample_counts_at_common_rates():
    from audio_analysis_amd.analyse import echodensity as D
    assert [D.half_window_samples(20.0, fs) for fs in (22050, 44100, 48000, 96000)] == [221, 441, 480, 960]
    assert [2 * D.half_window_samples(20.0, fs) + 1 for fs in (22050, 44100, 48000, 96000)] == [443, 883, 961, 1921]
    assert D.half_window_samples(20.0, 192000) == 1920 and D.half_window_samples(0.001, 8000) == 1
    assert [D.step_samples(1.0, fs) for fs in (22050, 44100, 48000, 96000)] == [22, 44, 48, 96]
    assert D.step_samples(0.0, 48000) == 1 and D.step_samples(0.001, 48000) == 1
    for fs in (22050, 44100, 48000, 96000):
        for ms in (20.0, 10.0, 1.0, 33.3):
            assert D.half_window_samples(ms, fs) == R.half_window(ms, fs) == max(1, math.floor(ms * fs / 2000.0 + 0.5))
            assert D.step_samples(ms, fs) == R.step_of(ms, fs) == max(1, math.floor(ms * fs / 1000.0 + 0.5))
            for step in (1, 7, D.step_samples(1.0, fs)):
                assert D.max_positions(ms, fs, step) == R.kmax_of(ms, fs, step) == 1 + math.ceil(ms * fs / 1000.0) // step
    assert D.max_positions(None, 48000, 48) == 1 << 31 and D.max_positions(0.0, 48000, 48) == 1
    assert D.max_positions(100.0, 48000, 48) == 101 and D.max_positions(100.0, 44100, 44) == 101
    # K: nothing at or after the onset, one sample, L - 1 - o an exact multiple of S and one sample either side of it
    assert D.position_count(0, 0, 1, 1 << 31) == 0 and D.position_count(100, 100, 1, 1 << 31) == 0
    assert D.position_count(100, 250, 48, 1 << 31) == 0 and D.position_count(1, 0, 48, 1 << 31) == 1
    for o in (0, 5, 480):
        for s in (1, 7, 48, 96):
            for m in (0, 1, 9):
                n = o + m * s + 1                                            # L - 1 - o == m S
                assert D.position_count(n, o, s, 1 << 31) == m + 1 == R.count(n, o, s, 1 << 31)
                assert D.position_count(n - 1, o, s, 1 << 31) == (m if s > 1 or m > 0 else 0)
                assert D.position_count(n + s - 1, o, s, 1 << 31) == m + 1
                assert D.position_count(n + s, o, s, 1 << 31) == m + 2
                assert D.position_count(n, o, s, 3) == min(m + 1, 3)


def test_host_built_weights():
    from audio_analysis_amd.analyse.echodensity import window_weights
    for delta in (1, 2, 31, 480, 2048):
        w = window_weights(delta, "hann")
        assert w.dtype == np.float64 and w.shape == (2 * delta + 1,)
        assert np.all(w > 0.0) and w[delta] == 1.0                           # no zero end points, the centre is 1; symmetric to the rounding of
        #                                                                      the cosine's argument (3 ulp of 2 pi, halved: 2e-15)
        assert np.allclose(w, w[::-1], rtol=0.0, atol=2e-15) and np.all(np.diff(w[: delta + 1]) > 0.0)
        assert np.allclose(w, np.hanning(2 * delta + 3)[1:-1], rtol=0.0, atol=2e-15)
        assert np.array_equal(w, R.weights(delta, "hann")) or np.allclose(w, R.weights(delta, "hann"), rtol=0.0, atol=2e-15)
        r = window_weights(delta, "rect")
        assert r.dtype == np.float64 and np.array_equal(r, np.ones(2 * delta + 1))
    with pytest.raises(ValueError, match="window"):
        window_weights(3, "hamming")


def test_settings_defaults_and_validation():
    from audio_analysis_amd.analyse.echodensity import EchoDensitySettings
    s = EchoDensitySettings()
    assert (s.window_ms, s.window, s.step_ms, s.max_time_ms, s.thresholds, s.onset_db, s.use_mono_downmix_for_stereo) == \
        (20.0, "hann", 1.0, None, (1.0,), -20.0, False)
    assert s.rel_energy == 10.0 ** (-20.0 / 10.0)
    assert EchoDensitySettings(thresholds=[0.5, 0.9, 1], step_ms=0, max_time_ms=250).thresholds == (0.5, 0.9, 1.0)
    nan, inf = float("nan"), float("inf")
    for bad, what in [(dict(window_ms=0.0), "window_ms"), (dict(window_ms=nan), "window_ms"), (dict(window_ms=inf), "window_ms"),
                      (dict(window="hamming"), "window must"), (dict(step_ms=-1.0), "step_ms"), (dict(step_ms=nan), "step_ms"),
                      (dict(max_time_ms=-1.0), "max_time_ms"), (dict(max_time_ms=inf), "max_time_ms"),
                      (dict(thresholds=()), "1 to 3"), (dict(thresholds=(0.5, 0.7, 0.9, 1.0)), "1 to 3"),
                      (dict(thresholds=(nan,)), "finite"), (dict(thresholds=(0.0,)), "> 0"), (dict(thresholds=(-1.0,)), "> 0"),
                      (dict(thresholds=(1.0, 0.5)), "ascend"), (dict(thresholds=(1.0, 1.0)), "ascend"),
                      (dict(thresholds=1.0), "sequence"), (dict(thresholds=("a",)), "sequence"),
                      (dict(onset_db=1.0), "onset_db"), (dict(onset_db=nan), "onset_db")]:
        with pytest.raises(ValueError, match=what):
            EchoDensitySettings(**bad)


def _hand_built():
    from audio_analysis_amd.analyse.echodensity import EchoDensityChannelResult
    nan = float("nan")
    ok = EchoDensityChannelResult(
        channel_name="left", sample_rate_hz=48000, onset_samples=240, onset_seconds=0.005, status=0, window_ms=20.0,
        window="hann", window_samples=961, step_seconds=0.001, thresholds=(0.9, 1.0), mixing_time_seconds=(0.062, nan),
        eta_max=0.98765, tau_max_seconds=0.1234, profile=np.array([0.25, nan, 0.5], np.float32))
    bad = EchoDensityChannelResult(
        channel_name="right", sample_rate_hz=48000, onset_samples=0, onset_seconds=0.0, status=3, window_ms=10.0,
        window="rect", window_samples=481, step_seconds=1.0 / 48000, thresholds=(1.0,), mixing_time_seconds=(nan,),
        eta_max=nan, tau_max_seconds=nan, profile=None)
    return [ok, bad]


def test_summary_text_format_is_pinned():
    from audio_analysis_amd.analyse.echodensity import summarise_echo_density_text
    assert summarise_echo_density_text(_hand_built()) == (
        "[left]\n"
        "Onset: 240 samples (5.000 ms)  Status: ok  Window: hann 20 ms (961 samples)  Step: 1.000 ms\n"
        "Threshold  mixing_time_ms\n"
        "0.9  62.00\n"
        "1  NA\n"
        "eta_max: 0.988 at 123.40 ms\n"
        "\n"
        "[right]\n"
        "Onset: 0 samples (0.000 ms)  Status: 3 (silent, too short)  Window: rect 10 ms (481 samples)  Step: 0.021 ms\n"
        "Threshold  mixing_time_ms\n"
        "1  NA\n"
        "eta_max: NA at NA ms\n"
        "\n")
    assert summarise_echo_density_text([]) == ""


def test_summary_markdown_format_is_pinned():
    from audio_analysis_amd.analyse.echodensity import summarise_echo_density_markdown
    assert summarise_echo_density_markdown(_hand_built()[:1]) == (
        "### left\n"
        "\n"
        "Onset: 240 samples (5.000 ms). Status: ok. Window: hann 20 ms (961 samples). Step: 1.000 ms.\n"
        "\n"
        "| Threshold | mixing time (ms) |\n"
        "|---|---:|\n"
        "| 0.9 | 62.00 |\n"
        "| 1 | NA |\n"
        "\n"
        "eta_max: 0.988 at 123.40 ms.\n"
        "\n")


def test_json_round_trip_keeps_nan_and_drops_the_profile_on_request():
    from audio_analysis_amd.analyse.echodensity import (echo_density_results_from_json, echo_density_results_to_json,
                                                        summarise_echo_density_text)
    res = _hand_built()
    doc = json.loads(json.dumps(echo_density_results_to_json(res), allow_nan=False))       # strict JSON: no NaN tokens
    rows = doc["echo_density"]
    assert rows[0]["profile"] == [0.25, None, 0.5] and rows[0]["mixing_time_seconds"] == [0.062, None]
    assert "profile" not in rows[1] and rows[1]["eta_max"] is None and rows[1]["tau_max_seconds"] is None
    assert rows[0]["thresholds"] == [0.9, 1.0] and rows[0]["step_seconds"] == 0.001 and rows[0]["window_samples"] == 961
    assert set(rows[0]) == {"channel_name", "sample_rate_hz", "onset_samples", "onset_seconds", "status", "window_ms",
                            "window", "window_samples", "step_seconds", "thresholds", "mixing_time_seconds", "eta_max",
                            "tau_max_seconds", "profile"}
    back = echo_density_results_from_json(doc)
    assert summarise_echo_density_text(back) == summarise_echo_density_text(res)
    assert math.isnan(back[1].eta_max) and back[1].profile is None and back[1].status == 3
    assert back[0].profile.dtype == np.float32 and np.array_equal(back[0].profile, res[0].profile, equal_nan=True)
    assert back[0].mixing_time_seconds[0] == 0.062 and math.isnan(back[0].mixing_time_seconds[1])
    slim = echo_density_results_to_json(res, with_profile=False)
    assert all("profile" not in r for r in slim["echo_density"])
    assert echo_density_results_from_json(json.loads(json.dumps(slim)))[0].profile is None


def test_results_from_records_status_bits():
    from audio_analysis_amd.analyse import echodensity as D
    nan = float("nan")
    st = D.EchoDensitySettings(thresholds=(0.5, 1.0))
    rec = np.array([[5.0, 0.0, 0.0, 1.25, 3.0, 1.0, 3.0, -1.0],               # fine
                    [5.0, 0.0, 0.0, 0.75, 2.0, 1.0, -1.0, -1.0],              # never reaches 1.0
                    [5.0, 0.0, 2.0, 1.25, 3.0, 1.0, 3.0, -1.0],               # two windows with a non-finite sum
                    [5.0, 5.0, 0.0, nan, -1.0, -1.0, -1.0, -1.0],             # silence
                    [2.0, 0.0, 0.0, 1.25, 1.0, 0.0, 1.0, -1.0],               # L - o < W
                    [0.0, 0.0, 0.0, nan, -1.0, -1.0, -1.0, -1.0]])            # empty channel
    prof = np.arange(30, dtype=np.float32) / 8
    res = D.EchoDensityRecords(settings=st, length=np.array([2000, 2000, 2000, 2000, 1060, 0]), onset=np.array([100, 0, 0, 0, 100, 0]),
                               peak_abs=np.array([1, 1, 1, 0, 1, 0], np.float32), records=rec, profile=prof,
                               profile_off=np.arange(6) * 5, delta=480, step=48)
    out = D.echo_density_results(res, 48000, list("abcdef"))
    assert [r.status for r in out] == [0, 0, D.STATUS_NON_FINITE, D.STATUS_SILENT, D.STATUS_TOO_SHORT,
                                       D.STATUS_SILENT | D.STATUS_TOO_SHORT]
    a = out[0]
    assert a.mixing_time_seconds == (48 / 48000, 3 * 48 / 48000) and a.eta_max == 1.25 and a.tau_max_seconds == 3 * 48 / 48000
    assert a.profile.dtype == np.float32 and list(a.profile) == [0.0, 0.125, 0.25, 0.375, 0.5] and a.step_seconds == 0.001 and a.window_samples == 961
    assert a.onset_samples == 100 and a.onset_seconds == 100 / 48000 and a.thresholds == (0.5, 1.0)
    assert out[1].mixing_time_seconds[0] == 0.001 and math.isnan(out[1].mixing_time_seconds[1])
    assert list(out[1].profile) == [0.625, 0.75, 0.875, 1.0, 1.125]
    for r in out[2:]:
        assert math.isnan(r.eta_max) and math.isnan(r.tau_max_seconds) and all(math.isnan(v) for v in r.mixing_time_seconds)
        assert all(math.isnan(v) for v in r.profile)
    assert [len(r.profile) for r in out] == [5, 5, 5, 5, 2, 0]
    assert D.echo_density_results(res, 48000, list("abcdef"), keep_profile=False)[0].profile is None
    assert D.status_text(0) == "ok" and D.status_text(6) == "6 (too short, non-finite)"


def test_cli_parser_defaults_and_help_through_the_shim():
    import analyse.echodensity as shim
    from audio_analysis_amd.analyse import echodensity as D
    assert shim is D
    p = D.build_parser()
    a = p.parse_args(["--input", "a.wav", "b.wav"])
    assert a.input == [Path("a.wav"), Path("b.wav")] and a.bundle is None
    assert (a.mono, a.window_ms, a.window, a.step_ms, a.max_time_ms, a.thresholds, a.onset_db, a.no_profile,
            a.expected_sample_rate, a.json) == (False, 20.0, "hann", 1.0, None, [1.0], -20.0, False, 48000, None)
    assert D.settings_from_args(a) == D.EchoDensitySettings()
    a = p.parse_args(["--bundle", "d", "--mono", "--window-ms", "10", "--window", "rect", "--step-ms", "0", "--max-time-ms",
                      "400", "--thresholds", "0.5", "0.9", "1", "--onset-db", "-30", "--no-profile",
                      "--expected-sample-rate", "44100", "--json", "o.json"])
    s = D.settings_from_args(a)
    assert a.bundle == Path("d") and (s.window_ms, s.window, s.step_ms, s.max_time_ms) == (10.0, "rect", 0.0, 400.0)
    assert s.thresholds == (0.5, 0.9, 1.0) and s.onset_db == -30.0 and s.use_mono_downmix_for_stereo and a.no_profile
    assert a.expected_sample_rate == 44100 and a.json == Path("o.json")
    for bad in ([], ["--input", "a.wav", "--bundle", "d"], ["--input", "a.wav", "--window", "hamming"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit):                                       # invalid settings end as a usage error
        D.main(["--input", "a.wav", "--thresholds", "1.0", "0.5"])
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.echodensity", "--help"], capture_output=True, text=True,
                       cwd=str(REPO), env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--input", "--bundle", "--mono", "--window-ms", "--window", "--step-ms", "--max-time-ms", "--thresholds",
                 "--onset-db", "--no-profile", "--expected-sample-rate", "--json"):
        assert flag in r.stdout


def test_header_constants_symbol_and_abi_version():
    from audio_analysis_amd import _lib, engine
    from audio_analysis_amd.analyse import echodensity as D
    hdr = (REPO / "include" / "ira.h").read_text()
    for name in ("DOUBLES", "TILE", "MAX_DELTA", "MAX_THRESHOLDS"):
        assert re.search(rf"#define IRA_NED_{name} {getattr(engine, 'NED_' + name)}\b", hdr), name
    assert f"#define IRA_NED_NAN_SILENT {engine.NED_NAN_SILENT:#x}u" in hdr
    assert f"#define IRA_NED_NAN_NONFINITE {engine.NED_NAN_NONFINITE:#x}u" in hdr
    assert D.MAX_DELTA_SAMPLES == engine.NED_MAX_DELTA == 2048 and D.MAX_THRESHOLDS == 3 and engine.NED_DOUBLES == 8
    assert D.GAUSSIAN_FRACTION == R.E == math.erfc(1.0 / math.sqrt(2.0)) or abs(D.GAUSSIAN_FRACTION - math.erfc(1.0 / math.sqrt(2.0))) < 1e-16
    src = (REPO / "audio_analysis_amd" / "csrc" / "ira_echodensity.hip").read_text()
    assert f"NED_SLOTS = {engine.NED_SLOTS};" in src and "0.31731050786291415" in src
    assert "#define IRA_ABI_VERSION 15 " in hdr and _lib.ABI_VERSION == 15
    assert "ira_echo_density" in _lib.PROTOTYPES and re.search(r"int32_t ira_echo_density\(", hdr)
    lib = _lib.load()
    assert lib.ira_abi_version() == 15 and lib.ira_echo_density is not None
    # positions per workgroup: the full tile at one sample per step up to 20 ms at 192 kHz, fewer when the span grows
    assert engine.ned_tile_positions(480, 1) == engine.ned_tile_positions(1920, 1) == engine.NED_TILE
    assert engine.ned_tile_positions(2048, 1) == 1024 and engine.ned_tile_positions(480, 48) == 85
    assert engine.ned_tile_positions(2048, 4102) == 1 and engine.ned_tile_positions(2048, 4000) == 1
    assert engine.ned_tile_positions(2, 48) == 105 and engine.ned_tile_positions(480, 961) == 5


def test_entry_point_validates_arguments_without_gpu():
    from audio_analysis_amd import _lib
    lib = _lib.load()
    E_NULL, E_SIZE = -1, -2

    def call(thresholds=(1.0,), **kw):
        # ira_echo_density(x, off, len, onset, nch, w, delta, step, kmax, thresholds, nthr, prof, prof_off, rec, stream)
        a = dict(x=1, off=1, len=1, onset=1, nch=0, w=1, delta=480, step=48, kmax=1 << 31, nthr=len(thresholds or ()),
                 prof=1, prof_off=1, rec=1)
        a.update(kw)
        arr = (ctypes.c_double * max(1, len(thresholds)))(*thresholds) if thresholds is not None else None
        return lib.ira_echo_density(a["x"], a["off"], a["len"], a["onset"], a["nch"], a["w"], a["delta"], a["step"],
                                    a["kmax"], arr, a["nthr"], a["prof"], a["prof_off"], a["rec"], 0)

    assert call() == 0                                                     # nch == 0: nothing to do
    for name in ("x", "off", "len", "onset", "w", "prof", "prof_off", "rec"):
        assert call(**{name: 0}) == E_NULL, name
    assert call(thresholds=None, nthr=1) == E_NULL and call(thresholds=None, nthr=0) == 0
    for kw in (dict(delta=0), dict(delta=2049), dict(delta=-1), dict(step=0), dict(step=-3), dict(nthr=4), dict(nthr=-1),
               dict(nch=-1), dict(nch=65536), dict(kmax=-1), dict(kmax=(1 << 31) + 1)):
        assert call(**kw) == E_SIZE, kw
    nan, inf = float("nan"), float("inf")
    for thr in ((nan,), (inf,), (1.0, -inf), (0.5, 0.9, nan)):
        assert call(thresholds=thr) == E_SIZE, thr
    assert call(delta=1) == 0 and call(delta=2048) == 0 and call(step=1) == 0 and call(thresholds=(0.5, 0.9, 1.0)) == 0
    assert call(thresholds=(), nthr=0) == 0 and call(kmax=0) == 0
    assert call(delta=0, nch=1) == E_SIZE and call(x=0, nch=1) == E_NULL       # refused before any launch


def test_echo_density_device_is_one_launch_over_every_channel():
    """The host side of echo_density_device on the recording engine: one ira_echo_density call whose tables hold the
    channels' offsets and lengths, the host-built weights, the profile offsets of onset 0, delta, S, Kmax and the
    thresholds."""
    from host_engine import HostEngine
    from audio_analysis_amd.analyse import echodensity as D
    from audio_analysis_amd.synth import synth_ir
    eng = HostEngine()
    lens = [60000, 5000, 7001]
    batch = eng.upload([synth_ir(i, 0, n, 48000) for i, n in enumerate(lens)])
    st = D.EchoDensitySettings(thresholds=(0.5, 1.0), max_time_ms=100.0)
    res = D.echo_density_device(eng, batch, 48000, st)
    assert len(eng.calls("ira_onset_index")) == 1
    calls = eng.calls("ira_echo_density")
    assert len(calls) == 1 and calls[0][0] == "ira_echo_density"
    x, off, ln, onset, nch, w, delta, step, kmax, thr, nthr, prof, prof_off, rec, stream = calls[0][1]
    assert (nch, delta, step, kmax, nthr, stream) == (3, 480, 48, 101, 2, None)      # 1 + ceil(100 ms) // 48
    assert thr[:2] == (0.5, 1.0)
    assert list(eng.table(off)[:3]) == list(batch.off) and list(eng.table(ln)[:3]) == lens
    assert np.array_equal(eng.table(w)[:961], D.window_weights(480, "hann"))
    assert list(eng.table(prof_off)[:3]) == [0, 101, 202]                          # every row: Kmax positions
    assert prof[:3] == ("empty", 303, "torch.float32") and rec[:3] == ("empty", 24, "torch.float64")
    assert onset[0] == "empty" and x[0] == "up"
    assert res.records.shape == (3, 8) and res.profile.shape == (303,) and list(res.profile_off) == [0, 101, 202]
    assert (res.delta, res.step) == (480, 48) and list(res.length) == lens
    # one sample per step, the whole channel, rect: the rows are sized by the lengths
    st = D.EchoDensitySettings(window="rect", window_ms=10.0, step_ms=0.0)
    res = D.echo_density_device(eng, batch, 48000, st)
    args = eng.calls("ira_echo_density")[1][1]
    assert args[4:5] + args[6:9] + args[10:11] == (3, 240, 1, 1 << 31, 1) and args[9][:1] == (1.0,)
    assert np.array_equal(eng.table(args[5])[:481], np.ones(481)) and list(eng.table(args[12])[:3]) == [0, 60000, 65000]
    assert args[11][:2] == ("empty", 72001)
    # an empty batch launches nothing
    empty = eng.upload([])
    n_before = len(eng.calls("ira_echo_density"))
    res = D.echo_density_device(eng, empty, 48000, st)
    assert len(eng.calls("ira_echo_density")) == n_before and res.records.shape == (0, 8)
    with pytest.raises(ValueError, match="at most 4097"):
        D.echo_density_device(eng, batch, 192000, D.EchoDensitySettings(window_ms=25.0))
    for bad, what in ((dict(delta=0), "delta"), (dict(weights=np.ones(5)), "weights"), (dict(step=0), "step"),
                      (dict(thresholds=(1, 2, 3, 4)), "thresholds")):
        kw = dict(weights=np.ones(7), delta=3, step=1, kmax=10, thresholds=(1.0,))
        kw.update(bad)
        with pytest.raises(ValueError, match=what):
            eng.echo_density(batch.x, batch.off, batch.length, batch.off_dev, **kw)


# ------------------------------------------------------------------------------------------------ the restatement
def _both(x, onset, delta, window, step):
    lo = R.profile(x, onset, delta, window, step, dtype=np.float64)
    hi = R.profile(x, onset, delta, window, step, dtype=np.longdouble)
    assert np.array_equal(lo[1], hi[1])                                       # the same positions are NaN, of the same kind
    assert np.all(lo[2] == 0) and np.all(hi[2] == 0)                          # no ambiguous sample in either precision
    ok = lo[1] == 0
    err = np.abs(lo[0][ok] - hi[0][ok].astype(np.float64))
    assert np.all(err <= (2.0 * (2 * delta + 1) + 16.0) * 2.0 ** -53 * hi[0][ok].astype(np.float64))
    return hi[0].astype(np.float64), hi[1]


@pytest.mark.parametrize("window", ["hann", "rect"])
def test_restatement_gaussian_noise_gives_one(window):
    """A decaying Gaussian: away from the edges the mean of eta lies within 0.02 of 1 (the window's own sigma follows
    the decay, which is slow against 20 ms)."""
    x = R.decaying_gaussian(12000)
    eta, kind = _both(x, 0, 100, window, 1)
    assert eta.size == 12000 and np.all(kind == 0)
    inner = eta[200:-200]
    assert abs(float(inner.mean()) - 1.0) <= 0.02, float(inner.mean())
    eta20, _ = _both(x, 0, 480, window, 48)
    assert abs(float(eta20[12:-12].mean()) - 1.0) <= 0.02, float(eta20[12:-12].mean())


def test_restatement_thickening_poisson_train_rises():
    x = R.thickening_poisson(20000)
    o = R.onset_index(x)
    assert o == 0
    eta, kind = _both(x, o, 480, "hann", 48)
    assert np.all(kind == 0)
    q = eta.size // 4
    means = [float(eta[i * q : (i + 1) * q].mean()) for i in range(4)]
    assert means[0] < means[1] < means[2] < means[3], means
    assert means[0] < 0.35 and means[3] > 0.8, means


@pytest.mark.parametrize("window", ["hann", "rect"])
def test_restatement_constant_magnitude_gives_exactly_zero(window):
    rng = np.random.default_rng(5)
    for a in (0.25, 0.3):
        x = (a * rng.choice([-1.0, 1.0], 1500)).astype(np.float32)
        for delta, step in ((100, 1), (1, 1), (480, 7)):
            for dtype in (np.float64, np.longdouble):
                eta, kind, amb, _ = R.profile(x, 0, delta, window, step, dtype=dtype)
                assert np.all(kind == 0) and np.all(eta == 0.0), (a, delta, step, dtype)
    # a window of one sample: a one-sample channel, both neighbours clipped away
    eta, kind, _, a_sum = R.profile(np.array([0.7], np.float32), 0, 1, window, 1)
    assert eta.size == 1 and kind[0] == 0 and eta[0] == 0.0


def test_restatement_edges_and_nan_kinds():
    x = R.decaying_gaussian(3000, seed=3)
    x[:500] = 0.0
    x[1500] = np.inf
    x[2500] = np.nan
    eta, kind, amb, a = R.profile(x, 0, 50, "hann", 1)
    assert np.all(kind[:450] == 1) and kind[449] == 1 and kind[450] == 0       # the window of 450 reaches sample 500
    assert np.all(kind[1450:1551] == 2) and kind[1449] == 0 and kind[1551] == 0
    assert np.all(kind[2450:2551] == 2) and np.all(np.isnan(eta[kind != 0])) and np.all(np.isfinite(eta[kind == 0]))
    w = R.weights(50, "hann")
    assert a[0] == pytest.approx(float(w[50:].sum()), rel=1e-15) and a[100] == pytest.approx(float(w.sum()), rel=1e-15)
    assert a[-1] == pytest.approx(float(w[:51].sum()), rel=1e-15)
    rec = R.record(np.array([0.5, np.nan, 1.5, 1.5, 0.25], np.float32), (1.0, 1.5, 2.0))
    assert list(rec) == [5.0, 1.0, 0.0, 1.5, 2.0, 2.0, 2.0, -1.0]
    odd = np.array([0x7fc00001, 0x7fc00000, 0x7fc00001], np.uint32).view(np.float32)
    rec = R.record(odd, (1.0,))
    assert list(rec[:3]) == [3.0, 1.0, 2.0] and np.isnan(rec[3]) and list(rec[4:]) == [-1.0] * 4
