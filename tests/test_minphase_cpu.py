"""
CPU-only tests of the minimum-phase / excess-phase module (audio_analysis_amd.analyse.minphase): settings validation, the
size and bin rules against hand-computed values, the sub-batch cut, the host arithmetic on hand-built records, the text,
Markdown and JSON formats, the command line's parser and the shim, the header's constants and symbols, the argument checks
of the C entry points (they return before touching a device), the host side of the device functions on the recording
engine, and the float64 restatement (tests/minphase_ref.py) against the analytic cases and its own bounds.
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

import minphase_ref as R

REPO = Path(__file__).resolve().parent.parent
FS = 48000


# ------------------------------------------------------------------------------------------------ settings, sizes, bins
def test_settings_defaults_and_validation():
    from audio_analysis_amd.analyse import minphase as D
    s = D.MinPhaseSettings()
    assert (s.oversample, s.post_ms, s.floor_db, s.points_per_octave, s.f_min_hz, s.f_max_hz, s.centre, s.onset_db,
            s.use_mono_downmix_for_stereo) == (4, None, -120.0, 48, 20.0, 20000.0, "peak", -20.0, False)
    assert s.rel_energy == 10.0 ** (-20.0 / 10.0) and s.floor_ratio == 10.0 ** (-120.0 / 10.0)
    assert D.MinPhaseSettings(post_ms=5).post_ms == 5.0 and D.MinPhaseSettings(oversample=np.int64(8)).oversample == 8
    nan, inf = float("nan"), float("inf")
    bad = [(dict(oversample=1), "oversample"), (dict(oversample=2.5), "oversample"), (dict(oversample=True), "oversample"),
           (dict(post_ms=-1.0), "post_ms"), (dict(post_ms=nan), "post_ms"), (dict(post_ms="long"), "post_ms"),
           (dict(floor_db=0.0), "floor_db"), (dict(floor_db=-301.0), "floor_db"), (dict(floor_db=nan), "floor_db"),
           (dict(points_per_octave=0), "points_per_octave"), (dict(points_per_octave=1.5), "points_per_octave"),
           (dict(f_min_hz=0.0), "f_min_hz"), (dict(f_min_hz=100.0, f_max_hz=50.0), "f_max_hz"), (dict(f_max_hz=inf), "f_max_hz"),
           (dict(centre="middle"), "centre must"), (dict(onset_db=1.0), "onset_db")]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            D.MinPhaseSettings(**kw)


def test_sizes_bins_and_the_transform_limit():
    from audio_analysis_amd.analyse import fdw, minphase as D
    st = D.MinPhaseSettings()
    seg, n = D.minphase_sizes([5, 8, 9, 64, 100, 257, 4097, 480000, 0], [0] * 9, FS, st)
    assert list(seg) == [5, 8, 9, 64, 100, 257, 4097, 480000, 0] and seg.dtype == np.int64
    assert list(n) == [32, 32, 64, 256, 512, 2048, 32768, 1 << 21, 32]
    assert list(D.minphase_sizes([5, 64, 4097], [0] * 3, FS, D.MinPhaseSettings(oversample=16))[1]) == [128, 1024, 1 << 17]
    assert list(D.minphase_sizes([4097, 4096], [0, 0], FS, D.MinPhaseSettings(oversample=2))[1]) == [16384, 8192]
    # post_ms: D = min(L, p + 1 + rint(post_ms fs / 1000)); 2.5 ms are 120 samples, 0.01 ms round to 0
    seg, n = D.minphase_sizes([1000, 1000, 100], [10, 950, 99], FS, D.MinPhaseSettings(post_ms=2.5))
    assert list(seg) == [131, 1000, 100] and list(n) == [1024, 4096, 512]
    assert list(D.minphase_sizes([1000], [10], FS, D.MinPhaseSettings(post_ms=0.01))[0]) == [11]
    for i, (length, p) in enumerate(((1000, 10), (77, 3))):
        assert R.sizes(length, p, FS, 4, 2.5) == (int(seg[i]) if i == 0 else 77, int(n[i]) if i == 0 else 512)
    # the limit: 2^21 points, the message names both remedies
    assert D.minphase_sizes([1 << 19], [0], FS, st)[1][0] == 1 << 21
    with pytest.raises(ValueError, match=r"at most 2\^21: lower oversample or set post_ms"):
        D.minphase_sizes([10, (1 << 19) + 1], [0, 0], FS, st)
    assert D.minphase_sizes([(1 << 19) + 1], [100], FS, D.MinPhaseSettings(post_ms=100.0))[1][0] == 32768
    # the grid is fdw_grid's own
    grid = D.minphase_grid(st, FS)
    assert np.array_equal(grid, fdw.fdw_grid(fdw.FdwSettings(), FS)[0]) and grid.size == 479 and grid[0] == 20.0
    bins = D.minphase_bins(grid, [32, 256, 1 << 21], FS)
    assert bins.shape == (3, 479) and bins.dtype == np.int64
    assert bins[0].min() == 1 and bins[0].max() == 13 and bins[1].max() == 106 and bins[1, 0] == 1      # clipped from 0 up to 1
    assert bins[2, 0] == 874 and bins[2, 48] == 1748 and bins[2, -1] == int(np.rint(grid[-1] * (1 << 21) / FS))
    for row, nf in zip(bins, (32, 256, 1 << 21)):
        assert np.array_equal(row, R.grid_bins(nf, float(FS)))
    top = D.minphase_bins(np.array([1.0, 23999.9, 24000.0]), [64], FS)
    assert list(top[0]) == [1, 31, 31]                                    # never bin 0, never the Nyquist bin


def test_the_sub_batch_cut(monkeypatch):
    from audio_analysis_amd import engine
    assert engine.MINPHASE_SCRATCH_BYTES == 4 << 30
    assert list(engine.minphase_scratch_bytes([32, 1 << 21])) == [44 * 32 + 64, 44 * (1 << 21) + 64]
    assert engine.minphase_cut([]) == [] and engine.minphase_cut([256] * 5) == [(0, 5)]
    assert engine.minphase_cut([1 << 21] * 100) == [(0, 46), (46, 92), (92, 100)]       # 92.3 MB a channel: 46 in 4 GiB
    per = 44 * 256 + 64
    for budget, want in ((per, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]), (2 * per, [(0, 2), (2, 4), (4, 5)]),
                         (2 * per - 1, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]), (5 * per, [(0, 5)]), (1, [(i, i + 1) for i in range(5)])):
        monkeypatch.setattr(engine, "MINPHASE_SCRATCH_BYTES", budget)
        assert engine.minphase_cut([256] * 5) == want, budget
    monkeypatch.setattr(engine, "MINPHASE_SCRATCH_BYTES", 44 * 1024 + 64 + 2 * per)
    assert engine.minphase_cut([256, 1024, 256, 256, 256, 2048, 256]) == [(0, 3), (3, 5), (5, 6), (6, 7)]


# ------------------------------------------------------------------------------------------------ host arithmetic
def test_host_arithmetic_on_hand_built_records():
    from audio_analysis_amd.analyse import minphase as D
    n, p, fs = 64, 3, 6400.0                                                # bins are 100 Hz apart
    k = np.array([1, 8, 16, 31])
    rec = np.zeros((4, 8))
    rec[:, 0] = [1.0, 0.0, -2.0, 1e-7]                                      # Re X
    rec[:, 1] = [0.0, 1.0, 0.0, 0.0]                                        # Im X
    rec[:, 2:5] = [[0.0, 0.1, 0.2], [0.5, 0.5, 0.5], [-0.25, -0.5, -0.75], [1.0, 0.0, -1.0]]      # Im T at k - 1, k, k + 1
    rec[:, 5:8] = [[0.0, 0.0, 0.0], [0.1, 0.2, 0.3], [-7.0, -7.5, -8.0], [3.0, 3.0, 3.0]]         # excess at k - 1, k, k + 1
    v = D.minphase_arithmetic(rec, k, n, p, pmax=4.0, floored_bins=3, sample_rate_hz=fs, floor_db=-120.0)
    assert list(v["frequencies_hz"]) == [100.0, 800.0, 1600.0, 3100.0] and list(v["bin"]) == [1, 8, 16, 31]
    assert list(v["floored"]) == [False, False, False, True] and v["floored_share"] == 3 / 33
    assert v["level_db"][0] == 0.0 and v["level_db"][2] == 10.0 * np.log10(4.0) and v["level_db"][3] == 10.0 * np.log10(4e-12)
    # phi_rel: angle + 2 pi frac(k p / N): 3/64, 24/64, 48/64 and 93/64 -> 29/64 turns
    want = np.degrees(R.wrap(np.array([0.0, np.pi / 2, np.pi, 0.0]) + 2 * np.pi * np.array([3, 24, 48, 29]) / 64.0))
    assert np.array_equal(v["phase_deg"], want) and abs(v["phase_deg"][1] + 135.0) < 1e-12 and abs(v["phase_deg"][2] - 90.0) < 1e-12
    assert np.array_equal(v["minimum_phase_deg"], np.degrees(2.0 * rec[:, 3]))
    assert np.array_equal(v["excess_phase_deg"], np.degrees(rec[:, 6])) and v["excess_phase_deg"][2] < -360.0       # never wrapped
    step = 4.0 * math.pi / n
    assert np.array_equal(v["excess_group_delay_seconds"], -(rec[:, 7] - rec[:, 5]) / step / fs)
    assert abs(v["excess_group_delay_seconds"][1] + 0.2 / step / fs) < 1e-18 and v["excess_group_delay_seconds"][3] == 0.0
    assert np.array_equal(v["minimum_group_delay_seconds"], -(2.0 * rec[:, 4] - 2.0 * rec[:, 2]) / step / fs)
    assert abs(v["minimum_group_delay_seconds"][3] - 4.0 / step / fs) < 1e-18
    power = rec[:, 0] ** 2 + rec[:, 1] ** 2
    tau = -(rec[:, 7] - rec[:, 5]) / step
    assert v["excess_delay_seconds"] == float(np.sum(power * tau)) / float(np.sum(power)) / fs
    assert v["excess_phase_span_deg"] == np.degrees(3.0) - np.degrees(-7.5)
    # a higher floor: more points are floored and held at the floor's level
    w = D.minphase_arithmetic(rec, k, n, p, 4.0, 0, fs, floor_db=-3.0)
    assert list(w["floored"]) == [True, True, False, True] and w["level_db"][0] == 10.0 * np.log10(4.0 * 10.0 ** -0.3)
    # without values: silence, a NaN, an infinity
    for pmax in (0.0, float("nan"), float("inf")):
        z = D.minphase_arithmetic(np.full((4, 8), np.nan), k, n, p, pmax, 0, fs)
        for name in ("level_db", "phase_deg", "minimum_phase_deg", "excess_phase_deg", "excess_group_delay_seconds",
                     "minimum_group_delay_seconds"):
            assert np.isnan(z[name]).all(), (pmax, name)
        assert not z["floored"].any() and list(z["frequencies_hz"]) == [100.0, 800.0, 1600.0, 3100.0]
        assert math.isnan(z["floored_share"]) and math.isnan(z["excess_delay_seconds"]) and math.isnan(z["excess_phase_span_deg"])
    # the restatement's own records go through the same arithmetic
    ref = R.chain(R.min_phase_fir(), 0, 6, 256)
    bins = R.grid_bins(256, float(FS))
    v = D.minphase_arithmetic(R.records(ref, bins), bins, 256, 0, ref["P"], 0, FS)
    assert np.array_equal(v["minimum_phase_deg"], np.degrees(ref["phi_min"][bins]))
    assert np.array_equal(v["excess_group_delay_seconds"], ref["tau_e"][bins] / FS)
    assert np.array_equal(v["minimum_group_delay_seconds"], ref["tau_min"][bins] / FS) and not v["floored"].any()
    assert np.array_equal(v["level_db"], 10.0 * np.log10(ref["power"][bins]))


def _hand_built():
    from audio_analysis_amd.analyse.minphase import MinPhaseChannelResult
    nan = float("nan")
    full = MinPhaseChannelResult(
        channel_name="left", sample_rate_hz=48000, centre="peak", centre_samples=240, centre_seconds=0.005,
        segment_samples=4800, fft_size=32768, floor_db=-120.0, points_per_octave=2, floored_share=0.03125,
        excess_delay_seconds=0.00125, excess_phase_span_deg=181.25,
        frequencies_hz=np.array([20.5, 29.3, 41.0]), bin=np.array([14, 20, 28]), level_db=np.array([-5.0, -3.25, -120.0]),
        phase_deg=np.array([10.0, -179.5, 90.0]), minimum_phase_deg=np.array([45.5, 12.25, -400.0]),
        excess_phase_deg=np.array([-35.5, -191.75, 490.0]), excess_group_delay_seconds=np.array([0.001, 0.0015, -0.00025]),
        minimum_group_delay_seconds=np.array([0.002, 0.0005, 0.0]), floored=np.array([False, False, True]))
    bare = MinPhaseChannelResult(
        channel_name="right", sample_rate_hz=44100, centre="onset", centre_samples=0, centre_seconds=0.0, segment_samples=0,
        fft_size=32, floor_db=-60.5, points_per_octave=1, floored_share=nan, excess_delay_seconds=nan,
        excess_phase_span_deg=nan)
    return [full, bare]


def test_summary_text_and_markdown_formats_are_pinned():
    from audio_analysis_amd.analyse.minphase import summarise_minphase_markdown, summarise_minphase_text
    assert summarise_minphase_text(_hand_built()) == (
        "[left]\n"
        "Centre: peak at 240 samples (5.000 ms)  Segment: 4800 samples, N = 32768  Floor: -120 dB  Points: 3 (2 per octave)\n"
        "freq_Hz  level_dB  phase_deg  min_phase_deg  excess_phase_deg  excess_gd_ms  min_gd_ms  floored\n"
        "20.5  -5.00  10.0  45.5  -35.5  1.000  2.000  no\n"
        "41.0  -120.00  90.0  -400.0  490.0  -0.250  0.000  yes\n"
        "excess delay: 1.250 ms, excess phase span: 181.2 deg, floored bins: 3.12 %\n"
        "\n"
        "[right]\n"
        "Centre: onset at 0 samples (0.000 ms)  Segment: 0 samples, N = 32  Floor: -60.5 dB  Points: NA (1 per octave)\n"
        "freq_Hz  level_dB  phase_deg  min_phase_deg  excess_phase_deg  excess_gd_ms  min_gd_ms  floored\n"
        "excess delay: NA ms, excess phase span: NA deg, floored bins: NA %\n"
        "\n")
    assert summarise_minphase_text([]) == ""
    md = summarise_minphase_markdown(_hand_built())
    assert md.startswith("### left\n\nCentre: peak at 240 samples (5.000 ms). Segment: 4800 samples, N = 32768. Floor: -120 dB. "
                         "Points: 3 (2 per octave).\n\n| freq (Hz) | level (dB) | phase (deg) | minimum phase (deg) | excess phase (deg) "
                         "| excess group delay (ms) | minimum group delay (ms) | floored |\n|---|---:|---:|---:|---:|---:|---:|---:|\n"
                         "| 20.5 | -5.00 | 10.0 | 45.5 | -35.5 | 1.000 | 2.000 | no |\n")
    assert "excess delay: NA ms, excess phase span: NA deg, floored bins: NA %.\n" in md


def test_json_round_trip_keeps_nan_and_drops_the_curve_on_request():
    from audio_analysis_amd.analyse.minphase import (minphase_results_from_json, minphase_results_to_json,
                                                     summarise_minphase_text)
    res = _hand_built()
    doc = json.loads(json.dumps(minphase_results_to_json(res), allow_nan=False))     # strict JSON: no NaN tokens
    rows = doc["minimum_phase"]
    scalars = {"channel_name", "sample_rate_hz", "centre", "centre_samples", "centre_seconds", "segment_samples", "fft_size",
               "floor_db", "points_per_octave", "floored_share", "excess_delay_seconds", "excess_phase_span_deg"}
    curves = {"frequencies_hz", "bin", "level_db", "phase_deg", "minimum_phase_deg", "excess_phase_deg",
              "excess_group_delay_seconds", "minimum_group_delay_seconds", "floored"}
    assert set(rows[0]) == scalars | curves and set(rows[1]) == scalars
    assert rows[0]["bin"] == [14, 20, 28] and rows[0]["floored"] == [False, False, True] and rows[0]["fft_size"] == 32768
    assert rows[1]["floored_share"] is None and rows[1]["excess_delay_seconds"] is None and rows[1]["excess_phase_span_deg"] is None
    back = minphase_results_from_json(doc)
    assert summarise_minphase_text(back) == summarise_minphase_text(res) and minphase_results_to_json(back) == doc
    assert back[0].floored.dtype == bool and back[0].bin.dtype == np.int64 and back[1].level_db is None
    assert np.array_equal(back[0].excess_phase_deg, res[0].excess_phase_deg) and math.isnan(back[1].excess_delay_seconds)
    slim = minphase_results_to_json(res, with_curve=False)
    assert all(set(r) == scalars for r in slim["minimum_phase"])
    assert minphase_results_from_json(json.loads(json.dumps(slim)))[0].level_db is None
    nan_curve = _hand_built()[0]
    object.__setattr__(nan_curve, "level_db", np.array([np.nan, 1.0, np.nan]))
    assert json.loads(json.dumps(minphase_results_to_json([nan_curve]), allow_nan=False))["minimum_phase"][0]["level_db"] == [None, 1.0, None]


def test_cli_parser_defaults_and_help_through_the_shim():
    import analyse.minphase as shim
    from audio_analysis_amd.analyse import minphase as D
    assert shim is D
    p = D.build_parser()
    a = p.parse_args(["--input", "a.wav", "b.wav"])
    assert a.input == [Path("a.wav"), Path("b.wav")] and a.bundle is None and a.mono is False and a.no_curve is False
    assert (a.expected_sample_rate, a.json, a.write_minimum_phase, a.post_ms) == (48000, None, None, None)
    assert D.settings_from_args(a) == D.MinPhaseSettings()
    a = p.parse_args(["--bundle", "d", "--mono", "--oversample", "8", "--post-ms", "12.5", "--floor-db", "-90",
                      "--points-per-octave", "12", "--f-min", "50", "--f-max", "10000", "--centre", "onset", "--onset-db", "-30",
                      "--no-curve", "--write-minimum-phase", "out", "--expected-sample-rate", "44100", "--json", "o.json"])
    assert D.settings_from_args(a) == D.MinPhaseSettings(
        oversample=8, post_ms=12.5, floor_db=-90.0, points_per_octave=12, f_min_hz=50.0, f_max_hz=10000.0, centre="onset",
        onset_db=-30.0, use_mono_downmix_for_stereo=True)
    assert a.bundle == Path("d") and a.no_curve and a.write_minimum_phase == Path("out") and a.json == Path("o.json")
    for bad in ([], ["--input", "a.wav", "--bundle", "d"], ["--input", "a.wav", "--centre", "middle"],
                ["--input", "a.wav", "--oversample", "2.5"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit):                                       # invalid settings end as a usage error
        D.main(["--input", "a.wav", "--oversample", "1"])
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.minphase", "--help"], capture_output=True, text=True, cwd=str(REPO),
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--input", "--bundle", "--mono", "--oversample", "--post-ms", "--floor-db", "--points-per-octave", "--f-min",
                 "--f-max", "--centre", "--onset-db", "--no-curve", "--write-minimum-phase", "--expected-sample-rate", "--json"):
        assert flag in r.stdout


# ------------------------------------------------------------------------------------------------ library and engine
NEW_SYMBOLS = ("ira_minphase_logmag", "ira_minphase_excess", "ira_minphase_gather", "ira_minphase_spectrum")


def test_header_constants_symbols_and_abi_version():
    from audio_analysis_amd import _lib, build, engine
    from audio_analysis_amd.analyse import deconvolve
    hdr = (REPO / "include" / "ira.h").read_text()
    assert re.search(rf"#define IRA_MINPHASE_FIELDS {engine.MINPHASE_FIELDS}\b", hdr) and engine.MINPHASE_FIELDS == 8
    assert re.search(rf"#define IRA_MINPHASE_MAX_LOG2 {engine.MINPHASE_MAX_LOG2}\b", hdr)
    assert engine.MINPHASE_MAX_LOG2 == deconvolve.MAX_LOG2_FFT == 21 and engine.MINPHASE_MIN_N == 32
    assert "#define IRA_MINPHASE_MIN_FLOOR_DB (-300.0)" in hdr and engine.MINPHASE_MIN_FLOOR_DB == -300.0
    assert build.SOURCES["ira_minphase.hip"] == ["-ffp-contract=off"]
    assert "#define IRA_ABI_VERSION 15 " in hdr and _lib.ABI_VERSION == 15
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES and re.search(rf"int32_t {name}\(", hdr)
    declared = set(re.findall(r"\b(ira_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_lib.PROTOTYPES)
    assert "replace no reference function" in hdr[hdr.index("Minimum phase, excess phase"):]
    lib = _lib.load()
    assert lib.ira_abi_version() == 15 and all(getattr(lib, name) is not None for name in NEW_SYMBOLS)


def test_entry_points_validate_arguments_without_gpu():
    from audio_analysis_amd import _lib
    lib = _lib.load()
    E_NULL, E_SIZE = -1, -2
    nan, inf = float("nan"), float("inf")

    def logmag(**kw):
        a = dict(spec=1, off=1, nfft=1, nb=0, max_nfft=256, floor_db=-120.0, g=1, pmax=1, floored=1)
        a.update(kw)
        return lib.ira_minphase_logmag(a["spec"], a["off"], a["nfft"], a["nb"], a["max_nfft"], a["floor_db"], a["g"], a["pmax"],
                                       a["floored"], 0)

    def excess(**kw):
        a = dict(spec=1, tspec=1, off=1, nfft=1, centre=1, pmax=1, nb=0, max_nfft=256, out=1)
        a.update(kw)
        return lib.ira_minphase_excess(a["spec"], a["tspec"], a["off"], a["nfft"], a["centre"], a["pmax"], a["nb"],
                                       a["max_nfft"], a["out"], 0)

    def gather(**kw):
        a = dict(spec=1, tspec=1, unwrapped=1, off=1, nfft=1, bins=1, pmax=1, nb=0, npts=479, out=1)
        a.update(kw)
        return lib.ira_minphase_gather(a["spec"], a["tspec"], a["unwrapped"], a["off"], a["nfft"], a["bins"], a["pmax"], a["nb"],
                                       a["npts"], a["out"], 0)

    def spectrum(**kw):
        a = dict(g=1, tspec=1, off=1, nfft=1, pmax=1, nb=0, max_nfft=256)
        a.update(kw)
        return lib.ira_minphase_spectrum(a["g"], a["tspec"], a["off"], a["nfft"], a["pmax"], a["nb"], a["max_nfft"], 0)

    pointers = {logmag: ("spec", "off", "nfft", "g", "pmax", "floored"),
                excess: ("spec", "tspec", "off", "nfft", "centre", "pmax", "out"),
                gather: ("spec", "tspec", "unwrapped", "off", "nfft", "bins", "pmax", "out"),
                spectrum: ("g", "tspec", "off", "nfft", "pmax")}
    for fn, names in pointers.items():
        assert fn() == 0                                                    # nb == 0: nothing to do
        for name in names:
            assert fn(**{name: 0}) == E_NULL and fn(nb=3, **{name: 0}) == E_NULL, (fn.__name__, name)
        for kw in (dict(nb=-1), dict(nb=65536)):
            assert fn(**kw) == E_SIZE, (fn.__name__, kw)
    for fn in (logmag, excess, spectrum):
        for size in (0, 16, 31, 33, 48, 1000, (1 << 21) + 1, 1 << 22, -256):
            assert fn(max_nfft=size) == E_SIZE and fn(nb=2, max_nfft=size) == E_SIZE, (fn.__name__, size)
        assert fn(max_nfft=32) == 0 and fn(max_nfft=1 << 21) == 0
    for floor in (0.5, -300.5, nan, inf, -inf):
        assert logmag(floor_db=floor) == E_SIZE and logmag(nb=2, floor_db=floor) == E_SIZE, floor
    assert logmag(floor_db=0.0) == 0 and logmag(floor_db=-300.0) == 0
    for npts in (-1, 4097):
        assert gather(npts=npts) == E_SIZE and gather(nb=2, npts=npts) == E_SIZE
    assert gather(npts=0) == 0 and gather(npts=4096) == 0 and gather(nb=0, npts=0) == 0


def _names(eng):
    return [c[0] for c in eng.calls()]


def test_minphase_device_calls_on_the_recording_engine(monkeypatch):
    """Order, arguments and allocation sizes of the library calls: two forward transforms, one inverse, the new calls and
    ira_phase_unwrap; then the sub-batch cut and the minimum-phase response."""
    from host_engine import HostEngine
    from audio_analysis_amd import engine
    from audio_analysis_amd.analyse import minphase as D
    eng = HostEngine()
    rng = np.random.default_rng(5)
    lens = [64, 60, 64, 33, 50]                                             # oversample 4: N = 256 for every channel
    batch = eng.upload([rng.standard_normal(n).astype(np.float32) for n in lens])
    res = D.minphase_device(eng, batch, FS, D.MinPhaseSettings())
    assert _names(eng) == ["ira_peak_index", "ira_onset_index", "ira_rfft_smooth", "ira_minphase_logmag", "ira_band_irfft_smooth",
                           "ira_rfft_smooth", "ira_minphase_excess", "ira_phase_unwrap", "ira_minphase_gather"]
    nbins, npts = 129, 479
    spec_off = np.arange(5) * nbins
    fwd1, fwd2 = eng.calls("ira_rfft_smooth")
    (x, xo, size, count, hann, _t1, _t2, _tf, _work, spec, so, *_rest) = fwd1[1]
    assert (size, count, hann) == (128, 5, 0) and x[0] == "up" and spec[:3] == ("empty", 5 * nbins * 2, "torch.float64")
    assert list(eng.table(xo)[:5]) == list(batch.off) and list(eng.table(so)[:5]) == list(spec_off)
    assert list(eng.table(fwd1[1][15])[:5]) == lens and list(eng.table(fwd1[1][16])[:5]) == [256] * 5     # data_len D, win_len N
    (spec_a, so_a, nf_a, nb, max_nfft, floor_db, g, pmax, floored, stream) = eng.calls("ira_minphase_logmag")[0][1]
    assert (nb, max_nfft, floor_db, stream) == (5, 256, -120.0, None) and spec_a == spec
    assert list(eng.table(so_a)[:5]) == list(spec_off) and list(eng.table(nf_a)[:5]) == [256] * 5 and nf_a[1] == "<i4"
    assert g[:3] == ("empty", 5 * nbins * 2, "torch.float64") and pmax[:3] == ("empty", 5, "torch.float64")
    assert floored[:3] == ("empty", 5, "torch.int64")
    inv = eng.calls("ira_band_irfft_smooth")[0][1]
    assert inv[0] == g and inv[2:4] == (128, 5) and inv[14] == 1                                           # half-length inverses of G
    c = inv[10]
    assert c[:3] == ("empty", 5 * 256, "torch.float32") and list(eng.table(inv[11])[:5]) == [0, 256, 512, 768, 1024]
    assert list(eng.table(inv[4])[:8]) == [2.0, -1.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0]                       # the all-pass record
    (x2, xo2, size2, count2, hann2, *_r, ) = fwd2[1][:5] + ((),)
    assert x2 == c and (size2, count2, hann2) == (128, 5, 0) and list(eng.table(xo2)[:5]) == [0, 256, 512, 768, 1024]
    assert list(eng.table(fwd2[1][15])[:5]) == [128] * 5 and list(eng.table(fwd2[1][16])[:5]) == [256] * 5  # c[0 : N/2], n = N
    tspec = fwd2[1][9]
    assert tspec[:3] == ("empty", 5 * nbins * 2, "torch.float64")
    (spec_b, tspec_b, so_b, nf_b, centre, pmax_b, nb, max_nfft, ex, stream) = eng.calls("ira_minphase_excess")[0][1]
    assert (spec_b, tspec_b, pmax_b, nb, max_nfft) == (spec, tspec, pmax, 5, 256) and ex[:3] == ("empty", 5 * nbins, "torch.float64")
    assert list(eng.table(centre)[:5]) == [0] * 5 and centre[1] == "<i8"     # the recording engine's onset call answers zeros
    (ph, po, pl, nb, do_unwrap, degrees, out32, oo, out64, stream) = eng.calls("ira_phase_unwrap")[0][1]
    assert ph == ex and (nb, do_unwrap, degrees, out32) == (5, 1, 0, None) and out64[:3] == ("empty", 5 * nbins, "torch.float64")
    assert list(eng.table(po)[:5]) == list(spec_off) and list(eng.table(pl)[:5]) == [256] * 5
    (spec_c, tspec_c, un, so_c, nf_c, bins, pmax_c, nb, npts_c, out, stream) = eng.calls("ira_minphase_gather")[0][1]
    assert (spec_c, tspec_c, un, pmax_c, nb, npts_c) == (spec, tspec, out64, pmax, 5, npts)
    assert out[:3] == ("empty", 5 * npts * 8, "torch.float64") and bins[1] == "<i4"
    assert np.array_equal(eng.table(bins)[: 5 * npts].reshape(5, npts), np.broadcast_to(R.grid_bins(256, float(FS)), (5, npts)))
    assert res.records.shape == (5, npts, 8) and list(res.segment) == lens and list(res.n_fft) == [256] * 5
    assert list(res.length) == lens and res.bins.shape == (5, npts) and res.pmax.shape == (5,) and res.floored.dtype == np.int64
    # the budget cuts the batch into sub-batches of whole channels: 2, 2, 1
    monkeypatch.setattr(engine, "MINPHASE_SCRATCH_BYTES", 2 * (44 * 256 + 64))
    first = len(eng.calls())
    D.minphase_device(eng, batch, FS, D.MinPhaseSettings(centre="onset"), centre_samples=[1, 2, 3, 4, 5])
    later = [c for c in eng.calls()[first:]]
    assert [c[0] for c in later] == ["ira_rfft_smooth", "ira_minphase_logmag", "ira_band_irfft_smooth", "ira_rfft_smooth",
                                     "ira_minphase_excess", "ira_phase_unwrap", "ira_minphase_gather"] * 3   # no onset call
    assert [c[1][3] for c in later if c[0] == "ira_minphase_logmag"] == [2, 2, 1]
    assert [list(eng.table(c[1][4])[: c[1][6]]) for c in later if c[0] == "ira_minphase_excess"] == [[1, 2], [3, 4], [5]]
    assert [c[1][9][1] for c in later if c[0] == "ira_minphase_gather"] == [2 * npts * 8, 2 * npts * 8, npts * 8]
    monkeypatch.setattr(engine, "MINPHASE_SCRATCH_BYTES", 4 << 30)
    # mixed sizes, an empty channel and post_ms: the empty channel is not transformed
    first = len(eng.calls())
    mixed = eng.upload([rng.standard_normal(n).astype(np.float32) for n in (100, 0, 5, 700)])
    res = D.minphase_device(eng, mixed, FS, D.MinPhaseSettings(post_ms=2.5), centre_samples=[10, 0, 4, 100])
    assert list(res.segment) == [100, 0, 5, 221] and list(res.n_fft) == [512, 32, 32, 1024]
    logmag = [c for c in eng.calls()[first:] if c[0] == "ira_minphase_logmag"]
    assert len(logmag) == 1 and logmag[0][1][3:5] == (3, 1024) and list(eng.table(logmag[0][1][2])[:3]) == [512, 32, 1024]
    assert np.isnan(res.records[1]).all() and res.pmax[1] == 0.0 and "ira_onset_index" not in [c[0] for c in eng.calls()[first:]]
    # an empty batch launches nothing but the calls for the centre
    first = len(eng.calls())
    res = D.minphase_device(eng, eng.upload([]), FS)
    assert [c[0] for c in eng.calls()[first:]] == ["ira_peak_index", "ira_onset_index"] and res.records.shape == (0, npts, 8)
    # the response: the same chain, then M in place of G and a second inverse into the output
    first = len(eng.calls())
    dev = D.minimum_phase_device(eng, batch, FS, D.MinPhaseSettings())
    later = eng.calls()[first:]
    assert [c[0] for c in later] == ["ira_peak_index", "ira_onset_index", "ira_rfft_smooth", "ira_minphase_logmag",
                                     "ira_band_irfft_smooth", "ira_rfft_smooth", "ira_minphase_spectrum", "ira_band_irfft_smooth"]
    (g2, tspec2, so2, nf2, pmax2, nb, max_nfft, stream) = later[6][1]
    assert g2 == later[3][1][6] and tspec2 == later[5][1][9] and pmax2 == later[3][1][7] and (nb, max_nfft) == (5, 256)
    assert later[7][1][0] == g2 and later[7][1][10][:3] == ("empty", 5 * 256, "torch.float32")
    assert list(dev["off"]) == [0, 256, 512, 768, 1024] and list(dev["n_out"]) == lens and list(dev["n_fft"]) == [256] * 5
    with pytest.raises(ValueError, match="centre_samples"):
        D.minphase_device(eng, batch, FS, centre_samples=[0, 0, 0, 33, 0])
    with pytest.raises(ValueError, match="lower oversample or set post_ms"):
        D.minphase_device(eng, eng.upload([np.zeros((1 << 19) + 1, np.float32)]), FS)


def test_engine_methods_refuse_bad_arguments():
    from host_engine import HostEngine
    eng = HostEngine()
    buf = eng.empty(4096, eng.torch.float64)
    off, nf = np.array([0, 17]), np.array([32, 64])
    for bad, what in ((dict(n_fft=[32]), "spec_off and n_fft"), (dict(n_fft=[32, 48]), "powers of two"),
                      (dict(n_fft=[16, 64]), "powers of two"), (dict(n_fft=[32, 1 << 22]), "powers of two"),
                      (dict(floor_db=1.0), "floor_db"), (dict(floor_db=-400.0), "floor_db")):
        kw = dict(spec_off=off, n_fft=nf, floor_db=-120.0)
        kw.update(bad)
        with pytest.raises(ValueError, match=what):
            eng.minphase_logmag(buf, **kw)
    pmax = eng.empty(2, eng.torch.float64)
    with pytest.raises(ValueError, match="centre"):
        eng.minphase_excess(buf, buf, off, nf, [0, -1], pmax)
    with pytest.raises(ValueError, match="centre"):
        eng.minphase_excess(buf, buf, off, nf, [0], pmax)
    for bins, what in ((np.ones((3, 4)), r"\(n, J\)"), (np.ones(4), r"\(n, J\)"), (np.array([[1, 15], [1, 32]]), "whole numbers"),
                       (np.array([[0, 15], [1, 31]]), "whole numbers"), (np.array([[1, 16], [1, 31]]), "whole numbers"),
                       (np.array([[1.5, 15], [1, 31]]), "whole numbers"), (np.ones((2, 4097)), "at most 4096")):
        with pytest.raises(ValueError, match=what):
            eng.minphase_gather(buf, buf, buf, off, nf, bins, pmax)
    assert eng.minphase_gather(buf, buf, buf, off, nf, np.array([[1, 15], [1, 31]]), pmax).shape == (2, 2, 8)
    assert eng.minphase_gather(buf, buf, buf, off, nf, np.zeros((2, 0)), pmax).shape == (2, 0, 8)
    before = len(eng.calls())
    g, p, f = eng.minphase_logmag(buf, [], [], -120.0)
    eng.minphase_spectrum(buf, buf, [], [], pmax)
    assert len(eng.calls()) == before and p.shape == (0,) and f.shape == (0,)


# ------------------------------------------------------------------------------------------------ the restatement
def _padded(x, length=128):
    out = np.zeros(length, dtype=np.float32)
    out[: len(x)] = x
    return out


def test_the_analytic_inputs_are_what_they_claim():
    a = R.min_phase_fir()
    assert a.dtype == np.float32 and a[0] == 1.0 and np.all(np.abs(a[1:]) < 1.0) and int(np.argmax(np.abs(a))) == 0
    assert np.array_equal(a.astype(np.float64) * 2.0 ** R.TAP_BITS, np.rint(a.astype(np.float64) * 2.0 ** R.TAP_BITS))
    assert np.max(np.abs(R.fir_zeros())) <= R.RADIUS and R.fir_zeros().size == 5
    for length in (64, 100):
        c = R.fir_through_allpass(length)
        exact = np.convolve(a.astype(np.float64), R.allpass_ir(length))[:length]
        assert np.array_equal(c.astype(np.float64), exact)                 # every sample exact in float32
    assert R.aliasing(256) < 1.2e-6 and R.aliasing(512) < 1e-12
    # the all-pass has unit magnitude and goes from 0 to -pi
    ph = R.allpass_phase(512)
    assert ph[0] == 0.0 and abs(abs(ph[-1]) - np.pi) < 1e-12 and np.all(np.diff(ph[:-1]) < 0)


@pytest.mark.parametrize("length", [64, 128])
def test_restatement_meets_the_analytic_cases(length):
    """(a) .. (e) on the float64 restatement: N = 256 and 512.  No bin is floored in any of them."""
    a = R.min_phase_fir()
    z = a.size - 1
    n = 4 * length
    k = np.arange(n // 2 + 1)
    phi = R.fir_phase(n)
    alias = R.aliasing(n)
    worst = {}

    def bound(ref, against=None):
        b = R.Bounds(ref)
        assert not ref["floored"].any() and ref["valid"]
        return b, alias + b.phi_min(against_device=False, analytic=True), b.phi_rel(k, 1)

    # (a) minimum phase: phi_min is the closed form, the excess phase 0
    ref = R.chain(_padded(a, length), 0, length, n)
    b, bm, br = bound(ref)
    worst["a"] = max(np.max(np.abs(ref["phi_min"] - phi) / bm), np.max(np.abs(ref["excess"]) / (bm + br)))
    # (b) delayed by d, centre = the peak
    for d in (1, 17, length - z - 1):
        x = np.zeros(length, dtype=np.float32)
        x[d : d + a.size] = a
        assert int(np.argmax(np.abs(x))) == d
        ref = R.chain(x, d, length, n)
        b, bm, br = bound(ref)
        worst["b"] = max(worst.get("b", 0.0), np.max(np.abs(ref["excess"]) / (bm + br)))
    # (c) through the all-pass, centre pinned to sample 0
    x = R.fir_through_allpass(length)
    ref = R.chain(x, 0, length, n)
    b, bm, br = bound(ref)
    trunc = 4.0 * float(np.sum(np.abs(a))) * R.ALLPASS_A ** (length - 1) / float(np.min(b.mag))
    worst["c"] = np.max(np.abs(R.wrap(ref["wrapped"] - R.allpass_phase(n))) / (bm + br + trunc))
    bins = R.grid_bins(n, float(FS), f_min=1.0, f_max=FS / 2.0)
    assert bins[0] == 1 and bins[-1] >= n // 2 - 2
    span = np.degrees(np.max(ref["excess"][bins]) - np.min(ref["excess"][bins]))
    short = 180.0 - np.degrees(R.allpass_phase(n)[bins[0]] - R.allpass_phase(n)[bins[-1]])   # what the end bins leave out
    assert 0.0 < short < 6.0 and abs(span - (180.0 - short)) <= np.degrees(2.0 * np.max(bm + br + trunc))
    # (d) the time reversal, maximum phase: relative to its peak (the last tap) the phase is -phi_min, the excess -2 phi_min
    x = _padded(a[::-1].copy(), length)
    assert int(np.argmax(np.abs(x))) == z
    ref = R.chain(x, z, length, n)
    b, bm, br = bound(ref)
    worst["d"] = np.max(np.abs(R.wrap(ref["wrapped"] + 2.0 * phi)) / (bm + br))
    # and against sample 0 the linear phase of the reversal is there as well
    ref0 = R.chain(x, 0, length, n)
    worst["d0"] = np.max(np.abs(R.wrap(ref0["wrapped"] + 2.0 * phi + 2.0 * np.pi * k * z / n)) / (bm + br))
    # (e) the response: (a) from (a) and from (d), with the input's energy
    for x, ref in ((_padded(a, length), R.chain(_padded(a, length), 0, length, n)), (x, ref)):
        h = R.minimum_phase_ir(ref)
        each = bm * float(np.sum(np.abs(a)))                                # the phase bound times ||x||_1
        worst["e"] = max(worst.get("e", 0.0), np.max(np.abs(h - _padded(a, length)) / each))
        energy, want = float(np.sum(h * h)), float(np.sum(a.astype(np.float64) ** 2))
        norm = math.sqrt(want)
        assert abs(energy - want) <= 2.0 * norm * math.sqrt(length) * each + length * each * each
    print(f"N = {n}: worst error / bound " + ", ".join(f"({q}) {v:.3g}" for q, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_float32_cepstrum_stays_inside_its_bound():
    """Rounding c to float32 moves phi_min by at most 2^-23 sum |c[n]|: a NumPy emulation of that one step."""
    rng = np.random.default_rng(31)
    worst = 0.0
    for d, over in ((64, 4), (100, 2), (257, 16), (4097, 4)):
        x = (rng.standard_normal(d) * np.exp(-np.arange(d) / (d / 6.0))).astype(np.float32)
        x[3] = 5.0
        _, n = R.sizes(d, 3, FS, over)
        ref = R.chain(x, 3, d, n)
        c32 = ref["c"].astype(np.float32).astype(np.float64)
        moved = np.abs(2.0 * np.fft.rfft(c32[: n // 2], n=n).imag - ref["phi_min"])
        worst = max(worst, float(np.max(moved)) / (2.0 ** -23 * ref["sum_abs_c"]))
        assert R.Bounds(ref).first >= 2.0 ** -23 * ref["sum_abs_c"]
    print(f"float32 cepstrum: worst movement of phi_min / (2^-23 sum |c|) = {worst:.3f}")
    assert worst <= 1.0


def test_comb_floor_flags_of_the_restatement_stay_within_the_cap():
    """x = [1, 0, .., 1] with floor_db = -60: |X|^2 = 4 cos^2 crosses the floor at every notch.  The bins whose |X|^2 lies
    within the transform's error of P_floor (where a flag may differ between two float64 transforms) are at most 1 %."""
    for d, over in ((64, 4), (257, 4), (100, 16)):
        x = np.zeros(d, dtype=np.float32)
        x[0] = x[-1] = 1.0
        _, n = R.sizes(d, 0, FS, over)
        ref = R.chain(x, 0, d, n, floor_db=-60.0)
        assert ref["P"] == 4.0 and 0 < ref["floored"].sum() < ref["floored"].size
        exact = 4.0 * np.cos(np.pi * np.arange(n // 2 + 1) * (d - 1) / n) ** 2
        b = R.Bounds(ref)
        near = np.abs(ref["power"] - ref["P_floor"]) <= 2.0 * (2.0 * np.sqrt(ref["power"]) * b.e_x + b.e_x ** 2) + 2.0 * b.e_x * 4.0e-6
        assert np.array_equal(ref["floored"][~near], (exact < ref["P_floor"])[~near])
        assert np.count_nonzero(near) <= 0.01 * near.size, (d, n, np.count_nonzero(near))
