"""
CPU-only tests of the multi-slope decay fits (audio_analysis_amd.analyse.multislope): settings validation, the level-0 grid
and the refinement grids, the host arithmetic of step 6 and 7, the fixed text / Markdown / JSON formats on hand-built
results, the command line's parser, the call sequence of multislope_device on the recording engine, the argument checks of
the new C entry points (they return before touching a device), and the restatement of tests/multislope_ref.py itself: on
exact model curves, and the margin conditions the GPU tests' inputs must meet, which are conditions on the restatement
alone.
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

import multislope_ref as R

REPO = Path(__file__).resolve().parent.parent


def test_settings_defaults_and_validation():
    from audio_analysis_amd.analyse.multislope import MultiSlopeSettings
    from audio_analysis_amd.analyse.rt60bands import Rt60BandsAnalysisSettings
    s = MultiSlopeSettings()
    assert (s.max_order, s.t_min, s.t_max, s.grid, s.refine_levels, s.min_ratio, s.fit_fraction, s.accept_rms_db) == \
        (3, 0.05, 20.0, 64, 3, 1.5, 0.9, 0.15)
    assert s.bands.band_mode == "octave" and not s.use_mono_downmix_for_stereo and MultiSlopeSettings(bands=None).bands is None
    for bad, what in [(dict(max_order=0), "max_order"), (dict(max_order=4), "max_order"), (dict(max_order=2.0), "max_order"),
                      (dict(grid=0), "grid"), (dict(grid=129), "grid"), (dict(t_min=0.0), "t_min"),
                      (dict(t_min=2.0, t_max=1.0), "t_min"), (dict(t_min=1.0, t_max=1.0), "t_min"),
                      (dict(t_max=float("inf")), "t_min"), (dict(refine_levels=-1), "refine_levels"),
                      (dict(min_ratio=1.0), "min_ratio"), (dict(min_ratio=float("nan")), "min_ratio"),
                      (dict(fit_fraction=0.0), "fit_fraction"), (dict(fit_fraction=1.01), "fit_fraction"),
                      (dict(fit_fraction=float("nan")), "fit_fraction"), (dict(accept_rms_db=-0.1), "accept_rms_db"),
                      (dict(bands=Rt60BandsAnalysisSettings(band_mode="sixth")), "band_mode"), (dict(bands="octave"), "bands")]:
        with pytest.raises(ValueError, match=what):
            MultiSlopeSettings(**bad)
    assert MultiSlopeSettings(grid=1, t_min=0.5, t_max=0.5, fit_fraction=1.0, refine_levels=0, max_order=1).grid == 1


def test_level0_grid_and_refinement_grids():
    from audio_analysis_amd.analyse import multislope as MS
    s = MS.MultiSlopeSettings()
    grid, h0 = MS.level0_grid(s)
    assert grid.size == 64 and grid[0] == 0.05 and abs(grid[-1] - 20.0) < 1e-14 and np.all(np.diff(grid) > 0)
    assert abs(h0 - math.log(400.0) / 63.0) < 1e-16 and np.allclose(np.diff(np.log(grid)), h0, rtol=0, atol=1e-13)
    ref, rh = R.level0()
    assert np.all(np.abs(grid - ref) <= 8 * np.spacing(ref)) and abs(rh - h0) < 1e-16           # float64 pow: a few ulp
    steps = MS.refine_steps(s)
    assert steps == [h0 / 4, h0 / 16, h0 / 64] and abs(steps[-1] - 0.0015) < 2e-5            # 0.15 % of T
    assert MS.refine_steps(MS.MultiSlopeSettings(refine_levels=0)) == []
    one = MS.refined_grid([0.4], steps[0])
    assert one.size == 7 and one[3] == 0.4 and np.allclose(np.diff(np.log(one)), steps[0])
    three = MS.refined_grid([0.4, 1.5, 6.0], steps[1])
    assert three.size == 21 and np.all(np.diff(three) > 0) and {0.4, 1.5, 6.0} <= set(three.tolist())
    assert np.all(np.abs(three - R.refined([0.4, 1.5, 6.0], steps[1])) <= 2 * np.spacing(three))
    # overlapping clusters merge in ascending order, equal values once
    both = MS.refined_grid([1.0, 1.0 * math.exp(2 * 0.1)], 0.1)
    assert np.all(np.diff(both) > 0) and both.size <= 14 and 1.0 in both.tolist()
    assert MS.level0_grid(MS.MultiSlopeSettings(grid=1, t_min=0.5, t_max=0.5))[0].tolist() == [0.5]


def _record(order, ts, a, a_nu, c=0.5, j=2000.0, d0=4.0):
    rec = np.full(16, np.nan)
    rec[0], rec[1], rec[2], rec[3], rec[14], rec[15] = 0.0, j, 1.0 if a_nu > 0 else 0.0, c, d0, 64.0
    rec[4:7] = -1.0
    for s in range(order):
        rec[4 + s], rec[7 + s], rec[10 + s] = 10.0 * s, ts[s], a[s]
    rec[13] = a_nu
    return rec


def test_host_arithmetic_of_step_6_and_7():
    from audio_analysis_amd.analyse import multislope as MS
    fs, L = 48000, 144000
    f = MS.fit_from_record(_record(2, (0.4, 1.5), (3.0, 0.25), 1e-5), 2, fs, L)
    lam = [math.log(1e6) / (t * fs) for t in (0.4, 1.5)]
    assert f.order == 2 and f.decay_times_seconds == (0.4, 1.5) and f.coefficients == (3.0, 0.25) and f.noise_coefficient == 1e-5
    assert abs(f.rms_db - (10 / math.log(10)) * math.sqrt(0.5 / 2000.0)) < 1e-15
    assert abs(f.start_levels_db[0] - 10 * math.log10(3.0 * (1 - math.exp(-lam[0] * L)) / 4.0)) < 1e-12
    assert abs(f.noise_share_db - 10 * math.log10(1e-5 / 4.0)) < 1e-12
    tx = math.log(3.0 / 0.25) / (lam[0] - lam[1])
    assert abs(f.turning_points_seconds[0] - tx / fs) < 1e-12 and 0.05 < tx / fs < 0.15
    assert abs(f.turning_levels_db[0] - 10 * math.log10(3.0 * math.exp(-lam[0] * tx) / 4.0)) < 1e-12
    want = R.finish(dict(idx=(0, 1), T=(0.4, 1.5), a=np.array([3.0, 0.25], R.LD), a_nu=R.LD(1e-5), c=R.LD(0.5)),
                    dict(L=L, J=2000, d=np.array([4.0], R.LD)), fs)
    assert abs(f.rms_db - want["rms_db"]) < 1e-14 and abs(f.turning_points_seconds[0] - want["turn_s"][0]) < 1e-12
    assert abs(f.start_levels_db[1] - want["start_db"][1]) < 1e-12 and abs(f.turning_levels_db[0] - want["turn_db"][0]) < 1e-12
    # the later slope starts above the earlier one: no turning point; no noise term: -inf
    g = MS.fit_from_record(_record(2, (0.4, 1.5), (0.2, 0.25), 0.0), 2, fs, L)
    assert math.isnan(g.turning_points_seconds[0]) and math.isnan(g.turning_levels_db[0]) and g.noise_share_db == -math.inf
    assert MS.fit_from_record(_record(1, (0.6,), (1.0,), 0.0), 1, fs, L).turning_points_seconds == ()
    none = np.full(16, np.nan)
    none[0] = 32.0
    assert MS.fit_from_record(none, 2, fs, L) is None
    # preferred order: the smallest whose rms_db is accepted, else the largest fitted
    mk = lambda o, rms: MS.MultiSlopeFit(o, (1.0,) * o, (1.0,) * o, 0.0, 1.0, rms, (0.0,) * o, -math.inf, (), ())   # noqa: E731
    assert MS.preferred_order({1: mk(1, 0.46), 2: mk(2, 0.04), 3: mk(3, 0.03)}, 0.15) == 2
    assert MS.preferred_order({1: mk(1, 0.15), 2: mk(2, 0.04)}, 0.15) == 1
    assert MS.preferred_order({1: mk(1, 0.5), 2: mk(2, 0.4)}, 0.15) == 2 and MS.preferred_order({}, 0.15) == 0
    assert MS.preferred_order({1: mk(1, 0.5), 3: mk(3, 0.1)}, 0.15) == 3 == R.preferred({1: 0.5, 3: 0.1})
    # rows: an error status ends the row; an order without a candidate sets its bit and the others stand
    recs = np.stack([_record(1, (0.6,), (1.0,), 1e-6, c=2000 * (0.46 * math.log(10) / 10) ** 2), none,
                     _record(3, (0.2, 0.6, 2.0), (1.0, 0.5, 0.1), 0.0, c=0.001)])
    v = MS.values_from_records(recs, fs, L, MS.MultiSlopeSettings())
    assert v.status == 64 and sorted(v.fits_by_order) == [1, 3] and v.preferred_order == 3
    assert MS.status_text(v.status) == "64 (no order-2 candidate)" and MS.status_text(0) == "ok"
    assert MS.values_from_records(recs, fs, L, MS.MultiSlopeSettings(max_order=1)).preferred_order == 1
    for st in (1, 2, 4, 16):
        bad = np.full((3, 16), np.nan)
        bad[:, 0] = st
        v = MS.values_from_records(bad, fs, L, MS.MultiSlopeSettings())
        assert v.status == st and v.fits_by_order == {} and v.preferred_order == 0
    assert (MS.STATUS_SILENT, MS.STATUS_TOO_SHORT, MS.STATUS_ZERO_IN_RANGE, MS.STATUS_NON_FINITE) == \
        (R.S_SILENT, R.S_SHORT, R.S_ZERO, R.S_NON_FINITE)
    assert MS.status_text(4) == "4 (silence in fit range)" and MS.status_text(2 | 16) == "18 (too short, non-finite)"


def _hand_built():
    from audio_analysis_amd.analyse.multislope import MultiSlopeChannelResult, MultiSlopeFit, MultiSlopeValues
    from audio_analysis_amd.analyse.rt60bands import BandDefinition
    nan = float("nan")
    bands = [BandDefinition("500Hz", 500.0, "band", 353.55, 707.11), BandDefinition("1000Hz", 1000.0, "band", 707.11, 1414.21)]
    f1 = MultiSlopeFit(1, (1.4585,), (0.9,), 2.5e-6, 29.83, 0.4565, (-0.46,), -55.23, (), ())
    f2 = MultiSlopeFit(2, (0.4058, 1.5025), (0.95, 0.061), 2.1e-6, 0.2233, 0.0395, (-0.22, -12.147), -56.0, (0.23456,), (-13.861,))
    f3 = MultiSlopeFit(3, (0.2, 0.6, 2.0), (1.0, 0.5, 0.1), 0.0, 0.1, 0.0306, (-1.0, -4.0, -11.0), -math.inf, (0.1, nan),
                       (-7.5, nan))
    a = MultiSlopeChannelResult("hall.wav:left", 48000, 240, MultiSlopeValues(0, {1: f1, 2: f2}, 2), bands,
                                {"500Hz": MultiSlopeValues(64, {1: f1, 3: f3}, 3), "1000Hz": MultiSlopeValues(2, {}, 0)})
    b = MultiSlopeChannelResult("mono.wav:mono", 44100, 0, MultiSlopeValues(0, {1: f1}, 1), [], {})
    return [a, b]


def test_summary_text_format_is_pinned():
    from audio_analysis_amd.analyse.multislope import summarise_multislope_text
    assert summarise_multislope_text(_hand_built()) == (
        "[hall.wav:left]\n"
        "Start: 240 samples (5.000 ms)\n"
        "Band  Order  Pref  RMS_dB  T_s  Start_dB  Noise_dB  Turn_ms  Turn_dB  Status\n"
        "Broadband  1  -  0.457  1.458  -0.46  -55.23  -  -  ok\n"
        "Broadband  2  *  0.040  0.406/1.502  -0.22/-12.15  -56.00  234.6  -13.86  ok\n"
        "500Hz  1  -  0.457  1.458  -0.46  -55.23  -  -  64 (no order-2 candidate)\n"
        "500Hz  3  *  0.031  0.200/0.600/2.000  -1.00/-4.00/-11.00  -inf  100.0/NA  -7.50/NA  64 (no order-2 candidate)\n"
        "1000Hz  NA  -  NA  NA  NA  NA  NA  NA  2 (too short)\n"
        "\n"
        "[mono.wav:mono]\n"
        "Start: 0 samples (0.000 ms)\n"
        "Band  Order  Pref  RMS_dB  T_s  Start_dB  Noise_dB  Turn_ms  Turn_dB  Status\n"
        "Broadband  1  *  0.457  1.458  -0.46  -55.23  -  -  ok\n"
        "\n")
    assert summarise_multislope_text([]) == ""


def test_summary_markdown_format_is_pinned():
    from audio_analysis_amd.analyse.multislope import summarise_multislope_markdown
    assert summarise_multislope_markdown(_hand_built()[1:]) == (
        "### mono.wav:mono\n"
        "\n"
        "Start: 0 samples (0.000 ms).\n"
        "\n"
        "| Band | Order | Preferred | RMS (dB) | T (s) | Start (dB) | Noise (dB) | Turning point (ms) | Level there (dB) | Status |\n"
        "|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|\n"
        "| Broadband | 1 | * | 0.457 | 1.458 | -0.46 | -55.23 | - | - | ok |\n"
        "\n")
    md = summarise_multislope_markdown(_hand_built())
    assert "| 1000Hz | NA | - | NA | NA | NA | NA | NA | NA | 2 (too short) |\n" in md
    assert "| 500Hz | 3 | * | 0.031 | 0.200/0.600/2.000 | -1.00/-4.00/-11.00 | -inf | 100.0/NA | -7.50/NA | 64 (no order-2 candidate) |\n" in md


def test_json_round_trip_keeps_nan_and_minus_infinity():
    from audio_analysis_amd.analyse.multislope import (multislope_results_from_json, multislope_results_to_json,
                                                       summarise_multislope_text)
    res = _hand_built()
    doc = json.loads(json.dumps(multislope_results_to_json(res), allow_nan=False))       # strict JSON: no NaN / Infinity tokens
    rows = doc["multislope"]
    assert rows[0]["broadband"]["preferred_order"] == 2 and [f["order"] for f in rows[0]["broadband"]["fits"]] == [1, 2]
    f3 = rows[0]["bands"][0]["fits"][1]
    assert f3["noise_share_db"] == "-inf" and f3["turning_points_seconds"] == [0.1, None] and f3["noise_coefficient"] == 0.0
    assert rows[0]["bands"][1]["status"] == 2 and rows[0]["bands"][1]["fits"] == [] and rows[0]["bands"][0]["name"] == "500Hz"
    back = multislope_results_from_json(doc)
    assert summarise_multislope_text(back) == summarise_multislope_text(res)
    assert back[0].broadband == res[0].broadband and back[0].band_definitions == res[0].band_definitions
    assert back[0].band_values_by_name["1000Hz"] == res[0].band_values_by_name["1000Hz"] and back[1] == res[1]
    got = back[0].band_values_by_name["500Hz"].fits_by_order[3]
    assert got.noise_share_db == -math.inf and math.isnan(got.turning_points_seconds[1]) and got.decay_times_seconds == (0.2, 0.6, 2.0)


def test_cli_parser_defaults_and_help():
    from audio_analysis_amd.analyse import multislope as MS
    p = MS.build_parser()
    a = p.parse_args(["--input", "a.wav", "b.wav"])
    assert a.input == [Path("a.wav"), Path("b.wav")] and a.bundle is None
    assert MS.settings_from_args(a) == MS.MultiSlopeSettings()
    a = p.parse_args(["--bundle", "d", "--bands", "none", "--mono", "--max-order", "2", "--t-min", "0.1", "--t-max", "10", "--grid",
                      "32", "--refine-levels", "2", "--min-ratio", "1.3", "--fit-fraction", "0.8", "--accept-rms-db", "0.2",
                      "--expected-sample-rate", "44100", "--json", "o.json"])
    assert a.bundle == Path("d") and a.expected_sample_rate == 44100 and a.json == Path("o.json")
    assert MS.settings_from_args(a) == MS.MultiSlopeSettings(max_order=2, t_min=0.1, t_max=10.0, grid=32, refine_levels=2,
                                                             min_ratio=1.3, fit_fraction=0.8, accept_rms_db=0.2, bands=None,
                                                             use_mono_downmix_for_stereo=True)
    for bad in ([], ["--input", "a.wav", "--bundle", "d"], ["--input", "a.wav", "--bands", "sixth"],
                ["--input", "a.wav", "--grid", "many"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(ValueError, match="grid"):
        MS.settings_from_args(p.parse_args(["--input", "a.wav", "--grid", "200"]))
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.multislope", "--help"], capture_output=True, text=True, cwd=str(REPO),
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--input", "--bundle", "--mono", "--bands", "--max-order", "--t-min", "--t-max", "--grid", "--refine-levels",
                 "--min-ratio", "--fit-fraction", "--accept-rms-db", "--expected-sample-rate", "--json"):
        assert flag in r.stdout
    r = subprocess.run([sys.executable, "-m", "analyse.multislope", "--input", "a.wav", "--min-ratio", "1.0"], capture_output=True,
                       text=True, cwd=str(REPO), env=env, timeout=120)
    assert r.returncode == 2 and "min_ratio" in r.stderr                              # a usage error, before any file is read


def test_shim_re_exports_the_module():
    import analyse.multislope as shim
    from audio_analysis_amd.analyse import multislope
    assert shim is multislope


def test_channel_length_limit_is_an_argument_error_before_any_launch():
    from host_engine import HostEngine
    from audio_analysis_amd.analyse import multislope as MS
    eng = HostEngine()
    batch = eng.wrap(eng.empty(8, eng.torch.float32), np.array([0]), np.array([MS.MAX_CHANNEL_SAMPLES + 1]))
    with pytest.raises(ValueError, match="channel 0 of the batch has 8384513 samples"):
        MS.multislope_device(eng, batch, 48000, MS.MultiSlopeSettings(bands=None))
    assert eng.calls() == [] and str(MS.MAX_CHANNEL_SAMPLES) in MS.build_parser().format_help().replace("\n", " ")


def _names(eng):
    return [n for n, _ in eng.calls()]


def test_call_sequence_on_the_recording_engine():
    """The same library calls in the same order for one batch and for the same channels split over two."""
    from host_engine import HostEngine
    from audio_analysis_amd.analyse import multislope as MS
    from audio_analysis_amd.analyse.rt60bands import Rt60BandsAnalysisSettings
    rng = np.random.default_rng(0)
    chans = [rng.standard_normal(n).astype(np.float32) for n in (6001, 6001, 6001, 6001)]
    s = MS.MultiSlopeSettings(bands=Rt60BandsAnalysisSettings(band_mode="three"), refine_levels=2, max_order=2)
    eng = HostEngine()
    dev = MS.multislope_device(eng, eng.upload(chans), 48000, s)
    whole = _names(eng)
    ms = [n for n in whole if n.startswith("ira_multislope") or n == "ira_block_energy"]
    assert ms == ["ira_block_energy", "ira_multislope_points"] + ["ira_multislope_gram", "ira_multislope_search"] * 3
    assert len(dev.level_records) == 3 and tuple(dev.records.shape) == (16, 3, 16) and len(dev.bands) == 3
    # the job tables: level 0 one Gram job per row on the shared grid and a search job per row and order
    gram = eng.calls("ira_multislope_gram")
    search = eng.calls("ira_multislope_search")
    assert [c[1][10] for c in gram] == [16, 32, 32] and [c[1][3] for c in search] == [32, 32, 32]
    jobs = eng.table(gram[0][1][9])[: 48].reshape(16, 3)
    assert jobs[:, 0].tolist() == list(range(16)) and np.all(jobs[:, 1] == 0) and jobs[:, 2].tolist() == list(range(16))
    jobs = eng.table(search[1][1][2])[: 128].reshape(32, 4)
    assert jobs[:4].tolist() == [[0, 1, 0, 0], [0, 2, 1, 1], [1, 1, 3, 3], [1, 2, 4, 4]]
    h0 = math.log(400.0) / 63.0
    assert [c[1][12] for c in search] == [h0 / 4, h0 / 16, 0.0] and [c[1][8] for c in search] == [64, 21, 21]
    assert search[2][1][13] is None and search[2][1][14] is None and search[0][1][13] is not None
    res = MS.multislope_results(dev, 48000, ["a", "b", "c", "d"], s)
    assert [r.channel_name for r in res] == ["a", "b", "c", "d"] and len(res[0].band_values_by_name) == 3
    eng2 = HostEngine()
    MS.multislope_device(eng2, eng2.upload(chans[:2]), 48000, s)
    first = _names(eng2)
    eng3 = HostEngine()
    MS.multislope_device(eng3, eng3.upload(chans[2:]), 48000, s)
    assert first == whole and _names(eng3) == whole
    # no band bank: the same chain without the filter bank's calls
    eng4 = HostEngine()
    MS.multislope_device(eng4, eng4.upload(chans), 48000, MS.MultiSlopeSettings(bands=None, refine_levels=0))
    assert [n for n in _names(eng4) if "multislope" in n] == ["ira_multislope_points", "ira_multislope_gram", "ira_multislope_search"]
    assert not any("irfft" in n for n in _names(eng4))


def test_engine_wrappers_refuse_bad_tables_before_any_launch():
    from audio_analysis_amd.engine import multislope_jobs, multislope_slot_doubles
    assert multislope_slot_doubles(64) == 66 * 67 // 2 and multislope_slot_doubles(128) == 130 * 131 // 2
    assert multislope_jobs([[0, 0, 0], [2, 1, 5]], 3, 3, 2, 6, 21).dtype == np.int32
    for jobs, width, what in (([[3, 0, 0]], 3, "column 0"), ([[0, 2, 0]], 3, "column 1"), ([[0, 0, 6]], 3, "column 2"),
                              ([[0, 0, 0, 0]], 4, "column 1"), ([[0, 4, 0, 0]], 4, "column 1"), ([[0, 1, 6, 0]], 4, "column 2"),
                              ([[0, 1, 0, 2]], 4, "column 3"), ([[-1, 1, 0, 0]], 4, "column 0")):
        with pytest.raises(ValueError, match=what):
            multislope_jobs(jobs, width, 3, 2, 6, 21)
    with pytest.raises(ValueError, match="1 .. 128"):
        multislope_jobs([[0, 0, 0]], 3, 3, 2, 6, 129)


def test_entry_points_validate_arguments_without_gpu():
    from audio_analysis_amd import _lib
    lib = _lib.load()
    E_NULL, E_SIZE = -1, -2
    # ira_multislope_points(base_len, chan_of_seg, start, blk_size, nblk, blk_off, nseg, blk, fit_fraction, d, info, rec, stream)
    ok = [1, 1, 1, 1, 1, 1, 1, 1, 0.9, 1, 1, 1, 0]
    for i in (0, 1, 2, 3, 4, 5, 7, 9, 10, 11):
        args = list(ok)
        args[i] = 0
        assert lib.ira_multislope_points(*args) == E_NULL, i
    for i, v in ((6, -1), (6, 65536), (8, 0.0), (8, 1.5), (8, float("nan"))):
        args = list(ok)
        args[i] = v
        assert lib.ira_multislope_points(*args) == E_SIZE, (i, v)
    assert lib.ira_multislope_points(*[0 if i == 6 else a for i, a in enumerate(ok)]) == 0       # empty batch: nothing to do
    # ira_multislope_gram(base_len, chan_of_seg, start, blk_size, nblk, blk_off, nseg, d, info, job, njobs, grid, grid_n,
    #                     grid_stride, ngrids, max_g, sample_rate_hz, nslots, gram, stream)
    ok = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 64, 1, 64, 48000.0, 1, 1, 0]
    for i in (0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 18):
        args = list(ok)
        args[i] = 0
        assert lib.ira_multislope_gram(*args) == E_NULL, i
    for i, v in ((6, -1), (6, 65536), (10, -1), (13, 63), (14, 0), (15, 0), (15, 129), (16, 0.0), (16, float("nan")), (17, 0)):
        args = list(ok)
        args[i] = v
        assert lib.ira_multislope_gram(*args) == E_SIZE, (i, v)
    for i in (6, 10):
        assert lib.ira_multislope_gram(*[0 if k == i else a for k, a in enumerate(ok)]) == 0
    # ira_multislope_search(nseg, info, job, njobs, grid, grid_n, grid_stride, ngrids, max_g, gram, nslots, min_ratio,
    #                       refine_step, grid_out, grid_n_out, rec, stream)
    ok = [1, 1, 1, 1, 1, 1, 64, 1, 64, 1, 1, 1.5, 0.02, 1, 1, 1, 0]
    for i in (1, 2, 4, 5, 9, 13, 14, 15):
        args = list(ok)
        args[i] = 0
        assert lib.ira_multislope_search(*args) == E_NULL, i
    for i, v in ((0, -1), (0, 65536), (3, -1), (6, 63), (7, 0), (8, 0), (8, 129), (10, 0), (11, 1.0), (11, float("nan")),
                 (12, -0.1), (12, float("inf"))):
        args = list(ok)
        args[i] = v
        assert lib.ira_multislope_search(*args) == E_SIZE, (i, v)
    for i in (0, 3):
        assert lib.ira_multislope_search(*[0 if k == i else a for k, a in enumerate(ok)]) == 0
    no_grid = list(ok)
    no_grid[0], no_grid[12], no_grid[13], no_grid[14] = 0, 0.0, 0, 0                 # refine_step = 0: the outputs may be NULL
    assert lib.ira_multislope_search(*no_grid) == 0


def test_header_lib_and_library_say_abi_15_and_export_the_symbols():
    from audio_analysis_amd import _lib, engine
    hdr = (REPO / "include" / "ira.h").read_text()
    assert re.search(r"#define IRA_ABI_VERSION 15\b", hdr) and _lib.ABI_VERSION == 15 and _lib.load().ira_abi_version() == 15
    lib = _lib.load()
    for name in ("ira_multislope_points", "ira_multislope_gram", "ira_multislope_search"):
        assert name in _lib.PROTOTYPES and re.search(rf"int32_t {name}\(", hdr) and getattr(lib, name) is not None
    for name, value in (("DOUBLES", engine.MS_DOUBLES), ("MAX_GRID", engine.MS_MAX_GRID), ("MAX_ORDER", engine.MS_MAX_ORDER),
                        ("TILE", engine.MS_TILE), ("REFINE_R", engine.MS_REFINE_R), ("REFINED", engine.MS_REFINED)):
        assert f"#define IRA_MS_{name} {value}\n" in hdr, name
    assert engine.MS_REFINED == (2 * engine.MS_REFINE_R + 1) * engine.MS_MAX_ORDER
    src = (REPO / "audio_analysis_amd" / "csrc" / "ira_multislope.hip").read_text()
    assert "atomic" not in src.replace("No atomics", "")
    from audio_analysis_amd import build
    assert build.SOURCES["ira_multislope.hip"] == ["-ffp-contract=off"]


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("noise", [False, True])
def test_restatement_recovers_exact_model_curves(order, noise):
    """d built from known T on the grid and known a: those indices, the coefficients to 1e-9, cost <= 1e-12 J."""
    R.need_longdouble()
    fs, L, B = 48000, 96000, 48
    grid, _ = R.level0()
    idx = {1: (26,), 2: (22, 36), 3: (14, 26, 41)}[order]
    a = {1: (2.0,), 2: (3.0, 0.2), 3: (5.0, 1.0, 0.05)}[order]
    a_nu = 1e-4 if noise else 0.0
    d = R.model_points(L, B, None, fs, [grid[i] for i in idx], a, a_nu)
    J = int(math.floor(0.9 * (L // B)))
    res = R.fit_points(d, J, L, B, fs, grid, order)
    assert res["found"] and res["idx"] == idx and res["noise"] == noise, (res["idx"], res["noise"])
    assert all(abs(float(res["a"][s] / R.LD(a[s]) - 1)) <= 1e-9 for s in range(order))
    assert (abs(float(res["a_nu"] / R.LD(a_nu) - 1)) <= 1e-9) if noise else res["a_nu"] == 0
    assert float(res["c"]) <= 1e-12 * J
    fin = R.finish(res, dict(L=L, J=J, d=d), fs)
    assert fin["rms_db"] <= 1e-5 and abs(fin["start_db"][0] - 10 * math.log10(a[0] * (1 - 1e-6 ** (L / fs / grid[idx[0]])) / float(d[0]))) < 1e-9


def test_restatement_meets_the_margin_condition_on_every_gpu_case():
    """The inputs of the GPU tests are chosen so that the restatement ALONE decides every index, noise flag and "no
    candidate" bit with a margin of at least 1e-6, and so that each case shows the path it is there for.  (The band rows of
    the chain test exist on the device only; that test asserts their margins itself.)"""
    R.need_longdouble()
    import test_gpu_multislope as T
    named = dict(T.fit_rows())
    seen = {}
    for name, grid, orders, mr in T.search_jobs():
        p = R.row_points(T._after_peak(named[name]), T.SR)
        assert p["status"] == 0
        G, b = R.gram(R.basis(grid, T.SR, p["L"], p["B"], p["J"], p["d"]))
        for S in orders:
            res = R.search(G, b, grid, p["J"], S, mr)
            assert R.margin_ok(res["margin"]), (name, len(grid), S, res["margin"])
            seen[(name, len(grid), S)] = res
    assert not seen[("one", 1, 2)]["found"] and seen[("one", 1, 2)]["candidates"] == 0 and seen[("one", 1, 1)]["found"]
    assert not seen[("three", 4, 3)]["found"] and seen[("three", 4, 3)]["candidates"] == 0 and seen[("three", 4, 2)]["found"]
    assert all(not seen[("two", 64, S)]["noise"] for S in (1, 2, 3)) and seen[("two floor", 64, 2)]["noise"]
    assert seen[("two floor", 128, 3)]["found"] and seen[("three", 64, 3)]["found"]
    for name, x in T.chain_channels():
        p = R.row_points(T._after_peak(x), T.SR)
        ch = R.chain(p, T.SR)
        for S, levels in ch.items():
            for lvl, res in enumerate(levels):
                assert R.margin_ok(res["margin"]), (name, S, lvl, res["margin"])
        rms = {S: R.rms_db(levels[-1]["c"], p["J"]) for S, levels in ch.items() if levels[-1]["found"]}
        if name == "one":
            assert R.preferred(rms) == 1 and abs(ch[1][-1]["T"][0] - 0.6) <= 0.02 * 0.6
        else:
            assert R.preferred(rms) == 2 and abs(ch[2][-1]["T"][1] - 1.5) <= 0.05 * 1.5 and rms[1] > 0.3
    fs, good, bad = T.status_rows()
    assert R.row_points(T._after_peak(good), fs)["status"] == 0
    for name, x, want in bad:
        assert R.row_points(T._after_peak(x) if np.isfinite(x).all() else x[int(np.nanargmax(np.abs(x))):], fs)["status"] == want, name
    rows = T.gram_rows()
    assert [int(math.floor(0.9 * (T._after_peak(x).size // 48))) for _, x in rows[2:]] == [28, 31, 32, 33, 63, 64, 65]


def test_restatement_levels_never_raise_the_cost_and_refine_around_the_winner():
    R.need_longdouble()
    import test_gpu_multislope as T
    x = dict(T.fit_rows())["two floor"]
    p = R.row_points(T._after_peak(x), T.SR)
    ch = R.chain(p, T.SR, max_order=2)
    for S, levels in ch.items():
        costs = [float(r["c"]) for r in levels]
        assert all(b <= a for a, b in zip(costs, costs[1:])), (S, costs)
        for prev, cur in zip(levels, levels[1:]):
            assert set(prev["T"]) <= set(cur["grid"].tolist()) and cur["grid"].size <= 7 * S
            assert abs(cur["step"] - prev["step"] / 4) < 1e-18
