"""
CPU-only tests of the Lundeby noise handling (audio_analysis_amd.analyse.lundeby): block and interval sizes, the row
tables' host layout, settings validation, status / validity arithmetic, the fixed text / Markdown / JSON formats on
hand-built results, the command line's parser, the argument checks of the new C entry points (they return before
touching a device), and the restatement of tests/lundeby_ref.py itself: the conditions the GPU tests' inputs must meet
are conditions on the restatement alone and are checked here.
"""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import lundeby_ref as R

REPO = Path(__file__).resolve().parent.parent


def test_block_size_and_first_interval():
    from audio_analysis_amd.analyse import lundeby as L
    assert L.block_size(48000, 31 * 48) == 48 and L.block_size(48000, 4096 * 48) == 48
    assert L.block_size(48000, 4096 * 48 + 1) == 49 and L.block_size(48000, 480000) == 118
    assert L.block_size(44100, 1000) == 45 and L.block_size(8000, 20000) == 8 and L.block_size(8000, 4096 * 8 + 1) == 9
    assert L.block_size(500, 10) == 1 and L.block_size(48000, 0) == 48
    assert L.first_interval_blocks(48000, 48) == 30 and L.first_interval_blocks(48000, 118) == 12
    assert L.first_interval_blocks(44100, 45) == 29 and L.first_interval_blocks(8000, 8) == 30
    assert L.first_interval_blocks(48000, 4000) == 1
    for fs, n in ((48000, 480000), (44100, 1807), (8000, 20000), (96000, 5_000_000)):
        assert L.block_size(fs, n) == R.block_size(fs, n)
        assert L.first_interval_blocks(fs, L.block_size(fs, n)) == R.first_interval(fs, R.block_size(fs, n))
        assert n // L.block_size(fs, n) <= L.MAX_BLOCKS


def test_row_tables_and_layout():
    from audio_analysis_amd.analyse import lundeby as L
    from audio_analysis_amd.engine import LUNDEBY_MAX_LEN, lundeby_layout
    ln, b, nb, m0 = L.row_tables([480000, 2000, 196700], [7, 0, 91], 48000, 2)
    assert ln.tolist() == [479993, 2000, 196609]
    assert b.tolist() == [118] * 3 + [48] * 3 + [49] * 3 and nb.tolist() == [4067] * 3 + [41] * 3 + [4012] * 3
    assert m0.tolist() == [12] * 3 + [30] * 3 + [29] * 3
    with pytest.raises(ValueError, match="start index"):
        L.row_tables([10], [11], 48000, 0)
    lay = lundeby_layout(np.arange(9) * 500000, np.repeat([480000, 2000, 196700], 3), np.repeat([0, 1, 2], 3), b, nb, m0)
    assert lay["nseg"] == 9 and lay["stride"] == 4068 and lay["table_doubles"] == 9 * 4068
    assert lay["blk_off"].tolist() == [j * 4068 for j in range(9)]
    # chunks of 4096 // B whole blocks cover the nb + 1 table entries: 34 blocks of 118, 85 of 48, 83 of 49
    assert lay["max_chunks"] == max(-(-4068 // 34), -(-42 // 85), -(-4013 // 83)) == 120
    assert lay["blk_size"].dtype == np.int32 and lay["base_off"].dtype == np.int64 and lay["chan_of_seg"].dtype == np.int32
    empty = lundeby_layout([], [], [], [], [], [])
    assert empty["nseg"] == 0 and empty["table_doubles"] == 0 and empty["max_chunks"] == 1
    ok = dict(base_off=[0], base_len=[1000], chan_of_seg=[0], blk_size=[8], nblk=[125], first_m=[30])
    lundeby_layout(**ok)
    for key, bad, what in (("blk_size", [0], "block sizes"), ("blk_size", [4097], "block sizes"), ("nblk", [4097], "block counts"),
                           ("nblk", [-1], "block counts"), ("first_m", [0], "first_m"), ("nblk", [126], "nb \\* B"),
                           ("base_len", [LUNDEBY_MAX_LEN + 1], "nb \\* B"), ("chan_of_seg", [-1], "chan_of_seg"),
                           ("nblk", [1, 2], "one entry per row")):
        with pytest.raises(ValueError, match=what):
            lundeby_layout(**dict(ok, **{key: bad}))


def test_settings_defaults_and_validation():
    from audio_analysis_amd.analyse.decay import DecayAnalysisSettings
    from audio_analysis_amd.analyse.lundeby import LundebySettings
    from audio_analysis_amd.analyse.rt60bands import Rt60BandsAnalysisSettings
    s = LundebySettings()
    assert s.mode == "compensate" and s.compensate and s.bands.band_mode == "octave" and s.decay.compute_edt
    assert s.decay.edc_epsilon == 1e-20 and s.decay.edc_floor_db == -120.0 and not s.use_mono_downmix_for_stereo
    assert not LundebySettings(mode="truncate").compensate and LundebySettings(bands=None).bands is None
    for bad, what in [(dict(mode="subtract"), "mode"),
                      (dict(decay=DecayAnalysisSettings()), "compute_edt"),
                      (dict(decay="fast"), "DecayAnalysisSettings"),
                      (dict(decay=DecayAnalysisSettings(compute_edt=True, edc_smoothing_window_samples=5)), "smoothing"),
                      (dict(decay=DecayAnalysisSettings(compute_edt=True, edc_epsilon=-1.0)), "edc_epsilon"),
                      (dict(decay=DecayAnalysisSettings(compute_edt=True, edc_floor_db=float("nan"))), "edc_floor_db"),
                      (dict(decay=DecayAnalysisSettings(compute_edt=True, t30_range_db=(-35.0, -5.0))), "range_db"),
                      (dict(bands=Rt60BandsAnalysisSettings(band_mode="sixth")), "band_mode"),
                      (dict(bands="octave"), "bands")]:
        with pytest.raises(ValueError, match=what):
            LundebySettings(**bad)


def test_status_and_validity_arithmetic():
    from audio_analysis_amd.analyse import lundeby as L
    assert L.validity(-45.0) == (True, True, True) and L.validity(-44.999) == (True, True, False)
    assert L.validity(-35.0) == (True, True, False) and L.validity(-34.9) == (True, False, False)
    assert L.validity(-20.0) == (True, False, False) and L.validity(-19.9) == (False, False, False)
    assert L.validity(float("nan")) == (False, False, False)
    assert L.status_text(0) == "ok" and L.status_text(32) == "32 (no noise floor in file)"
    assert L.status_text(2) == "2 (too short)" and L.status_text(4 | 8) == "12 (no decay range, slope not negative)"
    assert (L.STATUS_SILENT, L.STATUS_TOO_SHORT, L.STATUS_NO_RANGE, L.STATUS_SLOPE, L.STATUS_NON_FINITE, L.STATUS_NO_FLOOR) == \
        (R.S_SILENT, R.S_SHORT, R.S_NO_RANGE, R.S_SLOPE, R.S_NON_FINITE, R.S_NO_FLOOR)
    rec = np.full(16, np.nan)
    fits = np.zeros((3, 8))
    fits[:, 0] = 1.0
    fits[:, 6] = (0.9, 1.0, 1.1)
    for st in (1, 2, 4, 8, 16):
        rec[0] = st
        v = L.values_from_records(rec, fits, 48000)
        assert v.status == st and all(math.isnan(getattr(v, f)) for f in L._FLOAT_FIELDS)
        assert not (v.edt_valid or v.t20_valid or v.t30_valid)
    rec = np.array([32.0, -40.0, 48000.0, -60.0 / 48000.0, 0.5, 0.0, 2, 10, 0, 5, 15, 47000.0, 50000.0, 1.0, 3.0, 100])
    fits[2, 0] = 0.0                                                          # T30 range not available
    v = L.values_from_records(rec, fits, 48000)
    assert v.status == 32 and v.noise_db == -40.0 and v.dynamic_range_db == 40.0 and v.cross_point_seconds == 1.0
    assert v.late_slope_db_per_second == -60.0 and v.compensation_energy == 0.0
    assert (v.edt_seconds, v.t20_seconds) == (0.9, 1.0) and math.isnan(v.t30_seconds)
    assert (v.edt_valid, v.t20_valid, v.t30_valid) == (True, True, False)


def _hand_built():
    from audio_analysis_amd.analyse.lundeby import LundebyChannelResult, LundebyValues
    from audio_analysis_amd.analyse.rt60bands import BandDefinition
    nan = float("nan")
    bands = [BandDefinition("500Hz", 500.0, "band", 353.55, 707.11), BandDefinition("1000Hz", 1000.0, "band", 707.11, 1414.21)]
    a = LundebyChannelResult(
        "hall.wav:left", 48000, "compensate", 240, LundebyValues(0, -43.371, 0.74733, 43.371, -58.824, 1.23456e-3, 1.0123, 1.0204,
                                                                  1.0365, True, True, False),
        bands, {"500Hz": LundebyValues(32, -50.0, 2.0, 50.0, -30.0, 0.0, 1.9, 2.0, 2.1, True, True, True),
                "1000Hz": LundebyValues(4, nan, nan, nan, nan, nan, nan, nan, nan, False, False, False)})
    b = LundebyChannelResult("mono.wav:mono", 44100, "truncate", 0,
                             LundebyValues(0, -18.0, 0.5, 18.0, -20.5, 0.0, 2.9, nan, nan, False, False, False), [], {})
    return [a, b]


def test_summary_text_format_is_pinned():
    from audio_analysis_amd.analyse.lundeby import summarise_lundeby_text
    assert summarise_lundeby_text(_hand_built()) == (
        "[hall.wav:left]\n"
        "Start: 240 samples (5.000 ms)  Mode: compensate\n"
        "Band  Noise_dB  Cross_ms  Range_dB  Slope_dB_s  C  EDT_s  T20_s  T30_s  Valid  Status\n"
        "Broadband  -43.37  747.3  43.37  -58.82  1.2346e-03  1.012  1.020  1.036  EDT+T20  ok\n"
        "500Hz  -50.00  2000.0  50.00  -30.00  0.0000e+00  1.900  2.000  2.100  EDT+T20+T30  32 (no noise floor in file)\n"
        "1000Hz  NA  NA  NA  NA  NA  NA  NA  NA  none  4 (no decay range)\n"
        "\n"
        "[mono.wav:mono]\n"
        "Start: 0 samples (0.000 ms)  Mode: truncate\n"
        "Band  Noise_dB  Cross_ms  Range_dB  Slope_dB_s  C  EDT_s  T20_s  T30_s  Valid  Status\n"
        "Broadband  -18.00  500.0  18.00  -20.50  0.0000e+00  2.900  NA  NA  none  ok\n"
        "\n")
    assert summarise_lundeby_text([]) == ""


def test_summary_markdown_format_is_pinned():
    from audio_analysis_amd.analyse.lundeby import summarise_lundeby_markdown
    assert summarise_lundeby_markdown(_hand_built()[1:]) == (
        "### mono.wav:mono\n"
        "\n"
        "Start: 0 samples (0.000 ms). Mode: truncate.\n"
        "\n"
        "| Band | Noise (dB) | Cross-point (ms) | Range (dB) | Late slope (dB/s) | C | EDT (s) | T20 (s) | T30 (s) | Valid | Status |\n"
        "|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|\n"
        "| Broadband | -18.00 | 500.0 | 18.00 | -20.50 | 0.0000e+00 | 2.900 | NA | NA | none | ok |\n"
        "\n")
    assert "| 1000Hz | NA | NA | NA | NA | NA | NA | NA | NA | none | 4 (no decay range) |\n" in summarise_lundeby_markdown(_hand_built())


def test_json_round_trip_keeps_nan():
    from audio_analysis_amd.analyse.lundeby import lundeby_results_from_json, lundeby_results_to_json, summarise_lundeby_text
    res = _hand_built()
    doc = json.loads(json.dumps(lundeby_results_to_json(res), allow_nan=False))          # strict JSON: no NaN tokens
    assert doc["lundeby"][0]["bands"][1]["t30_seconds"] is None and doc["lundeby"][0]["bands"][1]["status"] == 4
    assert doc["lundeby"][1]["broadband"]["t20_seconds"] is None and doc["lundeby"][1]["mode"] == "truncate"
    assert doc["lundeby"][0]["broadband"]["t30_valid"] is False and doc["lundeby"][0]["broadband"]["noise_db"] == -43.371
    back = lundeby_results_from_json(doc)
    assert summarise_lundeby_text(back) == summarise_lundeby_text(res)
    assert back[0].broadband == res[0].broadband and back[0].band_definitions == res[0].band_definitions
    assert back[0].band_values_by_name["500Hz"] == res[0].band_values_by_name["500Hz"]
    assert math.isnan(back[0].band_values_by_name["1000Hz"].noise_db) and back[1].start_samples == 0


def test_cli_parser_defaults_and_help():
    from audio_analysis_amd.analyse import lundeby
    p = lundeby.build_parser()
    a = p.parse_args(["--input", "a.wav", "b.wav"])
    assert a.input == [Path("a.wav"), Path("b.wav")] and a.bundle is None
    assert (a.bands, a.mode, a.mono, a.expected_sample_rate, a.json) == ("octave", "compensate", False, 48000, None)
    assert lundeby.settings_from_args(a) == lundeby.LundebySettings()
    a = p.parse_args(["--bundle", "d", "--bands", "none", "--mode", "truncate", "--mono", "--expected-sample-rate", "44100",
                      "--json", "o.json"])
    assert a.bundle == Path("d") and a.expected_sample_rate == 44100 and a.json == Path("o.json")
    s = lundeby.settings_from_args(a)
    assert s.bands is None and s.mode == "truncate" and s.use_mono_downmix_for_stereo
    for bad in ([], ["--input", "a.wav", "--bundle", "d"], ["--input", "a.wav", "--bands", "sixth"],
                ["--input", "a.wav", "--mode", "subtract"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.lundeby", "--help"], capture_output=True, text=True, cwd=str(REPO),
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--input", "--bundle", "--mono", "--bands", "--mode", "--expected-sample-rate", "--json"):
        assert flag in r.stdout


def test_shim_re_exports_the_module():
    import analyse.lundeby as shim
    from audio_analysis_amd.analyse import lundeby
    assert shim is lundeby


def test_entry_points_validate_arguments_without_gpu():
    from audio_analysis_amd import _lib
    lib = _lib.load()
    E_NULL, E_SIZE = -1, -2
    # ira_block_energy(x, base_off, base_len, chan_of_seg, start, blk_size, nblk, blk_off, nseg, max_chunks, blk, stream)
    ok = [1, 1, 1, 1, 1, 1, 1, 1, 1, 4, 1, 0]
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 10):
        args = list(ok)
        args[i] = 0
        assert lib.ira_block_energy(*args) == E_NULL, i
    for i, v in ((8, -1), (8, 65536), (9, 0), (9, 4098)):
        args = list(ok)
        args[i] = v
        assert lib.ira_block_energy(*args) == E_SIZE, (i, v)
    assert lib.ira_block_energy(*[0 if i == 8 else a for i, a in enumerate(ok)]) == 0      # empty batch: nothing to do
    # ira_lundeby_estimate(base_len, chan_of_seg, start, blk_size, nblk, first_m, blk_off, nseg, blk, compensate, rec, len_out,
    #                      suffix, stream)
    ok = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0]
    for i in (0, 1, 2, 3, 4, 5, 6, 8, 10, 11, 12):
        args = list(ok)
        args[i] = 0
        assert lib.ira_lundeby_estimate(*args) == E_NULL, i
    for i, v in ((7, -1), (7, 65536), (9, 2), (9, -1)):
        args = list(ok)
        args[i] = v
        assert lib.ira_lundeby_estimate(*args) == E_SIZE, (i, v)
    assert lib.ira_lundeby_estimate(*[0 if i == 7 else a for i, a in enumerate(ok)]) == 0
    # ira_edc_truncated(x, base_off, base_len, chan_of_seg, start, blk_size, nblk, blk_off, nseg, max_chunks, rec, len, suffix,
    #                   eps, floor_db, edc, edc_off, stream)
    ok = [1, 1, 1, 1, 1, 1, 1, 1, 1, 4, 1, 1, 1, 1e-20, -120.0, 1, 1, 0]
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 15, 16):
        args = list(ok)
        args[i] = 0
        assert lib.ira_edc_truncated(*args) == E_NULL, i
    for i, v in ((8, -1), (8, 65536), (9, 0), (9, 4098), (13, -1.0), (13, float("nan")), (14, float("nan"))):
        args = list(ok)
        args[i] = v
        assert lib.ira_edc_truncated(*args) == E_SIZE, (i, v)
    assert lib.ira_edc_truncated(*[0 if i == 8 else a for i, a in enumerate(ok)]) == 0
    # tables: nb + 1 doubles per row at the stride of the longest row
    assert lib.ira_lundeby_scratch_doubles(3, 4096) == 3 * 4097 and lib.ira_lundeby_scratch_doubles(2560, 4067) == 2560 * 4068
    assert lib.ira_lundeby_scratch_doubles(0, 10) == 0 and lib.ira_lundeby_scratch_doubles(5, 0) == 5
    for bad in ((-1, 10), (65536, 10), (1, -1), (1, 4097)):
        assert lib.ira_lundeby_scratch_doubles(*bad) == E_SIZE, bad


def test_engine_wrappers_refuse_bad_tables_before_any_launch():
    """The wrappers' host checks need no device: lundeby_rows raises on the tables' layout before anything is uploaded."""
    from audio_analysis_amd.engine import Engine
    eng = Engine.__new__(Engine)                                            # no device, no library: the checks come first
    with pytest.raises(ValueError, match="block sizes"):
        eng.lundeby_rows([0], [1000], [0], [5000], [0], [1])
    with pytest.raises(ValueError, match="nb \\* B"):
        eng.lundeby_rows([0], [1000], [0], [8], [126], [30])


def test_channel_length_limit_is_an_argument_error_that_names_the_channel():
    from audio_analysis_amd.analyse import lundeby as L
    assert L.MAX_CHANNEL_SAMPLES == 2047 * 4096
    L.check_channel_lengths([0, 1000, L.MAX_CHANNEL_SAMPLES])
    with pytest.raises(ValueError, match="channel 2 of the batch has 8384513 samples"):
        L.check_channel_lengths([10, L.MAX_CHANNEL_SAMPLES, L.MAX_CHANNEL_SAMPLES + 1])
    assert str(L.MAX_CHANNEL_SAMPLES) in L.build_parser().format_help().replace("\n", " ")


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_meets_the_margin_condition_on_every_gpu_case():
    """The inputs of the GPU tests are chosen so that the restatement ALONE decides every integer with a margin of at least
    1e-6 dB and 1e-6 of an interval, and so that each case shows the path it is there for."""
    R.need_longdouble()
    import test_gpu_lundeby as T
    refs = []
    for name, fs, x in T.estimate_cases():
        refs.append((name, R.estimate(x[int(np.argmax(np.abs(x))):], fs)))
    T.check_case_conditions(refs)
    fs, good, bad = T.status_rows()
    assert R.estimate(good[int(np.argmax(np.abs(good))):], fs)["status"] == 0
    for name, x, want in bad[:3]:
        assert R.estimate(x[int(np.argmax(np.abs(x))):], fs)["status"] == want, name
    s, band_refs = T.band_references(T.band_case())
    assert sum(0 if r["margin"].ok() else 1 for _, _, r in band_refs) <= 2
    assert sum(1 for _, _, r in band_refs if r["status"] == 0) >= 7


def test_restatement_recovers_the_decay_and_the_plain_integration_does_not():
    R.need_longdouble()
    fs = 8000
    x = R.decaying_noise(fs, 4.0, 0.6, -45, 1)
    y = x[int(np.argmax(np.abs(x))):]
    r = R.estimate(y, fs)
    assert r["status"] == 0 and r["rounds"] <= 2 and abs(-60.0 / float(r["slope"]) / fs - 0.6) < 0.03

    def t30(curve):
        t = np.arange(curve.size) / fs
        a, b = int(np.argmax(curve <= -5.0)), int(np.argmax(curve <= -35.0))
        return -60.0 / np.polyfit(t[a:b], curve[a:b].astype(np.float64), 1)[0]

    _, comp = R.curve(y, r["length"], r["C"], 1e-20, -120.0)
    _, trunc = R.curve(y, r["length"], 0.0, 1e-20, -120.0)
    _, plain = R.curve(y, y.size, 0.0, 1e-20, -120.0)
    assert abs(t30(comp) - 0.6) < 0.03 and abs(t30(trunc) - 0.6) < 0.03 and abs(t30(plain) - 0.6) > 0.06
    assert comp[0] == 0.0 and np.all(np.diff(comp) <= 0.0)
    # t1 is block-aligned, inside the file, and the truncate mode only drops C
    assert r["t1"] % r["B"] == 0 and r["B"] <= r["t1"] <= r["nb"] * r["B"]
    r0 = R.estimate(y, fs, compensate=False)
    assert float(r0["C"]) == 0.0 and r0["t1"] == r["t1"] and float(r0["Ln"]) == float(r["Ln"])


def test_float64_curve_matches_long_double_on_99_percent():
    """The share of float32 samples on which a plain float64 curve equals the long-double one: what the GPU curve test
    requires of the kernel (99 %) is met by float64 arithmetic as such."""
    R.need_longdouble()
    fs = 8000
    x = R.decaying_noise(fs, 1.5, 0.5, -50, 0)
    y = x[int(np.argmax(np.abs(x))):]
    r = R.estimate(y, fs)
    _, a = R.curve(y, r["length"], r["C"], 1e-20, -120.0)
    _, b = R.curve(y, r["length"], float(r["C"]), 1e-20, -120.0, dtype=np.float64)
    assert np.mean(a.view(np.uint32) == b.view(np.uint32)) >= 0.99
    bound = R.curve_bound_db(y, r["length"], r["C"], 1e-20)
    assert np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= bound + np.spacing(np.abs(a)).astype(np.float64))
