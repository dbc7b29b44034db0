"""
CPU-only tests of the ISO 3382-1 energy parameters (audio_analysis_amd.analyse.energy): window counts, settings
validation, the fixed text / Markdown / JSON formats on hand-built results, the command line's parser, and the argument
checks of the new C entry points (they return before touching a device).
"""
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent


def test_window_counts_at_common_rates():
    from audio_analysis_amd.analyse.energy import window_samples
    assert window_samples((50.0, 80.0), 48000) == [2400, 3840]
    assert window_samples((50.0, 80.0), 44100) == [2205, 3528]
    assert window_samples((50.0, 80.0), 22050) == [1103, 1764]          # 1102.5 rounds up
    assert window_samples((50.0, 80.0), 96000) == [4800, 7680]
    # non-integer products round up; the expression is evaluated in float64 in exactly this order
    for fs in (22050, 44100, 48000, 96000):
        for ms in (1.0, 12.5, 33.3, 50.0, 80.0, 100.0, 0.01):
            assert window_samples((ms,), fs) == [math.ceil(ms * fs / 1000.0)]
    assert window_samples((12.5,), 44100) == [552]                       # 551.25
    assert window_samples((33.3,), 48000) == [1599]                      # 1598.4
    assert window_samples((0.01,), 22050) == [1]                         # 0.2205


def test_settings_defaults_and_validation():
    from audio_analysis_amd.analyse.energy import EnergyParameterSettings
    from audio_analysis_amd.analyse.rt60bands import Rt60BandsAnalysisSettings
    s = EnergyParameterSettings()
    assert s.onset_db == -20.0 and s.early_limits_ms == (50.0, 80.0) and s.bands.band_mode == "octave"
    assert not s.use_mono_downmix_for_stereo
    assert s.rel_energy == 10.0 ** (-20.0 / 10.0) and s.definition_limit_ms == 50.0
    assert EnergyParameterSettings(early_limits_ms=[80, 100]).early_limits_ms == (80.0, 100.0)
    assert EnergyParameterSettings(early_limits_ms=(80.0, 100.0)).definition_limit_ms == 80.0
    assert EnergyParameterSettings(early_limits_ms=(20.0, 50.0, 80.0)).definition_limit_ms == 50.0
    assert EnergyParameterSettings(onset_db=0.0).rel_energy == 1.0
    assert EnergyParameterSettings(bands=None).bands is None
    for bad, what in [(dict(early_limits_ms=(80.0, 50.0)), "ascending"),
                      (dict(early_limits_ms=(50.0, 50.0)), "ascending"),
                      (dict(early_limits_ms=()), "1 to 4"),
                      (dict(early_limits_ms=(10.0, 20.0, 30.0, 40.0, 50.0)), "1 to 4"),
                      (dict(early_limits_ms=(0.0, 50.0)), "positive"),
                      (dict(early_limits_ms=(-5.0,)), "positive"),
                      (dict(early_limits_ms=(float("nan"),)), "positive"),
                      (dict(onset_db=3.0), "onset_db"),
                      (dict(onset_db=float("nan")), "onset_db"),
                      (dict(bands=Rt60BandsAnalysisSettings(band_mode="sixth")), "band_mode")]:
        with pytest.raises(ValueError, match=what):
            EnergyParameterSettings(**bad)


def _hand_built():
    from audio_analysis_amd.analyse.energy import EnergyParameters, EnergyParametersChannelResult
    from audio_analysis_amd.analyse.rt60bands import BandDefinition
    nan, inf = float("nan"), float("inf")
    bands = [BandDefinition("500Hz", 500.0, "bandpass", 353.6, 707.1), BandDefinition("1000Hz", 1000.0, "bandpass", 707.1, 1414.2)]
    ok = EnergyParametersChannelResult(
        channel_name="left", sample_rate_hz=48000, early_limits_ms=(50.0, 80.0), definition_limit_ms=50.0,
        onset_samples=240, onset_seconds=0.005, status=0,
        broadband=EnergyParameters((1.23456, 4.5), 0.571234, 0.0482149),
        band_definitions=bands,
        band_parameters_by_name={"500Hz": EnergyParameters((-2.0, -0.004), 0.38, 0.1),
                                 "1000Hz": EnergyParameters((inf, inf), 1.0, 0.0)})
    bad = EnergyParametersChannelResult(
        channel_name="right", sample_rate_hz=48000, early_limits_ms=(80.0,), definition_limit_ms=80.0,
        onset_samples=0, onset_seconds=0.0, status=3,
        broadband=EnergyParameters((nan,), nan, nan), band_definitions=[], band_parameters_by_name={})
    return [ok, bad]


def test_summary_text_format_is_pinned():
    from audio_analysis_amd.analyse.energy import summarise_energy_parameters_text
    assert summarise_energy_parameters_text(_hand_built()) == (
        "[left]\n"
        "Onset: 240 samples (5.000 ms)  Status: ok\n"
        "Band  C50_dB  C80_dB  D50  Ts_ms\n"
        "Broadband  1.23  4.50  0.571  48.21\n"
        "500Hz  -2.00  -0.00  0.380  100.00\n"
        "1000Hz  +inf  +inf  1.000  0.00\n"
        "\n"
        "[right]\n"
        "Onset: 0 samples (0.000 ms)  Status: 3 (silent, too short)\n"
        "Band  C80_dB  D80  Ts_ms\n"
        "Broadband  NA  NA  NA\n"
        "\n")
    assert summarise_energy_parameters_text([]) == ""


def test_summary_markdown_format_is_pinned():
    from audio_analysis_amd.analyse.energy import summarise_energy_parameters_markdown
    assert summarise_energy_parameters_markdown(_hand_built()) == (
        "### left\n"
        "\n"
        "Onset: 240 samples (5.000 ms). Status: ok.\n"
        "\n"
        "| Band | C50 (dB) | C80 (dB) | D50 | Ts (ms) |\n"
        "|---|---:|---:|---:|---:|\n"
        "| Broadband | 1.23 | 4.50 | 0.571 | 48.21 |\n"
        "| 500Hz | -2.00 | -0.00 | 0.380 | 100.00 |\n"
        "| 1000Hz | +inf | +inf | 1.000 | 0.00 |\n"
        "\n"
        "### right\n"
        "\n"
        "Onset: 0 samples (0.000 ms). Status: 3 (silent, too short).\n"
        "\n"
        "| Band | C80 (dB) | D80 | Ts (ms) |\n"
        "|---|---:|---:|---:|\n"
        "| Broadband | NA | NA | NA |\n"
        "\n")


def test_json_round_trip_keeps_nan_and_infinite_clarity():
    import json
    from audio_analysis_amd.analyse.energy import (energy_results_from_json, energy_results_to_json,
                                                   summarise_energy_parameters_text)
    res = _hand_built()
    doc = json.loads(json.dumps(energy_results_to_json(res)))          # strict JSON: no NaN / Infinity tokens
    assert doc["energy_parameters"][0]["bands"][1]["clarity_db"] == ["+inf", "+inf"]
    assert doc["energy_parameters"][1]["broadband"]["definition"] is None
    back = energy_results_from_json(doc)
    assert summarise_energy_parameters_text(back) == summarise_energy_parameters_text(res)
    assert back[0].broadband == res[0].broadband and back[0].band_definitions == res[0].band_definitions
    assert math.isnan(back[1].broadband.centre_time_seconds) and back[1].status == 3


def test_parameters_from_sums_definitions():
    import numpy as np
    from audio_analysis_amd.analyse.energy import parameters_from_sums
    # P_0, P_1, P_2, S1
    sums = np.array([[4.0, 1.0, 1.0, 12.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    c, d, ts = parameters_from_sums(sums, 1000.0, 0)
    assert c[0, 0] == 10.0 * math.log10(4.0 / 2.0) and c[0, 1] == 10.0 * math.log10(5.0 / 1.0)
    assert d[0] == 4.0 / 6.0 and ts[0] == 12.0 / (1000.0 * 6.0)
    assert c[1, 0] == math.inf and c[1, 1] == math.inf and d[1] == 1.0 and ts[1] == 0.0      # a Dirac
    assert np.isnan(c[2]).all() and np.isnan(d[2]) and np.isnan(ts[2])                    # silence


def test_cli_parser_defaults_and_help():
    from audio_analysis_amd.analyse import energy
    p = energy.build_parser()
    a = p.parse_args(["--input", "a.wav", "b.wav"])
    assert a.input == [Path("a.wav"), Path("b.wav")] and a.bundle is None
    assert (a.mono, a.bands, a.onset_db, a.limits_ms, a.expected_sample_rate, a.json) == \
        (False, "octave", -20.0, [50.0, 80.0], 48000, None)
    s = energy.settings_from_args(a)
    assert s.bands.band_mode == "octave" and s.early_limits_ms == (50.0, 80.0)
    a = p.parse_args(["--bundle", "d", "--mono", "--bands", "none", "--onset-db", "-40", "--limits-ms", "80",
                      "--expected-sample-rate", "44100", "--json", "o.json"])
    assert a.bundle == Path("d") and a.mono and a.bands == "none" and a.onset_db == -40.0 and a.limits_ms == [80.0]
    assert a.expected_sample_rate == 44100 and a.json == Path("o.json")
    assert energy.settings_from_args(a).bands is None
    for bad in ([], ["--input", "a.wav", "--bundle", "d"], ["--input", "a.wav", "--bands", "sixth"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit):                                       # invalid settings end as a usage error
        energy.main(["--input", "a.wav", "--limits-ms", "80", "50"])
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.energy", "--help"], capture_output=True, text=True, cwd=str(REPO),
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--input", "--bundle", "--mono", "--bands", "--onset-db", "--limits-ms", "--expected-sample-rate", "--json"):
        assert flag in r.stdout


def test_shim_re_exports_the_module():
    import analyse.energy as shim
    from audio_analysis_amd.analyse import energy
    assert shim is energy


def test_energy_entry_points_validate_arguments_without_gpu():
    from audio_analysis_amd import _lib
    lib = _lib.load()
    E_NULL, E_SIZE = -1, -2
    # ira_onset_index(x, off, len, nseg, max_len, peak, peak_abs, rel_energy, onset, stream)
    assert lib.ira_onset_index(0, 1, 1, 1, 16, 1, 1, 0.01, 1, 0) == E_NULL
    assert lib.ira_onset_index(1, 1, 1, 1, 16, 1, 0, 0.01, 1, 0) == E_NULL
    assert lib.ira_onset_index(1, 1, 1, 1, 16, 1, 1, 0.01, 0, 0) == E_NULL
    assert lib.ira_onset_index(1, 1, 1, 1, 16, 1, 1, 1.5, 1, 0) == E_SIZE          # onset_db > 0
    assert lib.ira_onset_index(1, 1, 1, 1, 16, 1, 1, -0.1, 1, 0) == E_SIZE
    assert lib.ira_onset_index(1, 1, 1, 1, 16, 1, 1, float("nan"), 1, 0) == E_SIZE
    assert lib.ira_onset_index(1, 1, 1, -1, 16, 1, 1, 0.01, 1, 0) == E_SIZE
    assert lib.ira_onset_index(1, 1, 1, 70000, 16, 1, 1, 0.01, 1, 0) == E_SIZE
    assert lib.ira_onset_index(1, 1, 1, 1, -1, 1, 1, 0.01, 1, 0) == E_SIZE
    assert lib.ira_onset_index(1, 1, 1, 0, 16, 1, 1, 0.01, 1, 0) == 0                # empty batch: nothing to do
    # ira_energy_windows(x, base_off, base_len, chan, onset, nseg, max_len, limits, nlim, scratch, out, stream)
    ok = [1, 1, 1, 1, 1, 1, 16, 1, 2, 1, 1, 0]
    for i in (0, 1, 2, 3, 4, 7, 9, 10):
        args = list(ok)
        args[i] = 0
        assert lib.ira_energy_windows(*args) == E_NULL, i
    for i, v in ((8, 0), (8, 5), (5, -1), (5, 65536), (6, -1), (6, (1 << 31) + 1)):
        args = list(ok)
        args[i] = v
        assert lib.ira_energy_windows(*args) == E_SIZE, (i, v)
    args = list(ok)
    args[5] = 0
    assert lib.ira_energy_windows(*args) == 0
    # scratch: one record of nlim + 2 doubles per (segment, 16384-sample chunk of the longest segment)
    assert lib.ira_energy_scratch_doubles(3, 16384 * 2 + 1, 2) == 3 * 3 * 4
    assert lib.ira_energy_scratch_doubles(1, 16384, 4) == 6
    assert lib.ira_energy_scratch_doubles(5, 0, 1) == 0
    assert lib.ira_energy_scratch_doubles(1, 100, 0) == E_SIZE
    assert lib.ira_energy_scratch_doubles(1, 100, 5) == E_SIZE
    assert lib.ira_energy_scratch_doubles(-1, 100, 2) == E_SIZE
