"""
CPU-only tests of the ISO 3382-1 inter-channel cross-correlation (audio_analysis_amd.analyse.iacc): lag and window
counts, settings validation, the host arithmetic on hand-built sums, the fixed text / Markdown / JSON formats on hand-built
results, the command line's parser, and the argument checks of the two new C entry points (they return before touching a
device).
"""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent


def test_lag_and_window_counts_at_common_rates():
    from audio_analysis_amd.analyse.energy import window_samples
    from audio_analysis_amd.analyse.iacc import IaccSettings, max_lag_samples
    st = IaccSettings()
    assert [max_lag_samples(st.max_lag_ms, fs) for fs in (22050, 44100, 48000, 96000)] == [22, 44, 48, 96]   # 22.05 -> 22
    assert [window_samples(st.early_limits_ms, fs) for fs in (22050, 44100, 48000, 96000)] == [[1764], [3528], [3840], [7680]]
    for fs in (22050, 44100, 48000, 96000):
        for ms in (0.5, 1.0, 1.3, 2.0):
            assert max_lag_samples(ms, fs) == math.floor(ms * fs / 1000.0)
    assert max_lag_samples(1.3, 44100) == 57                              # 57.33
    assert max_lag_samples(0.01, 48000) == 0 and max_lag_samples(3.0, 48000) == 144      # outside 1 .. 128: refused later


def test_settings_defaults_and_validation():
    from audio_analysis_amd.analyse.iacc import IaccSettings
    from audio_analysis_amd.analyse.rt60bands import Rt60BandsAnalysisSettings
    s = IaccSettings()
    assert s.onset_db == -20.0 and s.early_limits_ms == (80.0,) and s.max_lag_ms == 1.0 and s.bands.band_mode == "octave"
    assert s.rel_energy == 10.0 ** (-20.0 / 10.0) and s.is_octave_bank
    assert IaccSettings(early_limits_ms=[50, 80]).early_limits_ms == (50.0, 80.0)
    assert IaccSettings(bands=None).bands is None and not IaccSettings(bands=None).is_octave_bank
    assert not IaccSettings(bands=Rt60BandsAnalysisSettings(band_mode="third")).is_octave_bank
    for bad, what in [(dict(early_limits_ms=(80.0, 50.0)), "ascending"),
                      (dict(early_limits_ms=(50.0, 50.0)), "ascending"),
                      (dict(early_limits_ms=()), "1 to 4"),
                      (dict(early_limits_ms=(10.0, 20.0, 30.0, 40.0, 50.0)), "1 to 4"),
                      (dict(early_limits_ms=(0.0, 50.0)), "positive"),
                      (dict(early_limits_ms=(float("nan"),)), "positive"),
                      (dict(onset_db=3.0), "onset_db"),
                      (dict(onset_db=float("nan")), "onset_db"),
                      (dict(max_lag_ms=0.0), "max_lag_ms"),
                      (dict(max_lag_ms=-1.0), "max_lag_ms"),
                      (dict(max_lag_ms=float("inf")), "max_lag_ms"),
                      (dict(max_lag_ms="wide"), "max_lag_ms"),
                      (dict(bands=Rt60BandsAnalysisSettings(band_mode="sixth")), "band_mode")]:
        with pytest.raises(ValueError, match=what):
            IaccSettings(**bad)


def test_iacc_from_sums_definitions():
    from audio_analysis_amd.analyse.iacc import iacc_from_sums
    # T = 2: a record is C(-2), C(-1), C(0), C(1), C(2), El, Er; three partitions (two limits)
    p0 = [0.0, 1.0, -3.0, 3.0, 0.0, 4.0, 4.0]
    p1 = [0.0, 0.0, 1.0, 0.0, 0.5, 1.0, 1.0]
    p2 = [0.25, 0.0, 0.0, 0.0, -2.0, 4.0, 1.0]
    v = iacc_from_sums(np.array([p0, p1, p2]))
    # limit 1: early = P0, late = P1 + P2; limit 2: early = P0 + P1, late = P2; whole = P0 + P1 + P2
    assert v["early"][0] == 3.0 / math.sqrt(16.0) and v["tau_early"][0] == 0.0      # |-3| at tau 0 ties |3| at tau 1: first
    assert v["late"][0] == 1.5 / math.sqrt(5.0 * 2.0) and v["tau_late"][0] == 2.0
    assert v["early"][1] == 3.0 / math.sqrt(5.0 * 5.0) and v["tau_early"][1] == 1.0  # C(0) = -2, C(1) = 3
    assert v["late"][1] == 2.0 / math.sqrt(4.0) and v["tau_late"][1] == 2.0
    assert v["whole"] == 3.0 / math.sqrt(9.0 * 6.0) and v["tau_whole"] == 1.0
    # partitions are added in ascending order: (P0 + P1) + P2, not P0 + (P1 + P2)
    a, b, c = 1.0, 2.0 ** -53, 2.0 ** -53
    assert (a + b) + c != a + (b + c)
    rec = lambda x: [0.0, 0.0, x, 0.0, 0.0, 1.0, 1.0]                     # noqa: E731
    w = iacc_from_sums(np.array([rec(a), rec(b), rec(c)]))
    assert w["whole"] == ((a + b) + c) / math.sqrt(3.0 * 3.0)
    assert w["late"][0] == (b + c) / math.sqrt(2.0 * 2.0)
    # zero or non-finite El * Er: NaN coefficient and lag for that cell only
    z = iacc_from_sums(np.array([[[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 3.0], p1],
                                 [[0.0, 1.0, 0.0, 0.0, 0.0, math.inf, 1.0], p1]]))
    assert np.isnan(z["early"]).all() and np.isnan(z["tau_early"]).all()
    assert z["late"][0, 0] == 1.0 and z["tau_late"][0, 0] == 0.0
    assert z["whole"][0] == 1.0 / math.sqrt(1.0 * 4.0) and np.isnan(z["whole"][1]) and np.isnan(z["tau_whole"][1])
    # batch shape: (pairs, rows, partitions, record) in, (pairs, rows, limits) out
    big = iacc_from_sums(np.tile(np.array([p0, p1, p2]), (3, 4, 1, 1)))
    assert big["early"].shape == (3, 4, 2) and big["whole"].shape == (3, 4)
    assert np.array_equal(big["late"][2, 3], v["late"]) and np.array_equal(big["tau_whole"], np.full((3, 4), 1.0))


def test_e3_only_for_the_octave_bank():
    from audio_analysis_amd.analyse import iacc as I
    from audio_analysis_amd.analyse.rt60bands import Rt60BandsAnalysisSettings, _build_band_definitions
    cells = {"250Hz": 0.9, "500Hz": 0.6, "1000Hz": 0.3, "2000Hz": 0.15, "4000Hz": 0.05}
    assert I.iacc_e3(cells, True) == (0.6 + 0.3 + 0.15) / 3.0
    assert math.isnan(I.iacc_e3(cells, False))
    assert math.isnan(I.iacc_e3({"500Hz": 0.6, "1000Hz": 0.3}, True))
    # through iacc_results: one pair, T = 1, the same record in every row but a row-dependent C(0)
    for mode, want_nan in (("octave", False), ("third", True), ("three", True), (None, True)):
        st = I.IaccSettings(bands=None if mode is None else Rt60BandsAnalysisSettings(band_mode=mode))
        bands = _build_band_definitions(st.bands, 48000) if mode else []
        sums = np.zeros((1, 1 + len(bands), 2, 5))
        sums[..., 3:] = 1.0                                               # El = Er = 1 per partition
        for row in range(1 + len(bands)):
            sums[0, row, 0, 1] = 0.1 * row / max(1, len(bands))          # early C(0)
        res = I.IaccSums(bands=bands, length=np.array([10000]), onset=np.array([5]), peak_abs=np.ones((1, 2), np.float32),
                         sums=sums, limits=np.array([3840]), max_lag=1)
        r = I.iacc_results(res, 48000, ["p"], st)[0]
        assert r.status == 0 and r.onset_samples == 5 and r.max_lag_samples == 1
        if want_nan:
            assert math.isnan(r.iacc_e3)
        else:
            three = [r.band_values_by_name[n].early[0] for n in ("500Hz", "1000Hz", "2000Hz")]
            assert r.iacc_e3 == sum(three) / 3.0 and r.iacc_e3 > 0.0


def test_status_flags_from_sums():
    from audio_analysis_amd.analyse import iacc as I
    st = I.IaccSettings(bands=None)
    sums = np.zeros((4, 1, 2, 5))
    sums[..., 3:] = 1.0
    sums[..., 1] = 0.5
    sums[3, 0, 1, 0] = math.nan
    res = I.IaccSums(bands=[], length=np.array([10000, 10000, 3845, 10000]), onset=np.array([0, 0, 5, 0]),
                     peak_abs=np.array([[1, 1], [1, 0], [1, 1], [1, 1]], np.float32), sums=sums, limits=np.array([3840]),
                     max_lag=1)
    out = I.iacc_results(res, 48000, list("abcd"), st)
    assert [r.status for r in out] == [0, I.STATUS_SILENT, I.STATUS_TOO_SHORT, I.STATUS_NON_FINITE]
    assert out[0].broadband.whole == 0.5 and out[0].broadband.tau_whole_seconds == 0.0
    for r in out[1:]:
        assert math.isnan(r.broadband.whole) and math.isnan(r.broadband.early[0]) and math.isnan(r.broadband.tau_late_seconds[0])
    assert I.status_text(0) == "ok" and I.status_text(9) == "9 (silent, not stereo)"


def _hand_built():
    from audio_analysis_amd.analyse.iacc import IaccPairResult, IaccSettings, IaccValues, not_stereo_result
    from audio_analysis_amd.analyse.rt60bands import BandDefinition
    nan = float("nan")
    bands = [BandDefinition("500Hz", 500.0, "bandpass", 353.6, 707.1), BandDefinition("1000Hz", 1000.0, "bandpass", 707.1, 1414.2)]
    ok = IaccPairResult(
        pair_name="hall.wav", sample_rate_hz=48000, early_limits_ms=(50.0, 80.0), max_lag_samples=48, onset_samples=240,
        onset_seconds=0.005, status=0,
        broadband=IaccValues((0.61234, 0.5), (0.2, 0.19996), 0.41, (1.0 / 48000, -3.0 / 48000), (0.0, 0.001), -0.001),
        band_definitions=bands,
        band_values_by_name={"500Hz": IaccValues((0.9, 0.8), (0.7, 0.6), 0.75, (0.0, 0.0), (0.0, 0.0), 0.0),
                             "1000Hz": IaccValues((nan, 0.5), (0.25, nan), 0.3, (nan, 0.0005), (-0.0005, nan), 0.0)},
        iacc_e3=0.4567)
    bad = not_stereo_result("mono.wav", 48000, IaccSettings(bands=None))
    return [ok, bad]


def test_summary_text_format_is_pinned():
    from audio_analysis_amd.analyse.iacc import summarise_iacc_text
    assert summarise_iacc_text(_hand_built()) == (
        "[hall.wav]\n"
        "Onset: 240 samples (5.000 ms)  Max lag: 48 samples  Status: ok\n"
        "Band  IACC_E50  tau_E50_ms  IACC_E80  tau_E80_ms  IACC_L50  tau_L50_ms  IACC_L80  tau_L80_ms  IACC_A  tau_A_ms\n"
        "Broadband  0.612  0.021  0.500  -0.062  0.200  0.000  0.200  1.000  0.410  -1.000\n"
        "500Hz  0.900  0.000  0.800  0.000  0.700  0.000  0.600  0.000  0.750  0.000\n"
        "1000Hz  NA  NA  0.500  0.500  0.250  -0.500  NA  NA  0.300  0.000\n"
        "IACC_E3: 0.457\n"
        "\n"
        "[mono.wav]\n"
        "Onset: 0 samples (0.000 ms)  Max lag: 48 samples  Status: 8 (not stereo)\n"
        "Band  IACC_E80  tau_E80_ms  IACC_L80  tau_L80_ms  IACC_A  tau_A_ms\n"
        "Broadband  NA  NA  NA  NA  NA  NA\n"
        "IACC_E3: NA\n"
        "\n")
    assert summarise_iacc_text([]) == ""


def test_summary_markdown_format_is_pinned():
    from audio_analysis_amd.analyse.iacc import summarise_iacc_markdown
    assert summarise_iacc_markdown(_hand_built()[1:]) == (
        "### mono.wav\n"
        "\n"
        "Onset: 0 samples (0.000 ms). Max lag: 48 samples. Status: 8 (not stereo).\n"
        "\n"
        "| Band | IACC_E80 | tau_E80 (ms) | IACC_L80 | tau_L80 (ms) | IACC_A | tau_A (ms) |\n"
        "|---|---:|---:|---:|---:|---:|---:|\n"
        "| Broadband | NA | NA | NA | NA | NA | NA |\n"
        "\n"
        "IACC_E3: NA\n"
        "\n")
    md = summarise_iacc_markdown(_hand_built())
    assert md.startswith("### hall.wav\n\nOnset: 240 samples (5.000 ms). Max lag: 48 samples. Status: ok.\n\n| Band | IACC_E50 | tau_E50 (ms) |")
    assert "| 1000Hz | NA | NA | 0.500 | 0.500 | 0.250 | -0.500 | NA | NA | 0.300 | 0.000 |\n\nIACC_E3: 0.457\n" in md


def test_json_round_trip_keeps_nan():
    from audio_analysis_amd.analyse.iacc import iacc_results_from_json, iacc_results_to_json, summarise_iacc_text
    res = _hand_built()
    doc = json.loads(json.dumps(iacc_results_to_json(res), allow_nan=False))          # strict JSON: no NaN tokens
    assert doc["iacc"][0]["bands"][1]["early"] == [None, 0.5] and doc["iacc"][0]["bands"][1]["tau_late_seconds"][1] is None
    assert doc["iacc"][1]["broadband"]["whole"] is None and doc["iacc"][1]["iacc_e3"] is None
    back = iacc_results_from_json(doc)
    assert summarise_iacc_text(back) == summarise_iacc_text(res)
    assert back[0].broadband == res[0].broadband and back[0].band_definitions == res[0].band_definitions
    assert back[0].band_values_by_name["500Hz"] == res[0].band_values_by_name["500Hz"] and back[0].iacc_e3 == 0.4567
    assert math.isnan(back[1].broadband.whole) and back[1].status == 8 and back[1].max_lag_samples == 48


def test_cli_parser_defaults_and_help():
    from audio_analysis_amd.analyse import iacc
    p = iacc.build_parser()
    a = p.parse_args(["--input", "a.wav", "b.wav"])
    assert a.input == [Path("a.wav"), Path("b.wav")] and a.bundle is None
    assert (a.bands, a.onset_db, a.limits_ms, a.max_lag_ms, a.expected_sample_rate, a.json) == \
        ("octave", -20.0, [80.0], 1.0, 48000, None)
    s = iacc.settings_from_args(a)
    assert s == iacc.IaccSettings()
    a = p.parse_args(["--bundle", "d", "--bands", "none", "--onset-db", "-40", "--limits-ms", "50", "80", "--max-lag-ms", "0.5",
                      "--expected-sample-rate", "44100", "--json", "o.json"])
    assert a.bundle == Path("d") and a.bands == "none" and a.onset_db == -40.0 and a.limits_ms == [50.0, 80.0]
    assert a.max_lag_ms == 0.5 and a.expected_sample_rate == 44100 and a.json == Path("o.json")
    assert iacc.settings_from_args(a).bands is None
    for bad in ([], ["--input", "a.wav", "--bundle", "d"], ["--input", "a.wav", "--bands", "sixth"], ["--input", "a.wav", "--mono"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit):                                       # invalid settings end as a usage error
        iacc.main(["--input", "a.wav", "--limits-ms", "80", "50"])
    with pytest.raises(SystemExit):                                       # 144 lags at 48 kHz: more than the kernel takes
        iacc.main(["--input", "a.wav", "--max-lag-ms", "3"])
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.iacc", "--help"], capture_output=True, text=True, cwd=str(REPO),
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--input", "--bundle", "--bands", "--onset-db", "--limits-ms", "--max-lag-ms", "--expected-sample-rate", "--json"):
        assert flag in r.stdout


def test_shim_re_exports_the_module():
    import analyse.iacc as shim
    from audio_analysis_amd.analyse import iacc
    assert shim is iacc


def test_xcorr_entry_points_validate_arguments_without_gpu():
    from audio_analysis_amd import _lib
    lib = _lib.load()
    E_NULL, E_SIZE = -1, -2
    # ira_xcorr_windows(x, l_off, r_off, len, lchan, rchan, onset, nseg, max_len, limits, nlim, max_lag, scratch, out, stream)
    ok = [1, 1, 1, 1, 1, 1, 1, 1, 16, 1, 2, 48, 1, 1, 0]
    for i in (0, 1, 2, 3, 4, 5, 6, 9, 12, 13):
        args = list(ok)
        args[i] = 0
        assert lib.ira_xcorr_windows(*args) == E_NULL, i
    for i, v in ((10, 0), (10, 5), (11, 0), (11, 129), (11, -1), (7, -1), (7, 65536), (8, -1), (8, (1 << 31) + 1)):
        args = list(ok)
        args[i] = v
        assert lib.ira_xcorr_windows(*args) == E_SIZE, (i, v)
    args = list(ok)
    args[7] = 0
    assert lib.ira_xcorr_windows(*args) == 0                             # empty batch: nothing to do
    # scratch: 2 T + 3 doubles per (segment, 4096-row chunk of the longest segment), and one more record per limit (a
    # chunk that a limit cuts writes one record per side)
    assert lib.ira_xcorr_scratch_doubles(3, 4096 * 2 + 1, 2, 48) == 3 * (3 + 2) * 99
    assert lib.ira_xcorr_scratch_doubles(1, 4096, 4, 128) == (1 + 4) * 259
    assert lib.ira_xcorr_scratch_doubles(1, 4096, 1, 1) == 2 * 5
    assert lib.ira_xcorr_scratch_doubles(5, 0, 1, 48) == 5 * 99
    assert lib.ira_xcorr_scratch_doubles(0, 100, 1, 48) == 0
    for bad in ((1, 100, 0, 48), (1, 100, 5, 48), (-1, 100, 2, 48), (65536, 100, 2, 48), (1, -1, 2, 48),
                (1, (1 << 31) + 1, 2, 48), (1, 100, 2, 0), (1, 100, 2, 129)):
        assert lib.ira_xcorr_scratch_doubles(*bad) == E_SIZE, bad


def test_iacc_device_is_one_launch_over_every_pair_and_row():
    """The host side of iacc_device on the recording engine: one ira_xcorr_windows call whose job tables hold, per pair, the
    broadband row and then the band rows of both channels, the two channels' indices into the onset array, and the limits."""
    from host_engine import HostEngine
    from audio_analysis_amd.analyse import iacc as I
    from audio_analysis_amd.analyse.rt60bands import Rt60BandsAnalysisSettings
    from audio_analysis_amd.synth import synth_ir
    eng = HostEngine()
    lens = [6000, 6000, 500, 7001, 7001]                                  # channel 2 belongs to no pair
    batch = eng.upload([synth_ir(i, i % 2, n, 48000) for i, n in enumerate(lens)])
    st = I.IaccSettings(early_limits_ms=(50.0, 80.0), bands=Rt60BandsAnalysisSettings(band_mode="three"))
    res = I.iacc_device(eng, batch, [(3, 4), (0, 1)], 48000, st)
    calls = eng.calls("ira_xcorr_windows")
    assert len(calls) == 1 and calls[0][0] == "ira_xcorr_windows[T48]"
    x, l_off, r_off, seg_len, lchan, rchan, onset, nseg, max_len, limits, nlim, max_lag, scratch, out, stream = calls[0][1]
    assert (nseg, max_len, nlim, max_lag) == (8, 7001, 2, 48) and out[:2] == ("empty", 8 * 3 * 99)
    assert list(eng.table(seg_len)[:8]) == [7001] * 4 + [6000] * 4
    assert list(eng.table(lchan)[:8]) == [3] * 4 + [0] * 4 and list(eng.table(rchan)[:8]) == [4] * 4 + [1] * 4
    assert list(eng.table(limits)[:16]) == [2400, 3840] * 8
    lo, ro = eng.table(l_off)[:8], eng.table(r_off)[:8]
    assert ro[0] - lo[0] == 7001 and ro[4] - lo[4] == 6000               # broadband rows: neighbours in the batch
    assert lo[0] - lo[4] == 6000 + 6000 + 500
    assert all(ro[i] - lo[i] == 3 * n for i, n in ((1, 7001), (2, 7001), (3, 7001), (5, 6000), (6, 6000), (7, 6000)))
    assert res.sums.shape == (2, 4, 3, 99) and res.max_lag == 48 and list(res.length) == [7001, 6000]
    assert [b.name for b in res.bands] == ["Low", "Mid", "High"]
    for bad, what in (([(0, 2)], "same length"), ([(0, 5)], "channel indices")):
        with pytest.raises(ValueError, match=what):
            I.iacc_device(eng, batch, bad, 48000, st)
    with pytest.raises(ValueError, match="1 to 128 samples"):
        I.iacc_device(eng, batch, [(0, 1)], 48000, I.IaccSettings(max_lag_ms=3.0))
    with pytest.raises(ValueError, match="1 to 128 samples"):
        I.iacc_device(eng, batch, [(0, 1)], 48000, I.IaccSettings(max_lag_ms=0.01))
