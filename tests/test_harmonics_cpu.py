"""
CPU-only tests of the harmonic distortion measure (audio_analysis_amd.analyse.harmonics): settings validation, the lag /
window / band tables on hand-worked cases and against the float64 restatement in harmonics_ref.py, the host arithmetic, the
fixed text / Markdown / JSON formats, the command line's parser, the argument checks of the two C entry points (they return
before touching a device), the call record of harmonic_distortion_device on the recording engine, and the restatement
itself against the analytic distortion of a synthetic sweep.
"""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import harmonics_ref as R

REPO = Path(__file__).resolve().parent.parent

# the small configuration the GPU tests share: 0.5 s sweep 100 Hz .. 20 kHz at 48 kHz, 0.1 s of silence (n_fft = 32768)
FS, T, F1, F2, AMP, TAIL = 48000, 0.5, 100.0, 20000.0, 0.5, 0.1
C2, C3 = 0.03, 0.01


def _settings(**kw):
    from audio_analysis_amd.analyse.harmonics import HarmonicDistortionSettings
    base = dict(sweep_seconds=T, start_frequency_hz=F1, end_frequency_hz=F2, max_harmonic=3, points_per_octave=3)
    base.update(kw)
    return HarmonicDistortionSettings(**base)


# ------------------------------------------------------------------------------------------------ surface
def test_settings_defaults_and_validation():
    from audio_analysis_amd.analyse.harmonics import HarmonicDistortionSettings as S
    s = S()
    assert (s.sweep_seconds, s.start_frequency_hz, s.end_frequency_hz) == (10.0, 20.0, 20000.0)
    assert (s.max_harmonic, s.points_per_octave, s.window_ms, s.guard_samples) == (5, 3, 200.0, 64)
    assert (s.fade_fraction, s.regularization_relative, s.use_mono_downmix_for_stereo) == (0.25, 1e-10, False)
    assert abs(s.sweep_rate_seconds - 10.0 / math.log(1000.0)) <= 1e-15
    assert S(max_harmonic=2).max_harmonic == 2 and S(max_harmonic=10).max_harmonic == 10
    assert S(points_per_octave=48).points_per_octave == 48 and S(fade_fraction=0.5).fade_fraction == 0.5
    for bad, what in [(dict(sweep_seconds=0.0), "sweep_seconds"), (dict(sweep_seconds=float("nan")), "sweep_seconds"),
                      (dict(start_frequency_hz=0.0), "start_frequency_hz"),
                      (dict(start_frequency_hz=20000.0), "start_frequency_hz"),
                      (dict(end_frequency_hz=10.0), "start_frequency_hz"),
                      (dict(max_harmonic=1), "max_harmonic"), (dict(max_harmonic=11), "max_harmonic"),
                      (dict(max_harmonic=2.5), "max_harmonic"),
                      (dict(points_per_octave=0), "points_per_octave"), (dict(points_per_octave=49), "points_per_octave"),
                      (dict(guard_samples=0), "guard_samples"), (dict(window_ms=0.0), "window_ms"),
                      (dict(fade_fraction=0.0), "fade_fraction"), (dict(fade_fraction=0.51), "fade_fraction"),
                      (dict(regularization_relative=-1.0), "regularization_relative")]:
        with pytest.raises(ValueError, match=what):
            S(**bad)
    from audio_analysis_amd.analyse import harmonics as H
    with pytest.raises(ValueError, match="half the sample rate"):          # f2 <= fs / 2 needs the rate: checked by the plan
        H.harmonic_plan(S(), 32000)
    assert H.status_text(0) == "ok" and H.status_text(3) == "3 (silent, too short)" and H.status_text(4) == "4 (non-finite)"
    hdr = (REPO / "include" / "ira.h").read_text()
    assert f"#define IRA_HARMONIC_MAX {H.MAX_HARMONIC}" in hdr


def test_band_tables_hand_worked_cases():
    from audio_analysis_amd.analyse import harmonics as H
    # 256-point spectra at 48 kHz: df = 187.5 Hz
    st = _settings(max_harmonic=2)
    f, lo, cnt = H.band_tables(st, 48000, 256)
    assert f.size == 23 and f[0] == 100.0 and abs(f[22] - 100.0 * 2.0 ** (22 / 3)) <= 1e-9     # floor(3 log2(200)) = 22
    # one-bin fallback: 100 Hz +- a sixth of an octave is 89.1 .. 112.2 Hz = bins 0.475 .. 0.599: ceil > floor, so the
    # nearest bin to 100 / 187.5 = 0.533: bin 1
    assert (lo[0, 0], cnt[0, 0]) == (1, 1)
    # its second harmonic, 178.2 .. 224.5 Hz = bins 0.950 .. 1.197: bin 1, no fallback needed
    assert (lo[1, 0], cnt[1, 0]) == (1, 1)
    # top grid point 16127 Hz: 14367.5 .. 18101.9 Hz = bins 76.63 .. 96.54 -> 77 .. 96
    assert (lo[0, 22], cnt[0, 22]) == (77, 20)
    # second harmonic: valid while 2 f_j 2^(1/6) <= 20 kHz, f_j <= 8909 Hz: j = 19 (8063 Hz) is, j = 20 (10159 Hz) is not
    assert cnt[1, 19] > 0 and (lo[1, 20], cnt[1, 20]) == (0, 0) and not cnt[1, 20:].any()
    assert (lo[1, 19], cnt[1, 19]) == (77, 20)                # 2 x 8063.5 Hz is the band of 16127 Hz
    # a band that ends on the Nyquist bin: f2 = fs / 2 = f1 2^(1/4) exactly, two points per octave, 64-point spectra.
    # The upper edge is bin (fs / 2) / (fs / 64) = 32, the lower 32 / sqrt(2) = 22.63 -> 23 .. 32
    edge = 1000.0 * 2.0 ** 0.25
    st = H.HarmonicDistortionSettings(sweep_seconds=1.0, start_frequency_hz=1000.0, end_frequency_hz=edge, max_harmonic=2,
                                      points_per_octave=2)
    f, lo, cnt = H.band_tables(st, 2.0 * edge, 64)
    assert f.size == 1 and (lo[0, 0], cnt[0, 0]) == (23, 10) and lo[0, 0] + cnt[0, 0] - 1 == 32
    assert (lo[1, 0], cnt[1, 0]) == (0, 0)
    # the restatement on the same cases
    for args, st in (((F1, F2, 48000, 2, 3, 256), _settings(max_harmonic=2)), ((1000.0, edge, 2.0 * edge, 2, 2, 64), st)):
        rf, rlo, rcnt = R.tables(*args)
        f, lo, cnt = H.band_tables(st, args[2], args[5])
        assert np.array_equal(f, rf) and np.array_equal(lo, rlo) and np.array_equal(cnt, rcnt)


def test_plan_matches_the_restatement_and_hand_values():
    from audio_analysis_amd.analyse import harmonics as H
    plan = H.harmonic_plan(_settings(), FS)
    # L fs = 24000 / ln 200 = 4529.74 samples: d = 0, floor(3139.78 + 0.5), floor(4976.43 + 0.5)
    scale = T / math.log(F2 / F1) * FS
    assert list(plan.lags) == [0, math.floor(scale * math.log(2) + 0.5), math.floor(scale * math.log(3) + 0.5)]
    assert list(plan.lags) == [0, 3140, 4976]
    assert plan.search_margin == math.ceil(scale * math.log(4)) + 64 == 6344
    assert plan.window_samples == 1772 and plan.seg == 1836 and plan.fft_size == 2048    # floor(4529.74 ln 1.5) - 64
    for st, fs in ((_settings(), FS), (_settings(max_harmonic=4), FS), (H.HarmonicDistortionSettings(), 48000),
                   (H.HarmonicDistortionSettings(max_harmonic=10, points_per_octave=12, window_ms=50.0, guard_samples=7,
                                                 fade_fraction=0.5), 44100)):
        plan = H.harmonic_plan(st, fs)
        a = (st.sweep_seconds, st.start_frequency_hz, st.end_frequency_hz, fs, st.max_harmonic)
        assert np.array_equal(plan.lags, R.lags(*a))
        assert plan.window_samples == R.window_length(*a, st.guard_samples, st.window_ms)
        assert plan.search_margin == 1000000 - R.search_length(1000000, *a, st.guard_samples)
        assert plan.seg == st.guard_samples + plan.window_samples and plan.fft_size == R.fft_size(plan.seg)
        w = R.window(st.guard_samples, plan.window_samples, st.fade_fraction)
        assert np.array_equal(plan.window, w) and w.dtype == np.float64
        rf, rlo, rcnt = R.tables(st.start_frequency_hz, st.end_frequency_hz, fs, st.max_harmonic, st.points_per_octave,
                                 plan.fft_size)
        assert np.array_equal(plan.frequencies, rf) and np.array_equal(plan.lo, rlo) and np.array_equal(plan.cnt, rcnt)
        assert plan.lo.dtype == np.int32 and int((plan.lo + plan.cnt).max()) <= plan.fft_size // 2 + 1
    # the default window: 200 ms = 9600 samples is shorter than the gap between harmonics 4 and 5, 15506 samples
    plan = H.harmonic_plan(H.HarmonicDistortionSettings(), 48000)
    assert plan.window_samples == 9600 and plan.fft_size == 16384
    w = plan.window
    assert w[0] == 0.5 - 0.5 * math.cos(math.pi * 0.5 / 64) and w[64] == 1.0 and w[plan.seg - 2400 - 1] == 1.0
    assert w[plan.seg - 2400] == 0.5 + 0.5 * math.cos(math.pi * 0.5 / 2400) and 0.0 < w[-1] < 1e-6
    # a sweep too fast for the window: W < 64 -> nothing to launch
    plan = H.harmonic_plan(_settings(sweep_seconds=0.01, max_harmonic=10), FS)
    assert not plan.usable and plan.window is None


def test_distortion_from_powers_hand_values_and_restatement():
    from audio_analysis_amd.analyse import harmonics as H
    e = np.array([[4.0, 1.0, 100.0], [0.04, 0.01, 0.0], [0.01, 0.0, 0.0]])
    cnt = np.array([[3, 3, 3], [2, 2, 0], [1, 0, 0]])
    hd, thd, counted, fund = H.distortion_from_powers(e, cnt)
    assert list(hd[0][:2]) == [0.1, 0.1] and math.isnan(hd[0][2])
    assert hd[1][0] == 0.05 and math.isnan(hd[1][1]) and math.isnan(hd[1][2])
    assert abs(thd[0] - math.sqrt(0.05 / 4.0)) <= 1e-17 and thd[1] == 0.1 and math.isnan(thd[2])
    assert list(counted) == [2, 1, 0] and abs(fund[0] - 10.0 * math.log10(4.0)) <= 1e-15 and fund[2] == 20.0
    rng = np.random.default_rng(3)
    e = rng.uniform(0.1, 2.0, (4, 5, 9))
    cnt = rng.integers(0, 3, (5, 9))
    cnt[0] = 1
    cnt[2:][:, cnt[1] == 0] = 0                               # a harmonic above an invalid one is invalid too
    hd, thd, counted, fund = H.distortion_from_powers(e * (cnt > 0), cnt)
    for c in range(4):
        rhd, rthd, rcounted, rfund = R.results(e[c] * (cnt > 0), cnt)
        assert np.array_equal(hd[c], rhd, equal_nan=True) and np.array_equal(fund[c], rfund, equal_nan=True)
        assert np.allclose(thd[c], rthd, rtol=1e-15, atol=0.0, equal_nan=True) and np.array_equal(counted, rcounted)


def test_status_rules_on_hand_built_sums():
    from audio_analysis_amd.analyse import harmonics as H
    st = _settings()
    plan = H.harmonic_plan(st, FS)
    j = plan.frequencies.size
    good = np.ones((3, j)) * np.array([[1.0], [0.0009], [0.0001]]) * (plan.cnt > 0)
    inf = good.copy()
    inf[0, 4] = np.inf
    sums = H.HarmonicSums(plan, n_fft=np.array([32768, 32768, 6344, 6345, 32768]), peak=np.array([0, 5, 0, 0, 9]),
                          peak_abs=np.array([1.0, 0.0, 1.0, 1.0, 1.0], np.float32),
                          powers=np.stack([good, np.zeros_like(good), good, good, inf]))
    res = H.harmonic_distortion_results(sums, FS, list("abcde"), st)
    assert [r.status for r in res] == [0, 1, 2, 0, 4]         # n_search = n_fft - 6344: 0 is too short, 1 is not
    for r in (res[0], res[3]):
        assert r.hd[0][9] == 0.03 and r.hd[1][9] == 0.01 and abs(r.thd[9] - math.sqrt(0.001)) <= 1e-17
        assert r.harmonics_counted[9] == 2 and r.harmonics_counted[20] == 0 and math.isnan(r.thd[20])
        assert r.fundamental_db[0] == 0.0 and math.isnan(r.fundamental_db[22]) is False
        assert (r.window_samples, r.fft_size, r.sample_rate_hz) == (1772, 2048, FS) and len(r.frequencies_hz) == j
    for r in (res[1], res[2], res[4]):
        assert all(math.isnan(v) for row in r.hd for v in row) and all(math.isnan(v) for v in r.thd + r.fundamental_db)
        assert len(r.hd) == 2 and len(r.thd) == j and r.harmonics_counted == (0,) * j
    assert res[1].peak_sample == 5
    # a plan without a window: every channel is too short
    st = _settings(sweep_seconds=0.01, max_harmonic=10)
    plan = H.harmonic_plan(st, FS)
    sums = H.HarmonicSums(plan, np.array([1 << 20]), np.zeros(1, np.int64), np.zeros(1, np.float32),
                          np.zeros((1, 10, plan.frequencies.size)))
    r, = H.harmonic_distortion_results(sums, FS, ["x"], st)
    assert r.status == 2 and len(r.hd) == 9 and math.isnan(r.thd[0])


def _hand_built():
    from audio_analysis_amd.analyse.harmonics import HarmonicDistortionChannelResult as Res
    nan = float("nan")
    ok = Res(channel_name="rec.wav:left", sample_rate_hz=48000, status=0, peak_sample=3, window_samples=1772, fft_size=2048,
             frequencies_hz=(100.0, 125.99210498948732), fundamental_db=(-3.2149, -60.0),
             hd=((0.03, 0.001), (0.01, nan)), thd=(0.0316227766, 0.0), harmonics_counted=(2, 1))
    bad = Res(channel_name="rec.wav:right", sample_rate_hz=44100, status=1, peak_sample=0, window_samples=1772,
              fft_size=2048, frequencies_hz=(100.0,), fundamental_db=(nan,), hd=((nan,), (nan,)), thd=(nan,),
              harmonics_counted=(0,))
    return [ok, bad]


def test_summary_text_and_markdown_formats_are_pinned():
    from audio_analysis_amd.analyse.harmonics import (summarise_harmonic_distortion_markdown,
                                                      summarise_harmonic_distortion_text)
    assert summarise_harmonic_distortion_text(_hand_built()) == (
        "[rec.wav:left]\n"
        "Peak: sample 3  Window: 1772 samples, 2048-point spectra  Status: ok\n"
        "Hz  H1_dB  HD2_dB  HD3_dB  THD_%\n"
        "100.0  -3.21  -30.46  -40.00  3.1623\n"
        "126.0  -60.00  -60.00  NA  0.0000\n"
        "\n"
        "[rec.wav:right]\n"
        "Peak: sample 0  Window: 1772 samples, 2048-point spectra  Status: 1 (silent)\n"
        "Hz  H1_dB  HD2_dB  HD3_dB  THD_%\n"
        "100.0  NA  NA  NA  NA\n"
        "\n")
    assert summarise_harmonic_distortion_text([]) == ""
    assert summarise_harmonic_distortion_markdown(_hand_built()) == (
        "### rec.wav:left\n"
        "\n"
        "Peak: sample 3. Window: 1772 samples, 2048-point spectra. Status: ok.\n"
        "\n"
        "| Hz | H1 (dB) | HD2 (dB) | HD3 (dB) | THD (%) |\n"
        "|---|---:|---:|---:|---:|\n"
        "| 100.0 | -3.21 | -30.46 | -40.00 | 3.1623 |\n"
        "| 126.0 | -60.00 | -60.00 | NA | 0.0000 |\n"
        "\n"
        "### rec.wav:right\n"
        "\n"
        "Peak: sample 0. Window: 1772 samples, 2048-point spectra. Status: 1 (silent).\n"
        "\n"
        "| Hz | H1 (dB) | HD2 (dB) | HD3 (dB) | THD (%) |\n"
        "|---|---:|---:|---:|---:|\n"
        "| 100.0 | NA | NA | NA | NA |\n"
        "\n")
    # a ratio of exactly 0 is -inf dB
    from audio_analysis_amd.analyse.harmonics import HarmonicDistortionChannelResult as Res
    zero = Res("z", 48000, 0, 0, 64, 128, (100.0,), (0.0,), ((0.0,),), (0.0,), (1,))
    assert summarise_harmonic_distortion_text([zero]).splitlines()[3] == "100.0  0.00  -inf  0.0000"


def test_json_round_trip_keeps_nan():
    from audio_analysis_amd.analyse.harmonics import (harmonic_results_from_json, harmonic_results_to_json,
                                                      summarise_harmonic_distortion_text)
    res = _hand_built()
    doc = json.loads(json.dumps(harmonic_results_to_json(res), allow_nan=False))       # strict JSON: no NaN tokens
    rows = doc["harmonic_distortion"]
    assert rows[0]["points"][1] == {"frequency_hz": 125.99210498948732, "fundamental_db": -60.0, "hd": [0.001, None],
                                    "thd": 0.0, "harmonics_counted": 1}
    assert rows[0]["max_harmonic"] == 3 and rows[1]["points"][0]["thd"] is None and rows[1]["status"] == 1
    back = harmonic_results_from_json(doc)
    assert back[0].hd[0] == res[0].hd[0] and back[0].thd == res[0].thd and back[0].frequencies_hz == res[0].frequencies_hz
    assert math.isnan(back[0].hd[1][1]) and back[0].harmonics_counted == (2, 1) and back[1].sample_rate_hz == 44100
    assert summarise_harmonic_distortion_text(back) == summarise_harmonic_distortion_text(res)


def test_cli_parser_defaults_and_help():
    from audio_analysis_amd.analyse import harmonics as H
    p = H.build_parser()
    a = p.parse_args(["--recorded", "a.wav", "b.wav", "--sweep", "s.wav"])
    assert a.recorded == [Path("a.wav"), Path("b.wav")] and a.sweep == Path("s.wav")
    assert (a.mono, a.expected_sample_rate, a.json) == (False, 48000, None)
    assert H.settings_from_args(a) == H.HarmonicDistortionSettings()
    a = p.parse_args(["--recorded", "a.wav", "--sweep", "s.wav", "--mono", "--sweep-seconds", "0.5", "--f1", "100", "--f2",
                      "18000", "--harmonics", "3", "--points-per-octave", "6", "--window-ms", "50",
                      "--expected-sample-rate", "44100", "--json", "o.json"])
    assert H.settings_from_args(a) == H.HarmonicDistortionSettings(
        sweep_seconds=0.5, start_frequency_hz=100.0, end_frequency_hz=18000.0, max_harmonic=3, points_per_octave=6,
        window_ms=50.0, use_mono_downmix_for_stereo=True)
    assert a.expected_sample_rate == 44100 and a.json == Path("o.json")
    for bad in ([], ["--recorded", "a.wav"], ["--sweep", "s.wav"], ["--recorded", "a.wav", "--sweep", "s.wav", "--harmonics", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit):                                       # invalid settings end as a usage error
        H.main(["--recorded", "a.wav", "--sweep", "s.wav", "--harmonics", "11"])
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.harmonics", "--help"], capture_output=True, text=True, cwd=str(REPO),
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--recorded", "--sweep", "--mono", "--sweep-seconds", "--f1", "--f2", "--harmonics", "--points-per-octave",
                 "--window-ms", "--expected-sample-rate", "--json"):
        assert flag in r.stdout


def test_shim_re_exports_the_module():
    import analyse.harmonics as shim
    from audio_analysis_amd.analyse import harmonics
    assert shim is harmonics


def test_wav_driver_refuses_before_the_engine(tmp_path):
    from scipy.io import wavfile
    from audio_analysis_amd.analyse import harmonics as H
    short = tmp_path / "sweep.wav"
    wavfile.write(str(short), FS, np.zeros(int(T * FS) - 1, np.float32))
    rec = tmp_path / "rec.wav"
    wavfile.write(str(rec), FS, np.zeros(1000, np.float32))
    with pytest.raises(ValueError, match="fewer than the 0.5 s sweep"):
        H.analyse_harmonic_distortion_from_wav_files([rec], short, _settings(), FS)
    with pytest.raises(ValueError, match=r"more than 2\^21 points"):     # 2^21 + 1 samples: checked on the host, first
        H.analyse_harmonic_distortion_batch([np.zeros((1 << 21) + 1, np.float32)], np.zeros(100, np.float32), FS, ["x"],
                                            _settings())
    with pytest.raises(ValueError, match="one name per channel"):
        H.analyse_harmonic_distortion_batch([np.zeros(100, np.float32)], np.zeros(100, np.float32), FS, [], _settings())


# ------------------------------------------------------------------------------------------------ C entries
def test_harmonic_entry_points_validate_arguments_without_gpu():
    from audio_analysis_amd import _lib
    lib = _lib.load()
    E_NULL, E_SIZE = -1, -2
    # ira_harmonic_windows(h, h_off, nfft, peak, lag, window, nch, nharm, guard, seg, out, stream)
    ok = [1, 1, 1, 1, 1, 1, 2, 3, 5, 208, 1, 0]
    for i in (0, 1, 2, 3, 4, 5, 10):
        args = list(ok)
        args[i] = 0
        assert lib.ira_harmonic_windows(*args) == E_NULL, i
    for i, v in ((6, -1), (6, 65536), (6, 21846), (7, 0), (7, 11), (8, 0), (8, 208), (9, 5), (9, (1 << 21) + 1)):
        args = list(ok)
        args[i] = v
        assert lib.ira_harmonic_windows(*args) == E_SIZE, (i, v)
    args = list(ok)
    args[6] = 0
    assert lib.ira_harmonic_windows(*args) == 0                            # empty batch: nothing to do
    # ira_harmonic_band_powers(spec, spec_off, lo, cnt, nrow, nharm, nband, nbins, out, stream)
    ok = [1, 1, 1, 1, 6, 3, 23, 1025, 1, 0]
    for i in (0, 1, 2, 3, 8):
        args = list(ok)
        args[i] = 0
        assert lib.ira_harmonic_band_powers(*args) == E_NULL, i
    for i, v in ((4, -1), (4, 65538), (4, 7), (5, 0), (5, 11), (6, 0), (6, 4097), (7, 0), (7, (1 << 20) + 2)):
        args = list(ok)
        args[i] = v
        assert lib.ira_harmonic_band_powers(*args) == E_SIZE, (i, v)
    args = list(ok)
    args[4] = 0
    assert lib.ira_harmonic_band_powers(*args) == 0


# ------------------------------------------------------------------------------------------------ recording engine
def test_harmonic_device_call_record_on_the_recording_engine():
    from host_engine import HostEngine
    from audio_analysis_amd.analyse import harmonics as H
    eng = HostEngine()
    rng = np.random.default_rng(1)
    lens = [28800, 40000, 9000]
    rec = eng.upload([rng.standard_normal(n).astype(np.float32) for n in lens])
    sw = eng.upload([rng.standard_normal(28800).astype(np.float32)])
    st = _settings()
    res = H.harmonic_distortion_device(eng, rec, [0, 1, 2], sw, [0, 0, 0], FS, st)
    plan = res.plan
    assert list(res.n_fft) == [32768, 65536, 32768] and res.powers.shape == (3, 3, 23)
    calls = eng.calls("ira_harmonic_windows")
    assert len(calls) == 1
    h, h_off, nfft, peak, lag, win, nch, nharm, guard, seg, out, stream = calls[0][1]
    assert (nch, nharm, guard, seg) == (3, 3, 64, 1836) and out[:2] == ("empty", 3 * 3 * 1836) and out[-1] == 0
    assert h[:2] == ("empty", 32768 + 65536 + 32768) and "float32" in h[2]
    assert list(eng.table(h_off)[:3]) == [0, 32768, 32768 + 65536] and list(eng.table(nfft)[:3]) == [32768, 65536, 32768]
    assert list(eng.table(lag)[:3]) == [0, 3140, 4976]
    assert np.array_equal(eng.table(win)[:1836], R.window(64, 1772, 0.25))
    # the peak the windows read is the one the restricted search wrote
    pk, = eng.calls("ira_peak_index")[-1:]
    assert pk[1][5] == peak and list(eng.table(pk[1][2])[:3]) == [32768 - 6344, 65536 - 6344, 32768 - 6344]
    assert pk[1][0] == h and pk[1][4] == 65536 - 6344
    calls = eng.calls("ira_harmonic_band_powers")
    assert len(calls) == 1
    spec, spec_off, lo, cnt, nrow, nharm, nband, nbins, pout, stream = calls[0][1]
    assert (nrow, nharm, nband, nbins) == (9, 3, 23, 1025) and pout[:2] == ("empty", 9 * 23)
    assert spec[:2] == ("empty", 9 * 1025 * 2) and list(eng.table(spec_off)[:9]) == [1025 * r for r in range(9)]
    rf, rlo, rcnt = R.tables(F1, F2, FS, 3, 3, 2048)
    assert np.array_equal(eng.table(lo)[:69].reshape(3, 23), rlo) and np.array_equal(eng.table(cnt)[:69].reshape(3, 23), rcnt)
    # the spectra are those of the rows the windows wrote: every transform of the call reads that buffer
    ffts = [c for c in eng.calls() if c[0].split("[")[0] in ("ira_rfft_any", "ira_rfft_smooth") and c[1][0] == out]
    assert ffts and all(c[1][0] == out for c in ffts)
    # an already-deconvolved response: no second deconvolution, the same two launches
    resp = dict(h=eng.empty(3 * 32768, eng.torch.float32), off=np.arange(3, dtype=np.int64) * 32768,
                n_fft=np.full(3, 32768, np.int32))
    before = len(eng.calls("ira_deconv_divide"))
    H.harmonic_distortion_device(eng, rec, [0, 1, 2], sw, [0, 0, 0], FS, st, response=resp)
    assert len(eng.calls("ira_deconv_divide")) == before
    assert len(eng.calls("ira_harmonic_windows")) == 2 and len(eng.calls("ira_harmonic_band_powers")) == 2
    # a plan without a window launches nothing
    H.harmonic_distortion_device(eng, rec, [0, 1, 2], sw, [0, 0, 0], FS, _settings(sweep_seconds=0.01, max_harmonic=10),
                                 response=resp)
    assert len(eng.calls("ira_harmonic_windows")) == 2
    # the engine's own argument checks
    with pytest.raises(ValueError, match="guard"):
        eng.harmonic_windows(resp["h"], resp["off"], resp["n_fft"], resp["h"], plan.lags, 1836, plan.window)
    with pytest.raises(ValueError, match="inside the half spectrum"):
        eng.harmonic_band_powers(resp["h"], np.zeros(3, np.int64), plan.lo, plan.cnt, 772)     # the top band ends at bin 772
    with pytest.raises(ValueError, match="multiple of K"):
        eng.harmonic_band_powers(resp["h"], np.zeros(4, np.int64), plan.lo, plan.cnt, 1025)
    with pytest.raises(ValueError, match="n_search"):
        eng.harmonic_peaks(resp["h"], resp["off"], np.array([5, 0, 5]))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.fixture(scope="module")
def responses():
    """The float32 responses of the muted and the unmuted test signal, deconvolved in float64."""
    out = {}
    for mute in (True, False):
        x, y = R.test_signal(FS, T, F1, F2, AMP, TAIL, C2, C3, mute=mute)
        out[mute] = R.deconvolve(y, x).astype(np.float32)
    return out


def test_restatement_finds_the_analytic_distortion(responses):
    h = responses[True]
    assert h.size == 32768
    r = R.analyse(h, FS, T, F1, F2, 3, 3)
    assert r["status"] == 0 and (r["W"], r["seg"], r["n_h"]) == (1772, 1836, 2048)
    for k, c in ((2, C2), (3, C3)):
        m = R.flat_range(r["f"], k, F2, 3)
        assert m.sum() >= 8 and r["f"][m][0] == 800.0
        err = np.abs(r["hd"][k - 2][m] / c - 1.0)
        print(f"HD{k}: {m.sum()} points, largest relative error {err.max():.2e}")
        assert err.max() <= 0.01
    assert np.allclose(r["thd"][R.flat_range(r["f"], 3, F2, 3)], math.hypot(C2, C3), rtol=0.01)
    # a harmonic the signal does not contain
    r = R.analyse(h, FS, T, F1, F2, 4, 3)
    m = R.flat_range(r["f"], 4, F2, 3)
    assert r["status"] == 0 and m.sum() >= 6
    print(f"HD4: {m.sum()} points, largest {r['hd'][2][m].max():.2e}")
    assert r["hd"][2][m].max() < 1e-3
    for k, c in ((2, C2), (3, C3)):
        m = R.flat_range(r["f"], k, F2, 3)
        assert np.abs(r["hd"][k - 2][m] / c - 1.0).max() <= 0.01


def test_restatement_restricted_search_finds_the_linear_peak_of_the_unmuted_signal(responses):
    h = responses[False]
    r = R.analyse(h, FS, T, F1, F2, 3, 3)
    assert int(np.argmax(np.abs(h))) >= r["n_search"]          # the largest sample lies in the harmonic region
    assert r["p"] == R.analyse(responses[True], FS, T, F1, F2, 3, 3)["p"] == 0
    for k, c in ((2, C2), (3, C3)):
        m = R.flat_range(r["f"], k, F2, 3)
        assert np.abs(r["hd"][k - 2][m] / c - 1.0).max() <= 0.01


def test_restatement_status_rules():
    rng = np.random.default_rng(2)
    h = rng.standard_normal(32768).astype(np.float32)
    assert R.analyse(np.zeros(32768, np.float32), FS, T, F1, F2, 3, 3)["status"] == R.STATUS_SILENT
    assert R.analyse(h[:4096], FS, T, F1, F2, 3, 3)["status"] == R.STATUS_TOO_SHORT          # n_search = 4096 - 6344
    assert R.analyse(h, FS, 0.01, F1, F2, 10, 3)["status"] == R.STATUS_TOO_SHORT              # W < 64
    assert R.analyse(h, FS, T, F1, F2, 3, 3)["status"] == 0
