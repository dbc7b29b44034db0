"""
CPU-only tests of the speech transmission index (audio_analysis_amd.analyse.sti): closed forms of the long-double
restatement in sti_ref.py, the host arithmetic against hand values, settings validation, status and rating boundaries, the
fixed text / Markdown / JSON formats, the command line's parser, the argument checks of the two C entry points (they return
before touching a device) and the job tables of sti_device on the recording engine.
"""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import sti_ref as R

REPO = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_unit_impulse_anywhere_gives_m_one_and_sti_one():
    w = R.turns(R.FREQS, 48000)
    for n, pos in ((1, 0), (5000, 0), (5000, 4999), (100003, 77777)):
        x = np.zeros(n, np.float32)
        x[pos] = -0.3
        m = R.mtf(x, w)
        assert np.max(np.abs(m - 1.0)) <= 1e-15, (n, pos)
        assert abs(R.sti([m] * 7)[0] - 1.0) <= 1e-12


def test_restatement_geometric_row_matches_the_finite_geometric_sum():
    for stride, count, fs in ((1, 100, 48000), (1, 100, 1000), (997, 100, 48000), (16385, 40, 44100)):
        x, a = R.geometric_row(stride, count)
        assert np.all(x[::stride].astype(np.float64) ** 2 == a ** np.arange(count))       # the squares are exactly a^j
        w = R.turns(R.FREQS, fs)
        got = R.mtf(x, w)
        want = R.geometric_m(a, stride, count, w)
        assert np.max(np.abs(got - want)) <= 1e-12, (stride, count, fs, got, want)
    assert R.geometric_m(0.25, 997, 100, R.turns(R.FREQS, 48000)).min() < 0.75            # the modulation is really reduced


# ------------------------------------------------------------------------------------------------ host arithmetic
def test_weights_sum_to_one():
    from audio_analysis_amd.analyse import sti as S
    assert abs(sum(S.ALPHA) - sum(S.BETA) - 1.0) <= 1e-15
    assert S.ALPHA == R.ALPHA and S.BETA == R.BETA and S.RECEPTION_THRESHOLD_DB == R.A_RT
    assert S.MODULATION_FREQUENCIES_HZ == R.FREQS and len(S.MODULATION_FREQUENCIES_HZ) == 14
    assert S.MAX_MODULATION_FREQUENCIES == 16 and S.MTF_CHUNK == 16384
    hdr = (REPO / "include" / "ira.h").read_text()
    assert "#define IRA_MTF_MAX_FREQS 16" in hdr and "#define IRA_MTF_CHUNK 16384" in hdr


def test_mtf_from_sums_and_index_arithmetic_hand_values():
    from audio_analysis_amd.analyse import sti as S
    sums = np.array([[2.0, 0.6, 0.8, -2.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0]])
    m = S.mtf_from_sums(sums)
    assert m.shape == (2, 2) and m[0, 0] == 0.5 and m[0, 1] == 1.0 and np.isnan(m[1]).all()
    # m = 0.5 everywhere: SNR_eff = 0, TI = 0.5, MTI = 0.5, STI = 0.5 (sum alpha - sum beta)
    sti, mti = S.sti_from_mtf(np.full((7, 14), 0.5))
    assert abs(sti - 0.5) <= 1e-15 and np.all(mti == 0.5)
    sti, mti = S.sti_from_mtf(np.ones((3, 7, 14)))
    assert sti.shape == (3,) and np.all(np.abs(sti - 1.0) <= 1e-15) and np.all(mti == 1.0)
    # clipping: 10 log10(m / (1 - m)) = +-15 dB at m = 1 / (1 + 10^-+1.5)
    hi, lo = 1.0 / (1.0 + 10.0 ** -1.5), 1.0 / (1.0 + 10.0 ** 1.5)
    ti = S.transmission_index(np.array([1.0, 1.5, 0.0, -0.2, hi + 1e-6, lo - 1e-6, 0.5, 0.999999, 1e-9]))
    assert list(ti[:4]) == [1.0, 1.0, 0.0, 0.0] and ti[4] == 1.0 and ti[5] == 0.0 and ti[6] == 0.5
    assert ti[7] == 1.0 and ti[8] == 0.0
    mid = 1.0 / (1.0 + 10.0 ** -0.6)                                      # +6 dB -> TI = 21 / 30
    assert abs(S.transmission_index(np.array([mid]))[0] - 0.7) <= 1e-15
    assert np.isnan(S.transmission_index(np.array([np.nan]))[0])
    # against the restatement on a random matrix
    rng = np.random.default_rng(5)
    m = rng.uniform(-0.1, 1.1, (4, 7, 14))
    sti, mti = S.sti_from_mtf(m)
    for i in range(4):
        s, t = R.sti(m[i])
        assert abs(sti[i] - s) <= 1e-14 and np.max(np.abs(mti[i] - np.array(t))) <= 1e-14


def test_noise_factor_and_masking_slopes():
    from audio_analysis_amd.analyse import sti as S
    m = np.full((7, 14), 0.8)
    out = S.apply_noise_and_levels(m, snr_db=[0.0] * 7)
    assert np.all(out == 0.4)                                             # 1 / (1 + 10^0)
    out = S.apply_noise_and_levels(m, snr_db=[10.0, 0.0, -10.0, 20.0, 3.0, 3.0, 3.0])
    assert abs(out[0, 0] - 0.8 / 1.1) <= 1e-16 and abs(out[2, 3] - 0.8 / 11.0) <= 1e-16 and abs(out[3, 0] - 0.8 / 1.01) <= 1e-16
    assert np.array_equal(S.apply_noise_and_levels(m), m)
    # the slopes on both sides of 63, 67 and 100 dB (the pieces do not meet exactly: the table is the standard's)
    for lv, want in ((62.0, -34.0), (63.0, -33.5), (66.0, -28.1), (67.0, -26.3), (99.0, -10.3), (100.0, -10.0),
                     (120.0, -10.0), (40.0, -45.0)):
        assert abs(S.masking_slope_db(lv) - want) <= 1e-12, lv
        assert abs(R.masking_db(lv) - want) <= 1e-12, lv
    # the level factor by hand: band 0 has no masker; band 1 is masked by band 0
    lev = [70.0, 60.0, 62.9, 63.0, 66.9, 67.0, 100.0]
    f = S.level_factors(lev)
    assert abs(f[0] - 1e7 / (1e7 + 10.0 ** 4.6)) <= 1e-15
    i_am = 1e7 * 10.0 ** ((0.5 * 70.0 - 59.8) / 10.0)
    assert abs(f[1] - 1e6 / (1e6 + i_am + 10.0 ** 2.7)) <= 1e-15
    i_am = 10.0 ** 6.29 * 10.0 ** ((0.5 * 62.9 - 65.0) / 10.0)            # the masker of band 3 sits just below 63 dB
    assert abs(f[3] - 10.0 ** 6.3 / (10.0 ** 6.3 + i_am + 10.0 ** 0.65)) <= 1e-15
    # noise first, levels second, against the restatement
    rng = np.random.default_rng(6)
    m = rng.uniform(0.0, 1.0, (7, 14))
    snr = [3.0, 6.0, 9.0, 12.0, 15.0, 18.0, 21.0]
    got = S.apply_noise_and_levels(m, snr, lev)
    assert np.max(np.abs(got - R.adjust(m, snr, lev))) <= 1e-15
    assert np.max(np.abs(S.apply_noise_and_levels(m, None, lev) - R.adjust(m, None, lev))) <= 1e-15
    assert np.all(got < m)


# ------------------------------------------------------------------------------------------------ surface
def test_settings_defaults_and_validation():
    from audio_analysis_amd.analyse.sti import StiSettings
    s = StiSettings()
    assert s.modulation_frequencies_hz == R.FREQS and s.snr_db is None and s.band_levels_db is None
    assert not s.use_mono_downmix_for_stereo
    assert (s.bands.band_mode, s.bands.f_min_hz, s.bands.f_max_hz) == ("octave", 125.0, 8000.0)
    assert StiSettings(snr_db=12).snr_db == (12.0,) * 7
    assert StiSettings(snr_db=[12.5]).snr_db == (12.5,) * 7
    assert StiSettings(snr_db=range(7)).snr_db == tuple(float(v) for v in range(7))
    assert StiSettings(band_levels_db=[60] * 7).band_levels_db == (60.0,) * 7
    assert StiSettings(modulation_frequencies_hz=[1, 2]).modulation_frequencies_hz == (1.0, 2.0)
    for bad, what in [(dict(modulation_frequencies_hz=()), "1 to 16"),
                      (dict(modulation_frequencies_hz=[1.0] * 17), "1 to 16"),
                      (dict(modulation_frequencies_hz=[0.0]), "positive"),
                      (dict(modulation_frequencies_hz=[float("nan")]), "positive"),
                      (dict(modulation_frequencies_hz=3.0), "sequence"),
                      (dict(snr_db=[1.0, 2.0]), "one value or 7"),
                      (dict(snr_db=float("inf")), "finite"),
                      (dict(band_levels_db=[60.0] * 6), "7 values"),
                      (dict(band_levels_db=[float("nan")] * 7), "finite")]:
        with pytest.raises(ValueError, match=what):
            StiSettings(**bad)


def test_rating_boundaries_and_status_words():
    from audio_analysis_amd.analyse import sti as S
    below = lambda v: math.nextafter(v, 0.0)
    assert [S.rating_word(v) for v in (0.0, below(0.30), 0.30, below(0.45), 0.45, below(0.60), 0.60, below(0.75), 0.75,
                                       1.0)] == \
        ["bad", "bad", "poor", "poor", "fair", "fair", "good", "good", "excellent", "excellent"]
    assert S.rating_word(float("nan")) == "NA"
    assert S.status_text(0) == "ok" and S.status_text(5) == "5 (silent, short)" and S.status_text(2) == "2 (non-finite)"


def test_status_rules_on_hand_built_sums():
    from audio_analysis_amd.analyse import sti as S
    nf = 14
    good = np.zeros((7, 2 * nf + 1))
    good[:, 0] = 2.0
    good[:, 1::2] = 1.0                                                   # m = 0.5 everywhere
    silent = np.zeros_like(good)
    hole = good.copy()
    hole[3] = 0.0                                                         # one empty band
    nan = good.copy()
    nan[5, 4] = np.nan
    inf = good.copy()
    inf[0, 0] = np.inf
    fs = 48000
    one_period = math.ceil(fs / 0.63)
    sums = S.StiSums(band_names=list(S.BAND_NAMES), sums=np.stack([good, silent, hole, nan, inf, good, good]),
                     length=np.array([fs * 2, fs * 2, fs * 2, fs * 2, fs * 2, one_period - 1, one_period], dtype=np.int64))
    res = S.sti_results(sums, fs, list("abcdefg"), S.StiSettings())
    assert [r.status for r in res] == [0, 1, 1, 2, 2, 4, 0]
    for r in (res[0], res[5], res[6]):
        assert abs(r.sti - 0.5) <= 1e-15 and r.rating == "fair" and all(v == 0.5 for v in r.mti)
        assert len(r.mtf) == 7 and all(len(row) == 14 and all(v == 0.5 for v in row) for row in r.mtf)
    for r in res[1:5]:
        assert math.isnan(r.sti) and r.rating == "NA" and all(math.isnan(v) for v in r.mti)
        assert all(math.isnan(v) for row in r.mtf for v in row)
    noisy = S.sti_results(sums, fs, list("abcdefg"), S.StiSettings(snr_db=0.0))[0]
    assert all(v == 0.25 for row in noisy.mtf for v in row)
    assert abs(noisy.sti - R.sti(np.full((7, 14), 0.25))[0]) <= 1e-15 and noisy.rating == "poor"


def _hand_built():
    from audio_analysis_amd.analyse.sti import StiChannelResult
    nan = float("nan")
    names = ("125Hz", "250Hz")
    ok = StiChannelResult(channel_name="left", sample_rate_hz=48000, status=4, sti=0.61234, rating="good",
                          band_names=names, modulation_frequencies_hz=(0.63, 12.5), mti=(0.5, 0.70049),
                          mtf=((0.91239, 0.25), (1.0, 0.0004)))
    bad = StiChannelResult(channel_name="right", sample_rate_hz=44100, status=1, sti=nan, rating="NA", band_names=names,
                           modulation_frequencies_hz=(1.0,), mti=(nan, nan), mtf=((nan,), (nan,)))
    return [ok, bad]


def test_summary_text_and_markdown_formats_are_pinned():
    from audio_analysis_amd.analyse.sti import summarise_sti_markdown, summarise_sti_text
    assert summarise_sti_text(_hand_built()) == (
        "[left]\n"
        "STI: 0.612 (good)  Status: 4 (short)\n"
        "Band  MTI  0.63Hz  12.5Hz\n"
        "125Hz  0.500  0.912  0.250\n"
        "250Hz  0.700  1.000  0.000\n"
        "\n"
        "[right]\n"
        "STI: NA (NA)  Status: 1 (silent)\n"
        "Band  MTI  1Hz\n"
        "125Hz  NA  NA\n"
        "250Hz  NA  NA\n"
        "\n")
    assert summarise_sti_text([]) == ""
    assert summarise_sti_markdown(_hand_built()) == (
        "### left\n"
        "\n"
        "STI: 0.612 (good). Status: 4 (short).\n"
        "\n"
        "| Band | MTI | 0.63Hz | 12.5Hz |\n"
        "|---|---:|---:|---:|\n"
        "| 125Hz | 0.500 | 0.912 | 0.250 |\n"
        "| 250Hz | 0.700 | 1.000 | 0.000 |\n"
        "\n"
        "### right\n"
        "\n"
        "STI: NA (NA). Status: 1 (silent).\n"
        "\n"
        "| Band | MTI | 1Hz |\n"
        "|---|---:|---:|\n"
        "| 125Hz | NA | NA |\n"
        "| 250Hz | NA | NA |\n"
        "\n")


def test_json_round_trip_keeps_nan():
    from audio_analysis_amd.analyse.sti import sti_results_from_json, sti_results_to_json, summarise_sti_text
    res = _hand_built()
    doc = json.loads(json.dumps(sti_results_to_json(res), allow_nan=False))     # strict JSON: no NaN tokens
    assert doc["sti"][1]["sti"] is None and doc["sti"][1]["bands"][0]["mtf"] == [None]
    assert doc["sti"][0]["bands"][1] == {"name": "250Hz", "mti": 0.70049, "mtf": [1.0, 0.0004]}
    back = sti_results_from_json(doc)
    assert back[0] == res[0]
    assert summarise_sti_text(back) == summarise_sti_text(res)
    assert math.isnan(back[1].sti) and back[1].status == 1 and back[1].rating == "NA"


def test_cli_parser_defaults_and_help():
    from audio_analysis_amd.analyse import sti
    p = sti.build_parser()
    a = p.parse_args(["--input", "a.wav", "b.wav"])
    assert a.input == [Path("a.wav"), Path("b.wav")] and a.bundle is None
    assert (a.mono, a.snr_db, a.levels_db, a.expected_sample_rate, a.json) == (False, None, None, 48000, None)
    assert sti.settings_from_args(a) == sti.StiSettings()
    a = p.parse_args(["--bundle", "d", "--mono", "--snr-db", "12", "--levels-db", "60", "61", "62", "63", "64", "65", "66",
                      "--expected-sample-rate", "44100", "--json", "o.json"])
    s = sti.settings_from_args(a)
    assert a.bundle == Path("d") and a.expected_sample_rate == 44100 and a.json == Path("o.json")
    assert s.use_mono_downmix_for_stereo and s.snr_db == (12.0,) * 7
    assert s.band_levels_db == (60.0, 61.0, 62.0, 63.0, 64.0, 65.0, 66.0)
    for bad in ([], ["--input", "a.wav", "--bundle", "d"], ["--input", "a.wav", "--levels-db", "60", "61"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit):                                       # invalid settings end as a usage error
        sti.main(["--input", "a.wav", "--snr-db", "1", "2"])
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.sti", "--help"], capture_output=True, text=True, cwd=str(REPO),
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--input", "--bundle", "--mono", "--snr-db", "--levels-db", "--expected-sample-rate", "--json"):
        assert flag in r.stdout


def test_shim_re_exports_the_module():
    import analyse.sti as shim
    from audio_analysis_amd.analyse import sti
    assert shim is sti


# ------------------------------------------------------------------------------------------------ C entries
def test_mtf_entry_points_validate_arguments_without_gpu():
    from audio_analysis_amd import _lib
    lib = _lib.load()
    E_NULL, E_SIZE = -1, -2
    # ira_mtf_sums(x, off, len, w, nseg, max_len, nf, scratch, out, stream)
    ok = [1, 1, 1, 1, 1, 16, 14, 1, 1, 0]
    for i in (0, 1, 2, 3, 7, 8):
        args = list(ok)
        args[i] = 0
        assert lib.ira_mtf_sums(*args) == E_NULL, i
    for i, v in ((6, 0), (6, 17), (6, -1), (4, -1), (4, 65536), (5, -1), (5, (1 << 31) + 1)):
        args = list(ok)
        args[i] = v
        assert lib.ira_mtf_sums(*args) == E_SIZE, (i, v)
    args = list(ok)
    args[4] = 0
    assert lib.ira_mtf_sums(*args) == 0                                   # empty batch: nothing to do
    # scratch: one record of 2 nf + 1 doubles per (row, 16384-sample chunk of the longest row)
    assert lib.ira_mtf_scratch_doubles(3, 16384 * 2 + 1, 14) == 3 * 3 * 29
    assert lib.ira_mtf_scratch_doubles(1, 16384, 16) == 33
    assert lib.ira_mtf_scratch_doubles(2, 1 << 31, 1) == 2 * 131072 * 3
    assert lib.ira_mtf_scratch_doubles(5, 0, 1) == 0
    for bad in ((1, 100, 0), (1, 100, 17), (-1, 100, 2), (65536, 100, 2), (1, -1, 2), (1, (1 << 31) + 1, 2)):
        assert lib.ira_mtf_scratch_doubles(*bad) == E_SIZE, bad


# ------------------------------------------------------------------------------------------------ recording engine
def test_sti_device_job_tables_on_the_recording_engine():
    from host_engine import HostEngine
    from audio_analysis_amd.analyse import energy as E
    from audio_analysis_amd.analyse import sti as S
    from audio_analysis_amd.synth import synth_ir
    eng = HostEngine()
    lens = [6000, 500, 7001]
    batch = eng.upload([synth_ir(i, 0, n, 48000) for i, n in enumerate(lens)])
    st = S.StiSettings()
    res = S.sti_device(eng, batch, 48000, st)
    calls = eng.calls("ira_mtf_sums")
    assert len(calls) == 1 and calls[0][0] == "ira_mtf_sums"
    x, off, length, w, nseg, max_len, nf, scratch, out, stream = calls[0][1]
    assert (nseg, max_len, nf) == (21, 7001, 14) and out[:2] == ("empty", 21 * 29)
    need = int(eng.lib.ira_mtf_scratch_doubles(21, 7001, 14))             # a host-only entry point: the library answers it
    assert need > 1 and scratch[:2] == ("empty", need)
    assert x[0] == "empty" and x[1] == 7 * sum(lens) and x[-1] == 0       # the band signals' own buffer
    assert list(eng.table(length)[:21]) == [6000] * 7 + [500] * 7 + [7001] * 7
    want_off = np.cumsum(np.repeat(lens, 7)) - np.repeat(lens, 7)
    assert list(eng.table(off)[:21]) == list(want_off)
    wt = eng.table(w)[: 21 * 14].reshape(21, 14)
    assert wt.dtype == np.float64 and all(list(row) == [f / 48000.0 for f in R.FREQS] for row in wt)
    assert res.sums.shape == (3, 7, 29) and list(res.length) == lens and tuple(res.band_names) == S.BAND_NAMES
    # already-built band signals: no second filter bank, the same launch
    sig = E.band_signals_device(eng, batch, 44100, st.bands)
    before = len(eng.calls("ira_band_irfft")) + len(eng.calls("ira_band_irfft_smooth"))
    S.sti_device(eng, batch, 44100, S.StiSettings(modulation_frequencies_hz=(1.0, 2.0)), band_signals=sig)
    assert len(eng.calls("ira_band_irfft")) + len(eng.calls("ira_band_irfft_smooth")) == before
    calls = eng.calls("ira_mtf_sums")
    assert len(calls) == 2 and calls[1][1][4:7] == (21, 7001, 2)
    assert list(eng.table(calls[1][1][3])[:4]) == [1.0 / 44100.0, 2.0 / 44100.0] * 2
    # a bank without the seven octaves (8 kHz at this rate is above Nyquist), and frequencies above Nyquist
    with pytest.raises(ValueError, match="seven octave bands"):
        S.sti_device(eng, batch, 8000, st)
    with pytest.raises(ValueError, match="half the sample rate"):
        S.modulation_turns((30.0,), 50)
    with pytest.raises(ValueError, match="0 .. 0.5"):
        eng.mtf_sums(batch.x, batch.off, batch.length, np.full((3, 1), 0.6))
    with pytest.raises(ValueError, match="nseg"):
        eng.mtf_sums(batch.x, batch.off, batch.length, np.zeros((2, 1)))
