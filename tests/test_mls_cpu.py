"""
CPU-only tests of the MLS measurement (audio_analysis_amd.analyse.mls, engine_geometry's MLS part): the sequences and the
tables of every order, the restatement of tests/mls_ref.py (the fast chain against the direct long-double sums and, for
PCM16-grid input, bit for bit against int64), the module's settings, period rules, formats, parsers and shim, the host side
of the device functions on the recording engine, the header's constants and symbols, and the argument checks of the three
C entry points (they return before touching a device).
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

import mls_ref as R

REPO = Path(__file__).resolve().parent.parent
FS = 48000
ORDERS = list(range(2, 22))


# ------------------------------------------------------------------------------------------------ sequences and tables
def test_default_taps_are_the_documented_ones():
    from audio_analysis_amd import engine
    assert engine.MLS_TAPS == R.TAPS and sorted(engine.MLS_TAPS) == ORDERS
    assert (engine.MLS_MIN_ORDER, engine.MLS_MAX_ORDER, engine.MLS_MAX_PERIODS) == (2, 21, 1024)


@pytest.mark.parametrize("order", [m for m in ORDERS if m <= 16])
def test_walking_the_state_gives_the_full_period(order):
    """The state (the last m bits) returns to all ones after exactly 2^m - 1 steps and not before."""
    taps, p = R.TAPS[order], (1 << order) - 1
    mask = (1 << order) - 1
    state, steps = mask, 0                        # bit q of the state: a[n - 1 - q]
    while True:
        new = 0
        for t in taps:
            new ^= (state >> (t - 1)) & 1
        state = ((state << 1) | new) & mask
        steps += 1
        if state == mask:
            break
        assert steps < p, "the state did not return within 2^m - 1 steps"
    assert steps == p


@pytest.mark.parametrize("order", ORDERS)
def test_all_windows_distinct_sum_and_tables(order):
    from audio_analysis_amd.engine import mls_bits, mls_tables
    from audio_analysis_amd.analyse.mls import mls_sequence
    p = (1 << order) - 1
    a = mls_bits(order)
    assert a.dtype == np.uint8 and a.shape == (p,) and np.all(a[:order] == 1)
    ext = np.concatenate([a, a[:order]]).astype(np.int64)
    windows = sum(ext[q : q + p] << q for q in range(order))
    assert np.array_equal(np.sort(windows), np.arange(1, p + 1))           # all P windows of m bits are distinct
    # the sequence obeys the plain recurrence across the wrap as well
    taps = R.TAPS[order]
    n = np.arange(order, p + order)
    acc = np.zeros(p, dtype=np.int64)
    for t in taps:
        acc ^= ext[n - t]
    assert np.array_equal(acc, ext[n])
    s = mls_sequence(order)
    assert s.dtype == np.int8 and set(np.unique(s)) <= {-1, 1} and int(s.sum(dtype=np.int64)) == -1
    g, out = mls_tables(order)
    for tab in (g, out):
        assert tab.dtype == np.int32 and tab.shape == (p,) and not tab.flags.writeable
        assert np.array_equal(np.sort(tab), np.arange(1, p + 1))
    assert mls_tables(order)[0] is g                                        # made once


@pytest.mark.parametrize("order", [5, 8, 12, 13, 16])
def test_doubling_generator_equals_the_plain_recurrence(order):
    from audio_analysis_amd.engine import mls_bits, mls_tables
    assert np.array_equal(mls_bits(order), R.bits(order))
    if order <= 13:
        g, out = mls_tables(order)
        rg, rout = R.tables(order)
        assert np.array_equal(g, rg) and np.array_equal(out, rout)


@pytest.mark.parametrize("order", range(2, 9))
def test_autocorrelation(order):
    from audio_analysis_amd.analyse.mls import mls_sequence
    s = mls_sequence(order).astype(np.int64)
    p = s.size
    for lag in range(p):
        assert int(np.dot(s, np.roll(s, -lag))) == (p if lag == 0 else -1)


def test_custom_taps():
    from audio_analysis_amd.engine import mls_bits, mls_tables, mls_taps
    from audio_analysis_amd.analyse.mls import MlsSettings
    assert mls_taps(4, [3, 4]) == (4, 3) == mls_taps(4)
    g, out = mls_tables(4, (4, 1))                                         # the other primitive trinomial of degree 4
    assert np.array_equal(np.sort(g), np.arange(1, 16)) and not np.array_equal(g, mls_tables(4)[0])
    assert MlsSettings(order=4, taps=[1, 4]).taps == (4, 1)
    assert np.array_equal(mls_bits(4, (4, 1)), R.bits(4, (4, 1)))
    with pytest.raises(ValueError, match="full period"):
        mls_tables(4, (4, 2))                                              # x^4 + x^2 + 1 = (x^2 + x + 1)^2
    with pytest.raises(ValueError, match="full period"):
        MlsSettings(order=6, taps=(6, 3))
    for bad in ((3, 1), (4,), (4, 4, 1), (5, 4), (4, 0), "ab"):
        with pytest.raises(ValueError):
            mls_taps(4, bad)
    for bad in (1, 22, 4.0, True):
        with pytest.raises(ValueError):
            mls_taps(bad)


# ------------------------------------------------------------------------------------------------ the restatement
RESTATED = (2, 3, 4, 7, 10, 12)


@pytest.mark.parametrize("order", RESTATED)
def test_fast_chain_against_direct_long_double(order):
    """Gaussian float32 input: the stage-ordered float64 chain within gamma_(m+2) sum |Y| / (2^m R) of the direct sums."""
    if np.finfo(np.longdouble).eps >= 2.0 ** -60:
        pytest.skip("numpy.longdouble is no wider than float64 here")
    p = (1 << order) - 1
    rng = np.random.default_rng(order)
    s = R.sequence(order)
    for periods in (1, 3):
        b = 5 + p
        x = rng.standard_normal(b + periods * p + 1).astype(np.float32)
        ch = R.fast_chain(x, b, order, periods)
        # the transform holds the correlation where the tables say: c[k] = W[out[k]], sum Y = W[0]
        ref = R.direct_ld(ch["Y"], order, periods)
        err = np.abs(ch["h64"].astype(np.longdouble) - ref)
        bound = R.bound(order, periods, ch["Y"])
        print(f"order {order} R {periods}: worst error {float(err.max()):.3e}, {float(err.max() / bound):.3f} of the bound")
        assert np.all(err <= bound)
        assert abs(ch["W"][0] - ch["Y"].sum()) <= R.gamma(order) * np.abs(ch["Y"]).sum()
        assert s.size == p


@pytest.mark.parametrize("order", RESTATED)
def test_fast_chain_equals_int64_on_the_pcm16_grid(order):
    p = (1 << order) - 1
    rng = np.random.default_rng(100 + order)
    for periods in (1, 2, 3, 5):
        assert order + 16 + math.ceil(math.log2(periods)) <= 53
        b = 3
        x = (rng.integers(-32768, 32768, b + periods * p) / 32768.0).astype(np.float32)
        ch = R.fast_chain(x, b, order, periods)
        h64, h32 = R.grid_int64(x, b, order, periods)
        assert np.array_equal(R.bits_of(ch["h64"]), R.bits_of(h64)) and np.array_equal(R.bits_of(ch["h"]), R.bits_of(h32))


def test_fast_chain_recovers_a_known_response_exactly():
    """Integer data: y = h (*) s circularly gives h back, DC included (orders 2, 3, 5, 9)."""
    rng = np.random.default_rng(9)
    for order in (2, 3, 5, 9):
        p = (1 << order) - 1
        h = rng.integers(-50, 50, p)
        s = R.sequence(order)
        y = np.array([sum(h[j] * s[(n - j) % p] for j in range(p)) for n in range(p)], dtype=np.int64)
        x = (np.tile(y, 2) / 32768.0).astype(np.float32)
        got = R.fast_chain(x, 0, order, 2)["h64"] * 32768.0
        assert np.array_equal(got, h.astype(np.float64))


MEASUREMENT_ORDERS = tuple(range(14, 22))           # 0.3 s to 44 s of sequence at 48 kHz: beyond what direct_ld can afford


@pytest.mark.parametrize("order", MEASUREMENT_ORDERS)
def test_fast_chain_at_sampled_positions_of_the_measurement_orders(order):
    """Gaussian float32 input, R = 2: at k = 0, 1, P - 1 and seeded positions the float64 chain lies within
    gamma_(m+2) sum |Y| / (2^m R) of correctly rounded sums (mls_ref.sampled_ld, O(P) a position).  The tables are the
    engine's (the plain loops of mls_ref.tables take seconds up here); the sequence is checked against the plain recurrence."""
    if np.finfo(np.longdouble).eps >= 2.0 ** -60:
        pytest.skip("numpy.longdouble is no wider than float64 here")
    from audio_analysis_amd.engine import mls_bits, mls_tables
    p, periods = (1 << order) - 1, 2
    a = mls_bits(order)
    assert np.array_equal(a, R.bits(order))
    s = 1 - 2 * a.astype(np.int64)
    x = np.random.default_rng(1000 + order).standard_normal(p + periods * p).astype(np.float32)
    ch = R.fast_chain(x, p, order, periods, tabs=mls_tables(order))
    ks = R.sample_positions(order, order, 16 if order < 19 else 8)
    assert {0, 1, p - 1} <= set(ks) and len(ks) >= 8
    err = np.abs(ch["h64"][ks].astype(np.longdouble) - R.sampled_ld(ch["Y"], s, order, periods, ks))
    bound = R.bound(order, periods, ch["Y"])
    print(f"order {order} R {periods}: worst sampled error {float(err.max()):.3e}, {float(err.max() / bound):.3g} of the bound")
    assert np.all(err <= bound)


def test_sampled_sums_equal_the_direct_sums_where_both_can_run():
    if np.finfo(np.longdouble).eps >= 2.0 ** -60:
        pytest.skip("numpy.longdouble is no wider than float64 here")
    order, periods = 10, 3
    p = (1 << order) - 1
    y = R.fold(np.random.default_rng(5).standard_normal(periods * p).astype(np.float32), 0, p, periods)
    ks = R.sample_positions(order, 1, 12)
    a, b = R.sampled_ld(y, R.sequence(order), order, periods, ks), R.direct_ld(y, order, periods)[ks]
    # direct_ld adds P + 1 terms in long double (2^-64 each); sampled_ld rounds c and sum Y to float64 once (2^-53 each)
    assert np.max(np.abs(a - b)) <= ((p + 2) * 2.0 ** -64 + 2.0 * 2.0 ** -53) * np.abs(y).sum() / ((1 << order) * periods)


@pytest.mark.parametrize("order", (14, 16, 21))
def test_fast_chain_recovers_a_sparse_response_exactly_at_measurement_orders(order):
    """Twelve taps k / 256 under the amplitude-0.5 sequence: every intermediate of the chain is an integer multiple of 2^-9
    below 2^(m + 5), so 0.5 h comes back exactly, zeros included -- a reference that owes nothing to fwht."""
    from audio_analysis_amd.engine import mls_bits, mls_tables
    p, periods = (1 << order) - 1, 2 if order == 21 else 3
    h = R.sparse_response(order, order)
    assert np.count_nonzero(h) == 12 and h[0] != 0.0 and h[p - 1] != 0.0 and np.array_equal(np.rint(h * 256.0), h * 256.0)
    y = R.sparse_period(h, 1 - 2 * mls_bits(order).astype(np.int64))
    assert np.array_equal(np.rint(y * 512.0), y * 512.0) and np.array_equal(y.astype(np.float32).astype(np.float64), y)
    ch = R.fast_chain(np.tile(y.astype(np.float32), periods), 0, order, periods, tabs=mls_tables(order))
    assert np.array_equal(R.bits_of(ch["h64"]), R.bits_of(0.5 * h)) and np.array_equal(R.bits_of(ch["h"]), R.bits_of((0.5 * h).astype(np.float32)))


def test_the_engine_tables_drive_the_restated_chain():
    """engine.mls_tables is what the kernels read: the chain with them equals the chain with the plain-loop tables."""
    from audio_analysis_amd.engine import mls_tables
    rng = np.random.default_rng(4)
    x = rng.standard_normal(4 * 127).astype(np.float32)
    a, b = R.fast_chain(x, 127, 7, 3), R.fast_chain(x, 127, 7, 3, tabs=mls_tables(7))
    assert np.array_equal(R.bits_of(a["h"]), R.bits_of(b["h"]))


# ------------------------------------------------------------------------------------------------ geometry
def test_geometry_of_the_kernels():
    from audio_analysis_amd import engine as E
    assert (E.MLS_TILE_LOG2, E.MLS_FOLD_THREADS, E.MLS_FOLD_BLOCKS) == (12, 256, 128)
    assert [E.mls_fold_blocks(m) for m in (2, 8, 9, 15, 16, 21)] == [1, 1, 2, 128, 128, 128]
    assert E.mls_scratch_bytes(3, 5) == 8 * 3 * (32 + 2) and E.mls_scratch_bytes(64, 21) == 8 * 64 * ((1 << 21) + 256)
    assert E.mls_sum_chain(5, 1) == 1 + 9 + 1 and E.mls_sum_chain(13, 5) == 5 + 9 + 32 and E.mls_sum_chain(21, 4) == 64 * 4 + 9 + 128
    assert E.mls_pass_plan(2) == [(0, 2)] and E.mls_pass_plan(12) == [(0, 12)] and E.mls_pass_plan(13) == [(0, 12), (12, 1)]
    assert E.mls_pass_plan(20) == [(0, 12), (12, 8)] and E.mls_pass_plan(21) == [(0, 12), (12, 5), (17, 4)]
    for m in ORDERS:
        plan = E.mls_pass_plan(m)
        assert sum(a for _, a in plan) == m and all(lo == sum(a for _, a in plan[:i]) for i, (lo, _) in enumerate(plan))
        assert all(1 <= a <= 8 for _, a in plan[1:])


# ------------------------------------------------------------------------------------------------ the module
def test_settings_defaults_and_validation():
    from audio_analysis_amd.analyse.mls import MlsSettings
    s = MlsSettings()
    assert (s.order, s.taps, s.start_samples, s.skip_periods, s.periods, s.use_mono_downmix_for_stereo) == (16, None, 0, 1, None, False)
    assert (s.normalise_peak, s.target_peak, s.remove_dc, s.period_samples) == (True, 0.95, True, 65535)
    assert MlsSettings(order=np.int64(10), periods=np.int32(4)).order == 10
    for bad in (dict(order=1), dict(order=22), dict(order=10.0), dict(order=True), dict(start_samples=-1), dict(skip_periods=-1),
                dict(skip_periods=1.5), dict(periods=0), dict(periods=1025), dict(periods=2.0), dict(target_peak=0.0),
                dict(target_peak=float("nan")), dict(target_peak="x"), dict(order=4, taps=(4, 2))):
        with pytest.raises(ValueError):
            MlsSettings(**bad)


def test_period_rules_and_their_errors():
    from audio_analysis_amd.analyse.mls import MlsSettings, mls_layout, mls_stimulus, period_snr_db
    p = 1023
    st = MlsSettings(order=10)
    b, r = mls_layout([4 * p, 4 * p + 1022, 2 * p], st)
    assert b == p and r.tolist() == [3, 3, 1]
    assert mls_layout([4 * p], MlsSettings(order=10, skip_periods=0, start_samples=7))[1].tolist() == [3]
    assert mls_layout([4 * p + 7], MlsSettings(order=10, skip_periods=0, start_samples=7))[1].tolist() == [4]
    assert mls_layout([9 * p], MlsSettings(order=10, periods=2))[1].tolist() == [2]
    with pytest.raises(ValueError, match="hall.wav:right"):
        mls_layout([4 * p, 2 * p - 1], st, ["hall.wav:left", "hall.wav:right"])            # R < 1
    with pytest.raises(ValueError, match="channel 0"):
        mls_layout([4 * p], MlsSettings(order=10, periods=4))                              # b + R P > L
    with pytest.raises(ValueError, match="channel 1.*1024"):
        mls_layout([5 * 3, 1027 * 3], MlsSettings(order=2))                                # R > 1024
    x = mls_stimulus(5, 3, 0.25)
    assert x.dtype == np.float32 and x.shape == (93,) and set(np.unique(x)) == {-0.25, 0.25} and np.array_equal(x[:31], x[31:62])
    for bad in (dict(periods=0), dict(periods=1.0), dict(amplitude=0.0), dict(amplitude=1.5)):
        with pytest.raises(ValueError):
            mls_stimulus(5, **{"periods": 2, **bad})
    assert math.isnan(period_snr_db(1.0, 0.0, 1)) and period_snr_db(1.0, 0.0, 2) == math.inf
    assert math.isnan(period_snr_db(float("nan"), 1.0, 2)) and period_snr_db(8.0, 0.4, 2) == pytest.approx(10.0)


def _results():
    from audio_analysis_amd.analyse.mls import MlsChannelResult
    return [MlsChannelResult("hall.wav:left", 48000, 10, 1023, 3, 1023, 12, 0.25, 41.256),
            MlsChannelResult("hall.wav:right", 48000, 10, 1023, 1, 1023, 0, math.nan, math.nan),
            MlsChannelResult("mono", 48000, 16, 65535, 2, 65535, 480, 0.5, math.inf)]


def test_text_and_markdown_formats_are_pinned():
    from audio_analysis_amd.analyse.mls import summarise_mls_markdown, summarise_mls_text
    text = summarise_mls_text(_results())
    assert text == ("[hall.wav:left]\n"
                    "Order: 10  Period: 1023 samples (0.0213 s at 48000 Hz)\n"
                    "value  periods  begin_samples  peak_samples  peak_ms  peak_value  period_snr_dB\n"
                    "response  3  1023  12  0.250  0.250000  41.26\n"
                    "\n"
                    "[hall.wav:right]\n"
                    "Order: 10  Period: 1023 samples (0.0213 s at 48000 Hz)\n"
                    "value  periods  begin_samples  peak_samples  peak_ms  peak_value  period_snr_dB\n"
                    "response  1  1023  0  0.000  NA  NA\n"
                    "\n"
                    "[mono]\n"
                    "Order: 16  Period: 65535 samples (1.3653 s at 48000 Hz)\n"
                    "value  periods  begin_samples  peak_samples  peak_ms  peak_value  period_snr_dB\n"
                    "response  2  65535  480  10.000  0.500000  +inf\n"
                    "\n")
    md = summarise_mls_markdown(_results()[:1])
    assert md == ("### hall.wav:left\n\nOrder: 10. Period: 1023 samples (0.0213 s at 48000 Hz).\n\n"
                  "| value | periods | begin (samples) | peak (samples) | peak (ms) | peak value | period SNR (dB) |\n"
                  "|---|---:|---:|---:|---:|---:|---:|\n"
                  "| response | 3 | 1023 | 12 | 0.250 | 0.250000 | 41.26 |\n\n")
    assert summarise_mls_text([]) == ""


def test_json_round_trip_writes_nan_as_null():
    from audio_analysis_amd.analyse.mls import mls_results_from_json, mls_results_to_json
    doc = mls_results_to_json(_results())
    text = json.dumps(doc, allow_nan=False)                                 # plain JSON: no NaN token
    assert doc["mls"][1]["peak_value"] is None and doc["mls"][1]["period_snr_db"] is None
    assert doc["mls"][2]["period_snr_db"] == "+inf"
    back = mls_results_from_json(json.loads(text))
    for a, b in zip(_results(), back):
        for name in a.__dataclass_fields__:
            va, vb = getattr(a, name), getattr(b, name)
            assert (va == vb) or (math.isnan(va) and math.isnan(vb)), name


def test_both_parsers_and_the_shim():
    import analyse.mls as shim
    from audio_analysis_amd.analyse import mls as D
    assert shim is D
    p = D.build_parser()
    a = p.parse_args(["generate", "--periods", "4", "--output", "s.wav"])
    assert (a.command, a.order, a.periods, a.amplitude, a.sample_rate, a.output) == ("generate", 16, 4, 0.5, 48000, Path("s.wav"))
    a = p.parse_args(["generate", "--order", "12", "--periods", "3", "--amplitude", "0.25", "--sample-rate", "44100",
                      "--output", "s.wav"])
    assert (a.order, a.periods, a.amplitude, a.sample_rate) == (12, 3, 0.25, 44100)
    a = p.parse_args(["deconvolve", "--recorded", "a.wav", "b.wav"])
    assert a.command == "deconvolve" and a.recorded == [Path("a.wav"), Path("b.wav")]
    assert (a.output_dir, a.json, a.expected_sample_rate) == (None, None, 48000)
    assert D.settings_from_args(a) == D.MlsSettings()
    a = p.parse_args(["deconvolve", "--recorded", "a.wav", "--order", "14", "--skip-periods", "2", "--periods", "6",
                      "--start-samples", "100", "--mono", "--no-normalise", "--keep-dc", "--output-dir", "out",
                      "--expected-sample-rate", "44100", "--json", "o.json"])
    assert D.settings_from_args(a) == D.MlsSettings(order=14, skip_periods=2, periods=6, start_samples=100,
                                                    use_mono_downmix_for_stereo=True, normalise_peak=False, remove_dc=False)
    assert (a.output_dir, a.json, a.expected_sample_rate) == (Path("out"), Path("o.json"), 44100)
    for bad in ([], ["generate", "--output", "s.wav"], ["generate", "--periods", "4"], ["deconvolve"],
                ["deconvolve", "--recorded", "a.wav", "--order", "2.5"], ["measure"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    for bad in (["deconvolve", "--recorded", "a.wav", "--order", "40"], ["generate", "--order", "1", "--periods", "2", "--output", "s.wav"]):
        with pytest.raises(SystemExit):                                     # invalid settings end as a usage error
            D.main(bad)
    assert D.default_output_ir_path("rec/hall.wav") == Path("rec/hall_ir.wav")
    assert D.default_output_ir_path("rec/hall.wav", "out") == Path("out/hall_ir.wav")
    env = dict(os.environ, PYTHONPATH=str(REPO))
    for sub, flags in (("generate", ("--order", "--periods", "--amplitude", "--sample-rate", "--output")),
                       ("deconvolve", ("--recorded", "--order", "--skip-periods", "--periods", "--start-samples", "--mono",
                                       "--no-normalise", "--keep-dc", "--output-dir", "--expected-sample-rate", "--json"))):
        r = subprocess.run([sys.executable, "-m", "analyse.mls", sub, "--help"], capture_output=True, text=True, cwd=str(REPO),
                           env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        for flag in flags:
            assert flag in r.stdout


def test_generate_writes_the_stimulus(tmp_path):
    from scipy.io import wavfile
    from audio_analysis_amd.analyse import mls as D
    D.main(["generate", "--order", "6", "--periods", "3", "--amplitude", "0.25", "--output", str(tmp_path / "s.wav")])
    fs, s = wavfile.read(str(tmp_path / "s.wav"))
    assert fs == 48000 and s.dtype == np.float32
    assert np.array_equal(np.asarray(s).reshape(-1), np.tile(0.25 * R.sequence(6), 3).astype(np.float32))


# ------------------------------------------------------------------------------------------------ library and engine
NEW_SYMBOLS = ("ira_mls_fold", "ira_mls_hadamard", "ira_mls_finish")


def test_header_constants_symbols_and_abi_version():
    from audio_analysis_amd import _lib, build, engine
    hdr = (REPO / "include" / "ira.h").read_text()
    for name, value in (("MIN_ORDER", engine.MLS_MIN_ORDER), ("MAX_ORDER", engine.MLS_MAX_ORDER),
                        ("MAX_PERIODS", engine.MLS_MAX_PERIODS), ("TILE_LOG2", engine.MLS_TILE_LOG2),
                        ("FOLD_THREADS", engine.MLS_FOLD_THREADS), ("FOLD_BLOCKS", engine.MLS_FOLD_BLOCKS)):
        assert re.search(rf"#define IRA_MLS_{name} {value}\b", hdr), name
    assert build.SOURCES["ira_mls.hip"] == ["-ffp-contract=off"]
    assert "#define IRA_ABI_VERSION 15 " in hdr and _lib.ABI_VERSION == 15
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES and re.search(rf"int32_t {name}\(", hdr)
    declared = set(re.findall(r"\b(ira_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_lib.PROTOTYPES) and len(declared) == 86
    assert "replace no reference function" in hdr[hdr.index("MLS impulse-response measurement"):]
    assert "8 nb (2^m + 2 B)" in hdr                                        # the size formula mls_scratch_bytes restates
    lib = _lib.load()
    assert lib.ira_abi_version() == 15 and all(getattr(lib, name) is not None for name in NEW_SYMBOLS)
    assert not any(name.startswith("ira_mls") and name.endswith("_doubles") for name in _lib.PROTOTYPES)


def test_entry_points_validate_arguments_without_gpu():
    from audio_analysis_amd import _lib
    lib = _lib.load()
    E_NULL, E_SIZE = -1, -2

    def fold(**kw):
        a = dict(x=1, begin=1, nb=0, order=10, periods=4, g=1, w=1, sums=1, scratch=1)
        a.update(kw)
        return lib.ira_mls_fold(a["x"], a["begin"], a["nb"], a["order"], a["periods"], a["g"], a["w"], a["sums"], a["scratch"], 0)

    def hadamard(**kw):
        a = dict(w=1, nb=0, order=10)
        a.update(kw)
        return lib.ira_mls_hadamard(a["w"], a["nb"], a["order"], 0)

    def finish(**kw):
        a = dict(w=1, out=1, nb=0, order=10, periods=4, h=1, h_off=1)
        a.update(kw)
        return lib.ira_mls_finish(a["w"], a["out"], a["nb"], a["order"], a["periods"], a["h"], a["h_off"], 0)

    pointers = {fold: ("x", "begin", "g", "w", "sums", "scratch"), hadamard: ("w",), finish: ("w", "out", "h", "h_off")}
    for fn, names in pointers.items():
        assert fn() == 0                                                    # nb == 0: nothing to do
        for name in names:
            assert fn(**{name: 0}) == E_NULL and fn(nb=3, **{name: 0}) == E_NULL, (fn.__name__, name)
        for kw in (dict(nb=-1), dict(nb=65536), dict(order=1), dict(order=22), dict(order=0), dict(order=-3)):
            assert fn(**kw) == E_SIZE and fn(**{"nb": 2, **kw}) == E_SIZE, (fn.__name__, kw)
        assert fn(order=2) == 0 and fn(order=21) == 0
    for fn in (fold, finish):
        for periods in (0, -1, 1025):
            assert fn(periods=periods) == E_SIZE and fn(nb=2, periods=periods) == E_SIZE, (fn.__name__, periods)
        assert fn(periods=1) == 0 and fn(periods=1024) == 0


def test_device_calls_on_the_recording_engine(monkeypatch):
    """Order, arguments and allocation sizes of the library calls; the tables go up once per order."""
    from host_engine import HostEngine
    from audio_analysis_amd import engine as E
    from audio_analysis_amd.analyse import mls as D
    eng = HostEngine()
    p = 255
    rng = np.random.default_rng(0)
    chans = [rng.standard_normal(n).astype(np.float32) for n in (3 * p, 4 * p + 3, 3 * p + 100)]      # R = 2, 3, 2
    batch = eng.upload(chans)
    before = eng.uploads
    dev = D.mls_device(eng, batch, [0, 0, 1], D.MlsSettings(order=8))
    names = [n for n, _ in eng.calls()]
    assert names == ["ira_mls_fold[8]", "ira_mls_hadamard[8]", "ira_mls_finish[8]"] * 2 + ["ira_peak_index", "ira_deconv_finish"]
    assert dev["periods"].tolist() == [2, 3, 2] and dev["begin"] == p
    assert dev["off"].tolist() == [0, 256, 512] and dev["n_out"].tolist() == [p] * 3 and dev["n_fft"].tolist() == [256] * 3
    assert dev["sums"].shape == (3, 2) and int(dev["h"].numel()) == 3 * 256
    g, out = E.mls_tables(8)
    fold2, fold3 = eng.calls("ira_mls_fold")
    for (_, a), nb, r, begins in ((fold2, 2, 2, [p, batch.off[2] + p]), (fold3, 1, 3, [batch.off[1] + p])):
        assert a[0][:3] == ("up", "<f4", (int(batch.x.numel()),))
        assert eng.table(a[1])[:nb].tolist() == [int(v) for v in begins] and a[2:5] == (nb, 8, r)
        assert np.array_equal(eng.table(a[5])[:p], g)
        assert a[6] == ("empty", nb * 256, "torch.float64", 0) and a[7] == ("empty", nb * 2, "torch.float64", 0)
        assert a[8] == ("empty", 2 * nb * E.mls_fold_blocks(8), "torch.float64", 0)
    for (_, a), (_, f), nb in zip(eng.calls("ira_mls_hadamard"), eng.calls("ira_mls_fold"), (2, 1)):
        assert a[0] == f[6] and a[1:3] == (nb, 8)                          # in place on the fold's workspace
    fin2, fin3 = eng.calls("ira_mls_finish")
    for (_, a), (_, f), nb, r, offs in ((fin2, fold2, 2, 2, [0, 512]), (fin3, fold3, 1, 3, [256])):
        assert a[0] == f[6] and np.array_equal(eng.table(a[1])[:p], out) and a[2:5] == (nb, 8, r)
        assert a[5] == ("empty", 3 * 256, "torch.float32", 0) and eng.table(a[6])[:nb].tolist() == offs
    _, fin = eng.calls("ira_deconv_finish")[0]
    assert fin[0] == ("empty", 3 * 256, "torch.float32", 0) and eng.table(fin[3])[:3].tolist() == [0, 0, 1]
    assert fin[4:10] == (3, 2, p, 1, 1, 0.95)
    # the tables: one upload each for the order, however many chains and calls follow
    tables_up = [d for _, _, d, _ in eng._live if d[0] == "up" and d[1] == "<i4" and d[2] == (p,)]
    assert len(tables_up) == 2
    D.mls_device(eng, batch, [0, 0, 1], D.MlsSettings(order=8, normalise_peak=False, remove_dc=False))
    assert len([d for _, _, d, _ in eng._live if d[0] == "up" and d[1] == "<i4" and d[2] == (p,)]) == 2
    assert eng.calls("ira_deconv_finish")[1][1][7:9] == (0, 0)
    other = HostEngine()
    other.mls_device_tables(8)
    other.mls_device_tables(8, (8, 6, 5, 4))                                # the default taps, spelt out: the same key
    other.mls_device_tables(9)
    assert other.uploads == 4
    # cut by the workspace budget: one channel a chain
    eng2 = HostEngine()
    monkeypatch.setattr(E, "MLS_SCRATCH_BYTES", E.mls_scratch_bytes(1, 8))
    D.mls_device(eng2, eng2.upload(chans), [0, 0, 1], D.MlsSettings(order=8))
    assert [a[2] for _, a in eng2.calls("ira_mls_fold")] == [1, 1, 1]
    assert eng.uploads > before


def test_engine_methods_refuse_bad_arguments():
    from host_engine import HostEngine
    import torch
    eng = HostEngine()
    x = eng.to_dev(np.zeros(4 * 31, np.float32))
    h = eng.empty(64, torch.float32)
    w, sums = eng.mls_fold(x, [0, 31], 5, 3)
    assert tuple(w.shape) == (2, 32) and tuple(sums.shape) == (2, 2)
    for kw in (dict(begin=[32], periods=3), dict(begin=[-1], periods=1), dict(begin=[0], periods=0), dict(begin=[0], periods=1025)):
        with pytest.raises(ValueError):
            eng.mls_fold(x, kw["begin"], 5, kw["periods"])
    for order in (1, 22):
        with pytest.raises(ValueError):
            eng.mls_fold(x, [0], order, 1)
        with pytest.raises(ValueError):
            eng.mls_hadamard(w, 1, order)
    with pytest.raises(ValueError):
        eng.mls_hadamard(w, 3, 5)                                          # the workspace holds two rows
    with pytest.raises(ValueError):
        eng.mls_finish(w, 2, 5, 3, h, [0])                                 # one offset per channel
    with pytest.raises(ValueError):
        eng.mls_finish(w, 2, 5, 3, h, [0, 34])                             # the second response would leave h
    eng.mls_finish(w, 2, 5, 3, h, [0, 33])
    calls = len(eng.calls())
    empty_w, empty_s = eng.mls_fold(x, [], 5, 3)                            # no channel: no launch
    eng.mls_hadamard(empty_w, 0, 5)
    eng.mls_finish(empty_w, 0, 5, 3, h, [])
    assert len(eng.calls()) == calls and tuple(empty_w.shape) == (0, 32)
