"""
Energy decay relief without a GPU: the header, the binding and the build flags, argument validation of both entry points
(nothing is launched: an empty call returns before any device is touched), the NumPy restatement (tests/edr_ref.py) against
long-double sums and against a closed-form input, the host geometry and row tables, the settings, the command line, the text
summary and the JSON round trip.
"""
import json
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import decay_ref as DR
import edr_ref as R

REPO = Path(__file__).resolve().parent.parent
U = 2.0 ** -53
NEW_SYMBOLS = ("ira_edr_power", "ira_edr_integrate")


def _edr():
    from audio_analysis_amd.analyse import edr as D
    return D


# ------------------------------------------------------------------------------------------------ library and binding
def test_header_prototypes_and_build_flags():
    from audio_analysis_amd import _lib, build, engine
    hdr = (REPO / "include" / "ira_edr.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ira_[a-z0-9_]+)\(", code))
    assert declared == set(_lib.EDR_PROTOTYPES) == set(NEW_SYMBOLS)
    assert not declared & set(_lib.PROTOTYPES) and not declared & set(_lib.EQUALISE_PROTOTYPES)
    for name, (res, args) in _lib.EDR_PROTOTYPES.items():
        m = re.search(rf"int32_t {name}\((.*?)\);", hdr, flags=re.S)
        assert m and len(m.group(1).split(",")) == len(args), name
        assert res is _lib.i32 and args[-1] is _lib.vp
    assert "replace no reference function" in hdr and '#include "ira.h"' in hdr
    for name, value in (("FRAMES", engine.EDR_FRAMES), ("BLOCK", engine.EDR_BLOCK), ("MAX_ROWS", engine.EDR_MAX_ROWS),
                        ("SERIAL", engine.EDR_SERIAL), ("DOUBLES", engine.EDR_DOUBLES)):
        assert re.search(rf"#define IRA_EDR_{name} {value}\b", hdr), name
    assert (engine.EDR_FRAMES, engine.EDR_BLOCK, engine.EDR_DOUBLES) == (R.FRAMES, R.BLOCK, 4) and engine.EDR_MAX_ROWS >= 240
    assert build.SOURCES["ira_edr.hip"] == ["-ffp-contract=off"]
    assert "IRA_ABI_VERSION" not in code                                    # the version is ira.h's, unchanged
    main = (REPO / "include" / "ira.h").read_text()
    assert re.search(r"#define IRA_ABI_VERSION 15\b", main) and _lib.ABI_VERSION == 15 and "ira_edr" not in main
    lib = _lib.load()
    assert lib.ira_abi_version() == 15
    assert all(getattr(lib, name).argtypes == _lib.EDR_PROTOTYPES[name][1] for name in NEW_SYMBOLS)
    src = (REPO / "audio_analysis_amd" / "csrc" / "ira_edr.hip").read_text()
    assert "atomic" not in src.replace("no atomics", "")


def test_entry_points_validate_arguments_without_gpu():
    from audio_analysis_amd import _lib
    lib = _lib.load()
    E_NULL, E_SIZE = -1, -2

    def call(fn, order, defaults):
        def run(**kw):
            a = dict(defaults)
            a.update(kw)
            return fn(*[a[q] for q in order], 0)
        run.__name__ = fn.__name__
        return run

    power = call(lib.ira_edr_power, ("x", "x_off", "n", "p_off", "nseg", "max_frames", "n_fft", "hop", "win", "tw", "first",
                                     "count", "nrows", "p"),
                 dict(x=1, x_off=1, n=1, p_off=1, nseg=0, max_frames=5, n_fft=2048, hop=256, win=1, tw=1, first=1, count=1,
                      nrows=30, p=1))
    integ = call(lib.ira_edr_integrate, ("p", "p_off", "T", "q", "c_off", "nseg", "nrows", "eps", "floor_db", "curve", "rec",
                                         "s"),
                 dict(p=1, p_off=1, T=1, q=1, c_off=1, nseg=0, nrows=30, eps=1e-30, floor_db=-120.0, curve=1, rec=1, s=0))
    pointers = {power: ("x", "x_off", "n", "p_off", "win", "tw", "first", "count", "p"),
                integ: ("p", "p_off", "T", "q", "c_off", "curve", "rec")}
    for fn, names in pointers.items():
        assert fn() == 0                                                    # nseg == 0: nothing to do
        for name in names:
            assert fn(**{name: 0}) == E_NULL and fn(nseg=3, **{name: 0}) == E_NULL, (fn.__name__, name)
        for kw in (dict(nseg=-1), dict(nseg=65536), dict(nrows=0), dict(nrows=257), dict(nrows=-3)):
            assert fn(**kw) == E_SIZE and fn(**{"nseg": 2, **kw}) == E_SIZE, (fn.__name__, kw)
        assert fn(nrows=1) == 0 and fn(nrows=256) == 0
    for kw in (dict(n_fft=128), dict(n_fft=16384), dict(n_fft=3000), dict(n_fft=0), dict(n_fft=-2048), dict(hop=0),
               dict(hop=2049), dict(hop=-1), dict(max_frames=-1)):
        assert power(**kw) == E_SIZE and power(nseg=2, **kw) == E_SIZE, kw
    assert power(n_fft=256, hop=256) == 0 and power(n_fft=8192, hop=1) == 0
    assert power(nseg=4, max_frames=0) == 0                                 # no frames: nothing to launch
    assert integ(s=1) == 0                                                  # the sums are optional
    for kw in (dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(floor_db=float("nan")),
               dict(floor_db=float("-inf"))):
        assert integ(**kw) == E_SIZE and integ(nseg=2, **kw) == E_SIZE, kw
    assert integ(eps=0.0) == 0


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 127, 128, 129, 1000])
def test_backward_sum_against_long_double(T):
    DR.need_longdouble()
    rng = np.random.default_rng(T)
    p = rng.random(T) ** 6 * 10.0 ** rng.uniform(-3, 3)
    got = R.backward_sum(p)
    want = np.cumsum(p.astype(np.longdouble)[::-1])[::-1]
    assert np.all(np.abs(got - want) <= T * U * want)
    # q = 0: nothing is subtracted, and the plain float64 running sum is within the same bound of it
    s, noise, rec = R.integrate_row(p, 0)
    assert noise == 0.0 and np.array_equal(s, got)
    assert np.all(np.abs(s - np.cumsum(p[::-1])[::-1]) <= T * U * np.cumsum(p[::-1])[::-1])
    assert rec.tolist() == [s[0], 0.0, p.max(), float(np.argmax(p))]


def test_backward_sum_is_exact_on_small_integers_and_keeps_the_block_order():
    p = np.arange(1, 201, dtype=np.float64)
    assert np.array_equal(R.backward_sum(p), np.cumsum(p[::-1])[::-1])
    # the stated order on one short block: the frames sit at the END of the 64 lanes, zeros in front
    a = np.array([1e16, 1.0, 1.0])
    assert R.backward_sum(a).tolist() == [(1e16 + 1.0) + 1.0, 2.0, 1.0] and (1e16 + 1.0) + 1.0 != 1e16 + 2.0


def test_noise_subtraction_and_non_finite_rows():
    p = np.array([8.0, 4.0, 2.0, 1.0, 1.0, 1.0])
    s, noise, rec = R.integrate_row(p, 3)
    assert noise == 1.0 and s.tolist() == [11.0, 4.0, 1.0, 0.0, 0.0, 0.0] and rec.tolist() == [11.0, 1.0, 8.0, 0.0]
    s, noise, _ = R.integrate_row(p, 6)
    assert noise == 17.0 / 6.0
    q = p.copy()
    q[2] = np.nan
    s, _, rec = R.integrate_row(q, 0)
    assert np.isnan(s[:3]).all() and s[3:].tolist() == [3.0, 2.0, 1.0] and np.isnan(rec[2]) and rec[3] == 2.0
    c = R.curve64(s, 1e-30, -120.0)
    assert np.isnan(c).all()                                                # S(0) NaN: the whole row
    assert R.curve64(np.zeros(4), 1e-30, -120.0).tolist() == [-120.0] * 4   # silent
    assert R.curve64(np.array([4.0, 1.0, 0.0]), 1e-30, -120.0).tolist() == [0.0, 10.0 * np.log10(0.25), -120.0]
    assert [R.status_of(0, 0.0, 1e-30), R.status_of(2, 0.0, 1e-30), R.status_of(2, np.nan, 1e-30),
            R.status_of(2, np.inf, 1e-30), R.status_of(2, 1.0, 1e-30)] == [1, 2, 4, 4, 0]


@pytest.mark.parametrize("n_fft,hop", [(1024, 256), (4096, 512)])
def test_closed_form_decay_times(n_fft, hop):
    x = R.closed_form_input()
    centres, first, count = R.rows_of(n_fft, 48000.0, *R.OCTAVE_EDGES, 1)
    assert np.allclose(centres[list(R.OCCUPIED)], R.TONES_HZ, rtol=1e-6) and centres.size == 7
    ref = R.channel_reference(x, 48000.0, n_fft, hop, "hann", first, count)
    worst = 0.0
    for j, t60 in zip(R.OCCUPIED, R.TONES_T60):
        assert ref["status"][j] == 0
        rel = np.abs(ref["times"][j] - t60) / t60
        worst = max(worst, float(rel.max()))
        assert np.all(rel <= 1e-3), (n_fft, j, ref["times"][j], t60)
    print(f"closed form at ({n_fft}, {hop}): worst relative deviation {worst:.3g}")


def test_closed_form_at_256_has_an_empty_row():
    x = R.closed_form_input(seconds=1.0)
    _, first, count = R.rows_of(256, 48000.0, *R.OCTAVE_EDGES, 1)
    assert count[0] == 0 and np.all(count[1:] > 0)                          # no bin between 88 and 177 Hz at 187.5 Hz a bin
    ref = R.channel_reference(x, 48000.0, 256, 64, "hann", first, count)
    assert ref["status"][0] == R.STATUS_EMPTY and np.isnan(ref["times"][0]).all() and np.all(ref["status"][1:] == 0)
    assert np.all(ref["curves"][0] == np.float32(-120.0)) and ref["records"][0, 0] == 0.0


# ------------------------------------------------------------------------------------------------ host geometry and rows
def test_layout_and_rows_equal_the_restatement():
    from audio_analysis_amd import engine_geometry as G
    from audio_analysis_amd.analyse.modalcloud import _build_log_bins
    D = _edr()
    frames = np.array([1, 15, 16, 17, 1000, 0, 33])
    for nrows in (1, 7, 256):
        pad, p_off, c_off, total = G.edr_layout(frames, nrows)
        rp, rpo, rco, rt = R.layout(frames, nrows)
        assert np.array_equal(pad, rp) and np.array_equal(p_off, rpo) and np.array_equal(c_off, rco) and total == rt
        assert np.all(pad % 16 == 0) and np.all(p_off % 16 == 0) and np.all(pad >= frames) and np.all(pad - frames < 16)
    for ppo in (4, 6, 24):
        assert np.array_equal(D.log_edges(20.0, 20000.0, ppo), _build_log_bins(20.0, 20000.0, ppo, 1))
    for n_fft, fs, lo, hi, ppo in ((2048, 48000, 20.0, 20000.0, 3), (8192, 48000, 20.0, 20000.0, 24), (256, 44100, 50.0, 30000.0, 1),
                                   (1024, 48000, *R.OCTAVE_EDGES, 1)):
        rows = D.edr_rows(n_fft, fs, lo, hi, ppo)
        nyq = 0.5 * fs
        centres, first, count = R.rows_of(n_fft, float(fs), min(max(lo, 1.0), nyq), min(hi, nyq), ppo)
        assert np.array_equal(rows.count, count) and np.array_equal(rows.centre_hz, centres)
        assert np.array_equal(rows.first[count > 0], first[count > 0])
        assert np.all(rows.first >= 0) and np.all(rows.first + rows.count <= n_fft // 2 + 1)
    assert D.edr_rows(2048, 48000, 20.0, 20000.0, 3).first.size == 30 and D.edr_rows(8192, 48000, 20.0, 20000.0, 24).first.size == 240
    assert np.any(D.edr_rows(2048, 48000, 20.0, 20000.0, 3).count == 0)     # the default settings have empty rows


# ------------------------------------------------------------------------------------------------ settings, CLI, text, JSON
def test_settings_defaults_and_validation():
    D = _edr()
    s = D.EdrSettings()
    assert (s.use_mono_downmix_for_stereo, s.trim_to_peak, s.ignore_leading_seconds, s.analysis_duration_seconds, s.n_fft,
            s.hop_length, s.use_hann_window, s.f_min_hz, s.f_max_hz, s.points_per_octave, s.noise_tail_fraction, s.eps,
            s.floor_db, s.min_fit_points, s.with_relief) == (False, True, 0.0, None, 2048, 256, True, 20.0, 20000.0, 3, 0.0,
                                                             1e-30, -120.0, 5, True)
    for kw in (dict(n_fft=128), dict(n_fft=16384), dict(n_fft=3000), dict(n_fft=2048.0), dict(hop_length=0),
               dict(hop_length=2049), dict(n_fft=256, hop_length=257), dict(ignore_leading_seconds=-1.0),
               dict(analysis_duration_seconds=0.0), dict(analysis_duration_seconds=float("nan")), dict(f_min_hz=0.0),
               dict(f_min_hz=500.0, f_max_hz=400.0), dict(f_max_hz=float("inf")), dict(points_per_octave=0),
               dict(points_per_octave=49), dict(points_per_octave=2.5), dict(noise_tail_fraction=-0.1),
               dict(noise_tail_fraction=1.5), dict(eps=-1.0), dict(eps=float("nan")), dict(floor_db=-30.0),
               dict(floor_db=float("-inf")), dict(min_fit_points=1)):
        with pytest.raises(ValueError):
            D.EdrSettings(**kw)
    assert D.EdrSettings(n_fft=256, hop_length=256, noise_tail_fraction=1.0, eps=0.0).n_fft == 256


def _result(D, relief=True, dead=False):
    j, t = 3, 4
    nan = float("nan")
    status = np.array([0, D.STATUS_EMPTY, D.STATUS_NON_FINITE if dead else 0], dtype=np.int64)
    ok = status == 0
    v = lambda a: np.where(ok, np.asarray(a, dtype=np.float64), np.nan)      # noqa: E731
    return D.EdrChannelResult(
        channel_name="a.wav:left", sample_rate_hz=48000, analysis_start_sample_index=12, analysis_length_samples=3000,
        n_fft=2048, hop_length=256, frames=t, noise_frames=0, frame_seconds=256 / 48000.0,
        centre_hz=np.array([125.0, 250.0, 500.0]), low_edge_hz=np.array([88.4, 176.8, 353.6]),
        high_edge_hz=np.array([176.8, 353.6, 707.1]), bin_count=np.array([4, 0, 15], dtype=np.int64), status=status,
        initial_level_db=v([0.0, 0.0, -6.25]), total_energy=np.array([4.0, 0.0, nan if dead else 1.0]),
        noise_power=np.zeros(j), peak_time_seconds=np.array([0.0, nan, 256 / 48000.0]),
        edt_seconds=v([1.5, 0, 0.9]), edt_r2=v([0.99991, 0, 0.98]), edt_valid=ok.copy(),
        t20_seconds=v([1.6, 0, 1.0]), t20_r2=v([0.99992, 0, 0.97]), t20_valid=ok.copy(),
        t30_seconds=v([1.625, 0, 1.01]), t30_r2=v([0.99993, 0, 0.96]), t30_valid=ok.copy(),
        median_t30_seconds=1.625 if dead else 1.3175, longest_t30_hz=125.0,
        relief_db=np.array([[0, -1, -2, -120], [-120] * 4, [nan] * 4 if dead else [0, -3, -6, -9]], dtype=np.float32)
        if relief else None)


def test_text_format_is_pinned():
    D = _edr()
    lines = D.summarise_edr_text([_result(D)]).split("\n")
    assert lines[0] == "[a.wav:left]"
    assert lines[1] == "Frames: 4 of 2048 every 256 samples (5.333 ms)  Noise frames: 0  Rows: 3"
    assert lines[2] == "freq_Hz  bins  level_dB  EDT_s  T20_s  T30_s  r2_T30  status"
    assert lines[3] == "125.0  4  0.00  1.500  1.600  1.625  0.9999  ok"
    assert lines[4] == "250.0  0  NA  NA  NA  NA  NA  1 (empty)"
    assert lines[5] == "500.0  15  -6.25  0.900  1.000  1.010  0.9600  ok"
    assert lines[6] == "median T30: 1.317 s over 2 rows, longest at 125.0 Hz" or lines[6].startswith("median T30: 1.318 s")
    assert lines[7] == "" and len(lines) == 9
    assert "500.0  15  NA  NA  NA  NA  NA  4 (non-finite)" in D.summarise_edr_text([_result(D, dead=True)])
    assert D.status_text(3) == "3 (empty, silent)"


def test_json_round_trip_writes_nan_as_null():
    D = _edr()
    for res in ([_result(D), _result(D, dead=True)], [_result(D, relief=False)]):
        text = json.dumps(D.edr_results_to_json(res))
        assert "NaN" not in text
        back = D.edr_results_from_json(json.loads(text))
        for a, b in zip(res, back):
            for name, v in a.__dict__.items():
                w = getattr(b, name)
                if v is None:
                    assert w is None, name
                elif isinstance(v, np.ndarray):
                    assert w.dtype == v.dtype and w.shape == v.shape and np.array_equal(v, w, equal_nan=v.dtype.kind == "f"), name
                elif isinstance(v, float) and math.isnan(v):
                    assert math.isnan(w), name
                else:
                    assert v == w and type(v) is type(w), name
    assert "relief_db" not in D.edr_results_to_json([_result(D)], with_relief=False)["energy_decay_relief"][0]


def test_parser_defaults_and_the_shim():
    D = _edr()
    p = D.build_parser()
    a = p.parse_args(["--input", "a.wav", "b.wav"])
    assert D.settings_from_args(a) == D.EdrSettings() and a.json is None and a.expected_sample_rate == 48000
    a = p.parse_args(["--bundle", "dir", "--mono", "--n-fft", "4096", "--hop", "512", "--window", "rect",
                      "--points-per-octave", "24", "--f-min", "30", "--f-max", "18000", "--noise-tail-fraction", "0.1",
                      "--duration", "2.5", "--ignore-leading", "0.01", "--no-trim", "--floor-db", "-100", "--min-fit-points",
                      "8", "--no-relief", "--expected-sample-rate", "44100", "--json", "o.json"])
    assert D.settings_from_args(a) == D.EdrSettings(
        use_mono_downmix_for_stereo=True, trim_to_peak=False, ignore_leading_seconds=0.01, analysis_duration_seconds=2.5,
        n_fft=4096, hop_length=512, use_hann_window=False, f_min_hz=30.0, f_max_hz=18000.0, points_per_octave=24,
        noise_tail_fraction=0.1, floor_db=-100.0, min_fit_points=8, with_relief=False)
    assert a.expected_sample_rate == 44100 and a.json == Path("o.json")
    with pytest.raises(SystemExit):
        p.parse_args(["--input", "a.wav", "--bundle", "d"])
    with pytest.raises(SystemExit):
        D.main(["--input", "a.wav", "--n-fft", "3000"])                     # a ValueError of the settings is a usage error
    sys.modules.pop("analyse.edr", None)
    import analyse.edr as shim
    assert shim is D
    for flag in ("--n-fft", "--hop", "--window", "--points-per-octave", "--f-min", "--f-max", "--noise-tail-fraction",
                 "--duration", "--ignore-leading", "--no-trim", "--floor-db", "--min-fit-points", "--no-relief"):
        assert flag in D.__doc__ and flag in p.format_help(), flag


def test_product_path_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from audio_analysis_amd._lib import IraError
    D = _edr()
    with pytest.raises(IraError):
        D.analyse_edr_for_channel(np.zeros(4000, np.float32), 48000, "m", D.EdrSettings())
