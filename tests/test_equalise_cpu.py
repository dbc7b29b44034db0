"""
Equalisation without a GPU: the NumPy restatement (tests/equalise_ref.py) against exact sums and closed forms, the host
tables of engine_geometry against it, the settings, the header and the binding, argument validation of every entry point
(nothing is launched: an empty call returns before any device is touched), the command line and the JSON round trip.
"""
import json
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import equalise_ref as R

REPO = Path(__file__).resolve().parent.parent
FS = 48000.0
U = 2.0 ** -53


def _eq():
    from audio_analysis_amd.analyse import equalise as D
    return D


def _geometry():
    from audio_analysis_amd import engine_geometry as G
    return G


# ------------------------------------------------------------------------------------------------ the window sum
def _exact(p, lo, hi):
    return np.array([math.fsum(p[a : c + 1]) for a, c in zip(lo, hi)])


def _exact_fast(p, lo, hi):
    """What math.fsum returns -- the exact sum rounded once -- for every window, from exact prefix sums in integers (a
    double is an integer multiple of 2^-1074; int / int divides with one correct rounding).  math.fsum itself over all
    windows of N = 65536 is 4e8 additions; it is called on every 97th window beside this and must agree to the bit."""
    units = [a * ((1 << 1074) // b) for a, b in (v.as_integer_ratio() for v in p.tolist())]
    prefix = [0]
    for u in units:
        prefix.append(prefix[-1] + u)
    out = np.array([(prefix[c + 1] - prefix[a]) / (1 << 1074) for a, c in zip(lo.tolist(), hi.tolist())])
    some = slice(None, None, 97)
    assert np.array_equal(out[some], _exact(p, lo[some], hi[some]))
    return out


def test_every_window_of_n32_against_fsum():
    rng = np.random.default_rng(1)
    p = rng.random(17) ** 8
    pairs = [(a, c) for a in range(17) for c in range(a, 17)]
    assert len(pairs) == 153
    lo, hi = np.array([a for a, _ in pairs]), np.array([c for _, c in pairs])
    got, want = R.query(R.pyramid(p), lo, hi), _exact(p, lo, hi)
    assert np.all(np.abs(got - want) <= R.window_ulps(32) * U * want)


@pytest.mark.parametrize("n", [64, 4096, 65536])
def test_window_sums_against_fsum(n):
    rng = np.random.default_rng(n)
    p = rng.random(n // 2 + 1) ** 8                                          # eight decades of dynamic range
    lv = R.pyramid(p)
    assert [a.size for a in lv] == R.layout(n)[1].tolist() and lv[-1].size == 1
    assert all(a.size % 2 == 1 for a in lv[:-2])                            # N/2 + 1: every level but the last two is odd
    for b in (0, 1, 3, 6, 48):
        lo, hi = R.windows(n, b)
        got, want = R.query(lv, lo, hi), (_exact if n <= 4096 else _exact_fast)(p, lo, hi)
        worst = float(np.max(np.abs(got - want) / (U * want)))
        assert worst <= R.window_ulps(n), (n, b, worst)
        if b == 0:
            assert np.array_equal(got, p)


def test_pyramid_copies_the_entry_without_a_partner():
    p = np.array([1.0, 2.0, 4.0, 8.0, 16.0])
    lv = R.pyramid(p)
    assert [a.tolist() for a in lv] == [[1, 2, 4, 8, 16], [3, 12, 16], [15, 16], [31]]
    assert R.query(lv, [0, 1, 4, 2], [4, 3, 4, 2]).tolist() == [31, 14, 16, 4]


@pytest.mark.parametrize("n", [32, 64, 4096, 1 << 20])
@pytest.mark.parametrize("b", [0, 1, 3, 6, 48])
def test_window_tables(n, b):
    G = _geometry()
    lo, hi = G.equalise_windows(n, b)
    k = np.arange(n // 2 + 1)
    assert lo.dtype == np.int32 and hi.dtype == np.int32 and lo.size == hi.size == n // 2 + 1
    assert np.all(lo <= k) and np.all(k <= hi) and lo[0] == 0 == hi[0] and hi.max() <= n // 2
    assert np.all(np.diff(lo) >= 0) and np.all(np.diff(hi) >= 0)
    rl, rh = R.windows(n, b)
    assert np.array_equal(lo, rl) and np.array_equal(hi, rh)
    if b:
        # the window of bin k spans 1/b octave: hi / lo <= 2^(1/b), and one more bin on either side would exceed it
        q = k[1:].astype(np.float64)
        assert np.all(hi[1:] <= q * 2.0 ** (0.5 / b)) and np.all(lo[1:] >= q * 2.0 ** (-0.5 / b))
    else:
        assert np.array_equal(lo, k) and np.array_equal(hi, k)


def test_window_tables_refuse_other_smoothings():
    G = _geometry()
    for b in (-1, 49):
        with pytest.raises(ValueError):
            G.equalise_windows(64, b)


def test_layout_row_doubles_and_cut():
    G = _geometry()
    for n in (32, 64, 4096, 1 << 14, 1 << 20, 1 << 21):
        off, lens = G.equalise_layout(n)
        ro, rl = R.layout(n)
        assert np.array_equal(off, ro) and np.array_equal(lens, rl)
        assert lens.size == int(math.log2(n)) + 1 and G.equalise_row_doubles(n) == n + int(math.log2(n))
    # the multi-pass pyramid: more than one tile of level 0 from N = 2^12 on
    assert (4096 // 2 + 1) > G.EQ_TILE >= (2048 // 2 + 1)
    need = G.equalise_scratch_bytes(1 << 20, [1, 1, 3])
    assert need.tolist() == [(8 * m + 60) * (1 << 20) + 1024 for m in (1, 1, 3)]
    assert G.equalise_cut(1 << 20, [1] * 5, scratch_bytes=2 * int(need[0])) == [(0, 2), (2, 4), (4, 5)]
    assert G.equalise_cut(1 << 20, [3], scratch_bytes=1) == [(0, 1)] and G.equalise_cut(64, []) == []


# ------------------------------------------------------------------------------------------------ tables
def test_target_and_regularisation_tables():
    G = _geometry()
    n, fs = 4800, 48000.0                                                    # 10 Hz a bin (the tables take any even size)
    t, beta = G.equalise_tables(n, fs, 40.0, 16000.0, 0.5, -20.0, 20.0, 0.0)
    rt, rb = R.tables(n, fs)
    assert np.array_equal(t, rt) and np.array_equal(beta, rb) and np.all(t == 1.0)
    db = 10.0 * np.log10(beta)
    assert db[0] == 20.0                                                     # k = 0: w = 1
    assert abs(db[4] + 20.0) < 1e-12 and abs(db[1600] + 20.0) < 1e-12        # the band edges: inside value
    assert np.all(np.abs(db[4:1601] + 20.0) < 1e-12)
    assert abs(db[2] - 20.0) < 1e-12                                         # 20 Hz: an octave below, beyond the transition
    assert np.all(np.abs(db[2263:] - 20.0) < 1e-12)                          # 16000 * 2^0.5 = 22627 Hz on: outside value
    # mid-transition (a quarter octave out): w = 0.5 -> 0 dB; no bin lies exactly there, so restate the formula at it
    for f, edge_lo in ((40.0 * 2.0 ** -0.25, True), (16000.0 * 2.0 ** 0.25, False)):
        u = (math.log2(40.0 / f) if edge_lo else math.log2(f / 16000.0)) / 0.5
        assert abs(u - 0.5) < 1e-12 and abs(-20.0 + 0.5 * (1.0 - math.cos(math.pi * u)) * 40.0) < 1e-9
    k = 1903                                                                 # 19030 Hz = 16000 * 2^0.2502: just past mid-transition
    assert abs(db[k] - (-20.0 + 0.5 * (1.0 - math.cos(math.pi * math.log2(19030.0 / 16000.0) / 0.5)) * 40.0)) < 1e-9
    assert -1.0 < db[k - 1] < 0.1 < db[k + 1] < 1.0 or abs(db[k]) < 0.1
    assert np.all(np.diff(db[1600:2264]) >= 0) and np.all(np.diff(db[1:5]) <= 0)
    # the tilt: 3 dB per octave around 1 kHz, t_0 = t_1
    t3, _ = G.equalise_tables(n, fs, 40.0, 16000.0, 0.5, -20.0, 20.0, 3.0)
    assert t3[0] == t3[1] and abs(20.0 * math.log10(t3[100])) < 1e-12
    assert abs(20.0 * math.log10(t3[200]) - 3.0) < 1e-12 and abs(20.0 * math.log10(t3[50]) + 3.0) < 1e-12


@pytest.mark.parametrize("taps,fade", [(16, 0.25), (2048, 0.25), (128, 0.0), (8, 1.0)])
def test_taper(taps, fade):
    G = _geometry()
    v = G.equalise_taper(taps, fade)
    assert np.array_equal(v, R.taper(taps, fade)) and v.size == taps
    n0 = taps - int(np.rint(fade * taps))
    assert np.all(v[:n0] == 1.0) and np.all(np.diff(v[max(n0 - 1, 0):]) < 0) and np.all(v > 0.0)
    if n0 < taps:
        m = taps - n0 + 1
        assert v[n0] == 0.5 * (1.0 + math.cos(math.pi / m)) and v[-1] == 0.5 * (1.0 + math.cos(math.pi * (m - 1) / m))
        assert v[-1] < 0.5 * (math.pi / m) ** 2                               # the last tap is the step before zero


# ------------------------------------------------------------------------------------------------ settings
def test_settings_defaults_and_validation():
    D = _eq()
    s = D.EqualiseSettings()
    assert (s.smoothing, s.f_low_hz, s.f_high_hz, s.transition_octaves, s.regularisation_db, s.outside_db, s.max_boost_db,
            s.tilt_db_per_octave, s.taps, s.fade, s.oversample, s.n_fft, s.post_ms, s.points_per_octave, s.f_min_hz,
            s.f_max_hz, s.average) == (6, 40.0, 16000.0, 0.5, -20.0, 20.0, 12.0, 0.0, 8192, 0.25, 2, None, None, 48, 20.0,
                                       20000.0, False)
    assert abs(s.max_gain - 10.0 ** 0.6) < 1e-15
    bad = [dict(smoothing=-1), dict(smoothing=49), dict(smoothing=2.5), dict(smoothing=True), dict(f_low_hz=0.0),
           dict(f_low_hz=float("nan")), dict(f_high_hz=40.0), dict(f_high_hz=30.0), dict(transition_octaves=0.0),
           dict(regularisation_db=float("inf")), dict(regularisation_db=-301.0), dict(outside_db="x"),
           dict(max_boost_db=float("nan")), dict(tilt_db_per_octave=float("inf")), dict(taps=0), dict(taps=1.5),
           dict(taps=(1 << 20) + 1), dict(fade=-0.1), dict(fade=1.5), dict(oversample=0), dict(n_fft=48), dict(n_fft=16),
           dict(n_fft=8192), dict(n_fft=1 << 22), dict(post_ms=-1.0), dict(points_per_octave=0), dict(f_min_hz=-1.0),
           dict(f_max_hz=10.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            D.EqualiseSettings(**kw)
    assert D.EqualiseSettings(n_fft=16384).n_fft == 16384 and D.EqualiseSettings(taps=16, n_fft=32).n_fft == 32


def test_sizes():
    D = _eq()
    st = D.EqualiseSettings(taps=16)
    assert D.equalise_sizes([5, 100], None, FS, st)[1] == 256                # 2 * 100 -> 256
    assert D.equalise_sizes([5], None, FS, st)[1] == 32                      # max(10, 32, 32)
    assert D.equalise_sizes([5], None, FS, D.EqualiseSettings())[1] == 16384  # 2 * taps
    seg, n = D.equalise_sizes([1000, 50], [10, 40], FS, D.EqualiseSettings(taps=16, post_ms=1.0))
    assert seg.tolist() == [59, 50] and n == 128
    assert D.equalise_sizes([100], None, FS, D.EqualiseSettings(taps=16, n_fft=128))[1] == 128
    with pytest.raises(ValueError, match="n_fft"):
        D.equalise_sizes([200], None, FS, D.EqualiseSettings(taps=16, n_fft=128))
    with pytest.raises(ValueError) as e:
        D.equalise_sizes([(1 << 20) + 1], None, FS, st)
    assert all(w in str(e.value) for w in ("post_ms", "oversample", "taps"))


# ------------------------------------------------------------------------------------------------ closed forms
def _filter(x, n, b, taps, fs=FS, **kw):
    X = np.fft.rfft(np.asarray(x, dtype=np.float32).astype(np.float64), n=n)
    d = R.design([X], n, fs, b=b, **kw)
    ch = R.filter_chain(d["c"], n)
    return d, ch, ch["g"][:taps] * R.taper(taps)


def test_unit_impulse_gives_the_unit_filter():
    x = np.zeros(40, dtype=np.float32)
    x[0] = 1.0
    for b in (0, 3, 6):
        d, ch, f = _filter(x, 256, b, 128)
        assert d["ref"] == 1.0 and np.all(d["c"] == 1.0) and d["clamped"] == 0
        delta = np.zeros(128)
        delta[0] = 1.0
        assert np.max(np.abs(f - delta)) <= R.closed_bound(256)


def test_one_pole_is_undone_by_its_inverse():
    n, taps = 256, 128
    d, ch, f = _filter(R.one_pole(64), n, 0, taps, reg_in=-300.0, reg_out=-300.0, max_boost_db=200.0)
    assert d["clamped"] == 0 and R.valid(d["ref"])
    want = np.zeros(taps)
    want[0], want[1] = 1.0, -0.5
    err = float(np.max(np.abs(f / math.sqrt(d["ref"]) - want)))
    assert err <= R.closed_bound(n), err
    # and the prediction is flat at the reference level: A_k / ref = 1
    F, a, a_s = R.predict([np.fft.rfft(R.one_pole(64).astype(np.float64), n=n)], f.astype(np.float32), n, d["lo"], d["hi"])
    assert np.max(np.abs(a_s / d["ref"] - 1.0)) < 1e-6                       # (float32 taps)


def test_correction_limits_and_clamp():
    t, beta = np.ones(5), np.full(5, 0.01)
    s = np.array([0.0, 1e-8, 1.0, 1e4, 0.01])
    c, over = R.correction(s, 1.0, t, beta, 10.0 ** 0.6)
    assert c[0] == 1.0 and over == 1                                         # an exact zero: the unit filter
    assert abs(c[1] - 1.01) < 1e-3 and abs(c[2] - 1.0) < 1e-15 and abs(c[3] - 0.01) < 1e-6
    assert c[4] == 10.0 ** 0.6                                               # (0.1 + 0.01) / 0.02 = 5.5 > 3.98: clamped
    # the largest boost without the clamp at reg_in -20 dB: 14.85 dB
    a = np.logspace(-4, 1, 200001)
    assert abs(20.0 * math.log10(float(np.max((a + 0.01) / (a * a + 0.01)))) - 14.85) < 0.005
    for ref in (0.0, float("nan"), float("inf"), -1.0):
        c, over = R.correction(s, ref, t, beta, 4.0)
        assert np.all(c == 1.0) and over == 0
    # d ln c / d ln s lies in (-1, 0.5): the slope the device-against-NumPy bound rests on
    s = np.logspace(-12, 12, 4001)
    for b in (1e-30, 0.01, 100.0):
        lc = np.log((np.sqrt(s) + b) / (s + b))
        slope = np.diff(lc) / np.diff(np.log(s))
        assert slope.min() > -1.0 and slope.max() < 0.5


def test_arithmetic_equals_the_restatement_bit_for_bit():
    D = _eq()
    rng = np.random.default_rng(3)
    x = rng.standard_normal(300).astype(np.float32)
    n = 1024
    X = np.fft.rfft(x.astype(np.float64), n=n)
    d = R.design([X], n, FS, b=3)
    ch = R.filter_chain(d["c"], n)
    f32 = R.apply_taper(ch["g"].astype(np.float32), R.taper(64))
    _, _, a_s = R.predict([X], f32, n, d["lo"], d["hi"])
    k = d["bins"]
    st = D.EqualiseSettings(smoothing=3, taps=64)
    assert np.array_equal(D.equalise_grid(st, FS), d["f"]) and np.array_equal(D.equalise_bins(d["f"], n, FS), k)
    assert D.reference_level(d["S"][k], d["in_band"]) == d["ref"]
    got = D.equalise_arithmetic(d["S"][k], d["c"][k], a_s[k], d["t"][k], k, d["in_band"], n, d["ref"], d["clamped"], FS)
    want = R.arithmetic(d["S"][k], d["c"][k], a_s[k], d["t"][k], k, d["in_band"], n, d["ref"], d["clamped"], FS)
    for name, v in want.items():
        assert np.array_equal(np.asarray(got[name]), np.asarray(v)), name
    assert got["deviation_after_db"] < got["deviation_before_db"]
    dead = D.equalise_arithmetic(d["S"][k], d["c"][k], a_s[k], d["t"][k], k, d["in_band"], n, 0.0, 0, FS)
    assert math.isnan(dead["reference_level_db"]) and np.isnan(dead["before_db"]).all() and np.isnan(dead["after_db"]).all()
    assert math.isnan(D.reference_level(d["S"][k], np.zeros(k.size, dtype=bool)))


# ------------------------------------------------------------------------------------------------ library and binding
NEW_SYMBOLS = ("ira_eq_power", "ira_eq_pyramid", "ira_eq_smooth", "ira_eq_invert", "ira_eq_gather", "ira_eq_taper")


def test_header_prototypes_and_build_flags():
    from audio_analysis_amd import _lib, build, engine
    hdr = (REPO / "include" / "ira_equalise.h").read_text()
    declared = set(re.findall(r"\b(ira_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_lib.EQUALISE_PROTOTYPES) == set(NEW_SYMBOLS)
    assert not declared & set(_lib.PROTOTYPES)
    for name, (res, args) in _lib.EQUALISE_PROTOTYPES.items():
        m = re.search(rf"int32_t {name}\((.*?)\);", hdr, flags=re.S)
        assert m and len(m.group(1).split(",")) == len(args), name
        assert res is _lib.i32 and args[-1] is _lib.vp
    assert "replace no reference function" in hdr and '#include "ira.h"' in hdr
    for name, value in (("TILE_LOG2", engine.EQ_TILE_LOG2), ("MAX_MEMBERS", engine.EQ_MAX_MEMBERS)):
        assert re.search(rf"#define IRA_EQ_{name} {value}\b", hdr), name
    assert engine.EQ_TILE == 1 << engine.EQ_TILE_LOG2
    assert build.SOURCES["ira_equalise.hip"] == ["-ffp-contract=off"]
    assert "IRA_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)  # the version is ira.h's, unchanged
    lib = _lib.load()
    assert all(getattr(lib, name).argtypes == _lib.EQUALISE_PROTOTYPES[name][1] for name in NEW_SYMBOLS)
    src = (REPO / "audio_analysis_amd" / "csrc" / "ira_equalise.hip").read_text()
    assert "atomicAdd(clamped + row, (u64)over)" in src and src.count("atomic") == 3  # one integer atomic (and two comments)


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

    power = call(lib.ira_eq_power, ("spec", "spec_off", "nspec", "member", "nmember", "first", "nrows", "spec2", "spec2_off",
                                    "nfft", "pyr"),
                 dict(spec=1, spec_off=1, nspec=1, member=1, nmember=1, first=1, nrows=0, spec2=0, spec2_off=0, nfft=64, pyr=1))
    pyramid = call(lib.ira_eq_pyramid, ("pyr", "nrows", "nfft"), dict(pyr=1, nrows=0, nfft=64))
    smooth = call(lib.ira_eq_smooth, ("pyr", "lo", "hi", "nrows", "nfft", "s"), dict(pyr=1, lo=1, hi=1, nrows=0, nfft=64, s=1))
    invert = call(lib.ira_eq_invert, ("s", "ref", "t", "beta", "gain", "c_off", "nrows", "nfft", "c", "clamped"),
                  dict(s=1, ref=1, t=1, beta=1, gain=4.0, c_off=1, nrows=0, nfft=64, c=1, clamped=1))
    gather = call(lib.ira_eq_gather, ("src", "src_off", "stride", "bins", "nrows", "npts", "nfft", "out"),
                  dict(src=1, src_off=1, stride=1, bins=1, nrows=0, npts=5, nfft=64, out=1))
    taper = call(lib.ira_eq_taper, ("g", "g_off", "v", "nrows", "taps", "nfft", "f"),
                 dict(g=1, g_off=1, v=1, nrows=0, taps=16, nfft=64, f=1))
    pointers = {power: ("spec", "spec_off", "member", "first", "pyr"), pyramid: ("pyr",), smooth: ("pyr", "lo", "hi", "s"),
                invert: ("s", "ref", "t", "beta", "c_off", "c", "clamped"), gather: ("src", "src_off", "bins", "out"),
                taper: ("g", "g_off", "v", "f")}
    for fn, names in pointers.items():
        assert fn() == 0                                                    # nrows == 0: nothing to do
        for name in names:
            assert fn(**{name: 0}) == E_NULL and fn(nrows=3, **{name: 0}) == E_NULL, (fn.__name__, name)
        for kw in (dict(nrows=-1), dict(nrows=65536), dict(nfft=16), dict(nfft=48), dict(nfft=0), dict(nfft=-64),
                   dict(nfft=1 << 22)):
            assert fn(**kw) == E_SIZE and fn(**{"nrows": 2, **kw}) == E_SIZE, (fn.__name__, kw)
        assert fn(nfft=32) == 0 and fn(nfft=1 << 21) == 0
    assert power(spec2=1) == E_NULL and power(spec2=1, spec2_off=1) == 0     # a second spectrum needs its offsets
    for kw in (dict(nspec=0), dict(nmember=0), dict(nspec=(1 << 24) + 1), dict(nmember=-2)):
        assert power(**kw) == E_SIZE and power(nrows=2, **kw) == E_SIZE
    for gain in (0.0, -1.0, float("nan"), float("inf")):
        assert invert(gain=gain) == E_SIZE and invert(nrows=2, gain=gain) == E_SIZE
    for kw in (dict(stride=0), dict(stride=3), dict(npts=-1), dict(npts=4097)):
        assert gather(**kw) == E_SIZE and gather(nrows=2, **kw) == E_SIZE
    assert gather(nrows=2, npts=0) == 0 and gather(stride=2) == 0
    for kw in (dict(taps=0), dict(taps=33), dict(taps=-4)):
        assert taper(**kw) == E_SIZE and taper(nrows=2, **kw) == E_SIZE
    assert taper(taps=32) == 0 and taper(taps=1) == 0


# ------------------------------------------------------------------------------------------------ text, JSON, CLI
def _result(D, with_curve=True, dead=False):
    j = 97
    curves = {}
    if with_curve:
        f = 20.0 * 2.0 ** (np.arange(j) / 48.0)
        nan = np.full(j, np.nan)
        curves = dict(frequencies_hz=f, bin=np.arange(1, j + 1), before_db=nan if dead else np.linspace(-3, 3, j),
                      target_db=np.zeros(j), correction_db=nan if dead else np.linspace(3, -3, j),
                      after_db=nan if dead else np.full(j, 0.125))
    nanv = float("nan")
    return D.EqualiseResult(name="a.wav:left", members=("a.wav:left",), sample_rate_hz=48000, fft_size=16384, taps=8192,
                            smoothing=6, points_per_octave=48, reference_level_db=nanv if dead else -12.5,
                            clamped_share=nanv if dead else 0.015, deviation_before_db=nanv if dead else 2.25,
                            deviation_after_db=nanv if dead else 0.5, **curves)


def test_text_and_markdown_formats_are_pinned():
    D = _eq()
    text = D.summarise_equalise_text([_result(D)])
    lines = text.split("\n")
    assert lines[0] == "[a.wav:left]"
    assert lines[1] == "Members: 1  N = 16384, 8192 taps  Smoothing: 1/6 octave  Reference level: -12.50 dB  Points: 97 (48 per octave)"
    assert lines[2] == "freq_Hz  before_dB  target_dB  correction_dB  after_dB"
    assert lines[3] == "20.0  -3.00  0.00  3.00  0.12" or lines[3] == "20.0  -3.00  0.00  3.00  0.13"
    assert len(lines) == 3 + 3 + 3 and lines[5].startswith("80.0  3.00")
    assert lines[6] == "deviation from the target: 2.25 dB before, 0.50 dB after, clamped bins: 1.50 %" and lines[7] == ""
    dead = D.summarise_equalise_text([_result(D, dead=True)])
    assert "Reference level: NA dB" in dead and "20.0  NA  0.00  NA  NA" in dead and "clamped bins: NA %" in dead
    md = D.summarise_equalise_markdown([_result(D)])
    assert md.startswith("### a.wav:left\n\nMembers: 1. N = 16384, 8192 taps. Smoothing: 1/6 octave.")
    assert "| freq (Hz) | before (dB) | target (dB) | correction (dB) | after (dB) |" in md
    assert "Smoothing: none" in D.summarise_equalise_text([D.EqualiseResult(**{**_result(D, False).__dict__, "smoothing": 0})])


def test_json_round_trip_writes_nan_as_null():
    D = _eq()
    for res in ([_result(D), _result(D, dead=True)], [_result(D, with_curve=False)]):
        doc = D.equalise_results_to_json(res)
        text = json.dumps(doc)
        assert "NaN" not in text
        back = D.equalise_results_from_json(json.loads(text))
        for a, b in zip(res, back):
            for name, v in a.__dict__.items():
                w = getattr(b, name)
                if v is None:
                    assert w is None
                elif isinstance(v, np.ndarray):
                    assert np.array_equal(v, w, equal_nan=v.dtype.kind == "f") and w.dtype == (np.int64 if name == "bin" else v.dtype)
                elif isinstance(v, float) and math.isnan(v):
                    assert math.isnan(w)
                else:
                    assert v == w, name
    assert json.loads(json.dumps(D.equalise_results_to_json([_result(D, dead=True)])))["equalisation"][0]["reference_level_db"] is None
    assert "before_db" not in D.equalise_results_to_json([_result(D)], with_curve=False)["equalisation"][0]


def test_parser_and_the_shim():
    D = _eq()
    p = D.build_parser()
    a = p.parse_args(["--input", "a.wav", "b.wav"])
    assert D.settings_from_args(a) == D.EqualiseSettings() and a.write_filters is None and not a.no_curve
    a = p.parse_args(["--bundle", "dir", "--mono", "--average", "--smoothing", "3", "--f-low", "50", "--f-high", "12000",
                      "--transition-octaves", "1", "--regularisation-db", "-30", "--outside-db", "10", "--max-boost-db", "6",
                      "--tilt-db-per-octave", "-1", "--taps", "4096", "--fade", "0.5", "--oversample", "4", "--fft-size", "32768",
                      "--post-ms", "20", "--points-per-octave", "24", "--f-min", "30", "--f-max", "18000", "--no-curve",
                      "--write-filters", "out", "--expected-sample-rate", "44100", "--json", "o.json"])
    assert D.settings_from_args(a) == D.EqualiseSettings(
        smoothing=3, f_low_hz=50.0, f_high_hz=12000.0, transition_octaves=1.0, regularisation_db=-30.0, outside_db=10.0,
        max_boost_db=6.0, tilt_db_per_octave=-1.0, taps=4096, fade=0.5, oversample=4, n_fft=32768, post_ms=20.0,
        points_per_octave=24, f_min_hz=30.0, f_max_hz=18000.0, average=True, use_mono_downmix_for_stereo=True)
    assert a.write_filters == Path("out") and a.no_curve and a.expected_sample_rate == 44100 and a.json == Path("o.json")
    with pytest.raises(SystemExit):
        p.parse_args(["--input", "a.wav", "--bundle", "d"])
    with pytest.raises(SystemExit):
        D.main(["--input", "a.wav", "--smoothing", "99"])                    # a ValueError of the settings is a usage error
    sys.modules.pop("analyse.equalise", None)
    import analyse.equalise as shim
    assert shim is D
    for flag in ("--average", "--smoothing", "--write-filters", "--fft-size", "--tilt-db-per-octave"):
        assert flag in D.__doc__ and flag in p.format_help()
