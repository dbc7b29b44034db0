"""
The equalisation kernels alone (ira_eq_power, ira_eq_pyramid, ira_eq_smooth, ira_eq_invert, ira_eq_gather, ira_eq_taper)
on uploaded spectra and tables: every result BIT FOR BIT equal to the NumPy restatement of tests/equalise_ref.py.
N = 32, 64 and 4096: every level of the N/2 + 1 layout but the last two has an odd length, so the entry without a partner
is met at every level, and 4096 takes two tiles and two passes of the pyramid.  Rows of 1, 2 and 3 members in one call,
exact zero power bins, arbitrary window tables (all 153 windows of N = 32, the whole range), b = 0, 1, 3 and 48, the
second-spectrum form, clamped counts, rows without values beside live ones, the taper at 16 and 2048 taps, empty calls,
and the same bits whatever the cut into calls.
"""
import functools

import numpy as np
import pytest

import equalise_ref as R

pytestmark = pytest.mark.gpu

FS = 48000.0
SIZES = (32, 64, 4096)
ROWS = ([0], [1, 2], [3, 4, 5])


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def _host(t):
    return t.cpu().numpy()


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@functools.lru_cache(maxsize=None)
def spectra(n):
    """Six spectra of N/2 + 1 bins over twelve decades, with exact zeros: bin 3 of every one (a zero power bin in every
    row), a run in spectrum 0 and the whole of its upper quarter."""
    rng = np.random.default_rng(n)
    nb = n // 2 + 1
    x = (rng.standard_normal((6, nb)) + 1j * rng.standard_normal((6, nb))) * 10.0 ** rng.uniform(-6, 6, (6, nb))
    x[:, 3] = 0.0
    x[0, 7:11] = 0.0
    x[0, 3 * nb // 4 :] = 0.0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def second(n):
    rng = np.random.default_rng(7 * n)
    f = rng.standard_normal((len(ROWS), n // 2 + 1)) + 1j * rng.standard_normal((len(ROWS), n // 2 + 1))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference(n, with_second=False):
    """(P per row, flat pyramid per row): computed once per size."""
    x = spectra(n)
    p = [R.power([x[m] for m in row], second(n)[r] if with_second else None) for r, row in enumerate(ROWS)]
    return p, [R.flat_pyramid(q) for q in p]


def upload(eng, x):
    """complex128 (rows, bins) -> (float64 device, offsets in complex doubles)."""
    x = np.ascontiguousarray(x, dtype=np.complex128)
    return eng.to_dev(x.view(np.float64).reshape(-1).copy()), np.arange(x.shape[0], dtype=np.int64) * x.shape[1]


def device_pyramid(eng, n, rows=ROWS, with_second=False):
    spec, off = upload(eng, spectra(n))
    if with_second:
        f, f_off = upload(eng, second(n)[: len(rows)])
        pyr = eng.eq_power(spec, off, rows, n, spec2_dev=f, spec2_off=f_off)
    else:
        pyr = eng.eq_power(spec, off, rows, n)
    level0 = _host(pyr)[:, : n // 2 + 1].copy()
    eng.eq_pyramid(pyr, n)
    return pyr, level0


@pytest.mark.parametrize("with_second", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_power_and_every_level_of_the_pyramid(n, with_second):
    eng = _eng()
    p, flat = reference(n, with_second)
    pyr, level0 = device_pyramid(eng, n, with_second=with_second)
    got = _host(pyr)
    assert got.shape == (3, n + int(np.log2(n)))
    for r in range(3):
        assert same(level0[r], p[r]), (n, r)
        assert same(got[r], flat[r]), (n, r)
        assert p[r][3] == 0.0 and np.all(np.isfinite(p[r]))
    assert np.all(p[0][3 * (n // 2 + 1) // 4 :] == 0.0)


@pytest.mark.parametrize("b", [0, 1, 3, 48])
@pytest.mark.parametrize("n", SIZES)
def test_smoothing(n, b):
    eng = _eng()
    p, _ = reference(n)
    pyr, _ = device_pyramid(eng, n)
    lo, hi = R.windows(n, b)
    got = _host(eng.eq_smooth(pyr, lo, hi, n))
    for r in range(3):
        assert same(got[r], R.smooth(p[r], lo, hi)), (n, b, r)


def test_every_window_of_n32_and_the_whole_range():
    eng = _eng()
    p, _ = reference(32)
    pyr, _ = device_pyramid(eng, 32)
    pairs = [(a, c) for a in range(17) for c in range(a, 17)]
    assert len(pairs) == 153
    for at in range(0, 153, 17):                                             # 17 windows a call: one per bin
        lo, hi = np.array([a for a, _ in pairs[at : at + 17]]), np.array([c for _, c in pairs[at : at + 17]])
        got = _host(eng.eq_smooth(pyr, lo, hi, 32))
        for r in range(3):
            assert same(got[r], R.smooth(p[r], lo, hi)), (at, r)
    for n in SIZES:
        p, _ = reference(n)
        pyr, _ = device_pyramid(eng, n)
        nb = n // 2 + 1
        lo, hi = np.zeros(nb, dtype=np.int64), np.full(nb, n // 2, dtype=np.int64)
        lo[1::2] = np.arange(nb)[1::2]                                       # odd bins: from the bin to the end
        got = _host(eng.eq_smooth(pyr, lo, hi, n))
        for r in range(3):
            assert same(got[r], R.smooth(p[r], lo, hi)), (n, r)


def test_no_result_depends_on_the_cut_into_calls():
    eng = _eng()
    for n in (64, 4096):
        lo, hi = R.windows(n, 3)
        pyr, _ = device_pyramid(eng, n)
        whole = _host(eng.eq_smooth(pyr, lo, hi, n))
        for r, row in enumerate(ROWS):
            alone, _ = device_pyramid(eng, n, rows=(row,))
            assert same(_host(alone)[0], _host(pyr)[r])
            assert same(_host(eng.eq_smooth(alone, lo, hi, n))[0], whole[r])


@pytest.mark.parametrize("n", SIZES)
def test_inversion_counts_and_rows_without_values(n):
    eng = _eng()
    nb = n // 2 + 1
    rng = np.random.default_rng(n + 1)
    s = 10.0 ** rng.uniform(-6, 3, (5, nb))
    s[0, 2], s[0, 5] = 0.0, 0.0                                              # exact zero power bins: c = 1
    s[2] = 0.0                                                               # a silent row
    s[3, 4] = np.nan                                                         # a NaN row
    ref = np.array([1.0, 0.37, 0.0, np.nan, np.inf])
    t, beta = R.tables(n, FS, tilt=1.5)
    gain = 10.0 ** (6.0 / 20.0)
    off = np.arange(5, dtype=np.int64)[::-1].copy() * (nb + 3)               # rows placed in reverse, with gaps
    c_dev, clamped = eng.eq_invert(eng.to_dev(s.reshape(-1).copy()).view(5, nb), ref, t, beta, gain, off, n)
    got, counts = _host(c_dev), _host(clamped)
    for r in range(5):
        c, over = R.correction(s[r], ref[r], t, beta, gain)
        row = got[2 * off[r] : 2 * (off[r] + nb)].reshape(nb, 2)
        assert same(row[:, 0], c) and np.all(row[:, 1] == 0.0) and not np.signbit(row[:, 1]).any(), (n, r)
        assert int(counts[r]) == over, (n, r)
    c0, over0 = R.correction(s[0], 1.0, t, beta, gain)
    assert c0[2] == 1.0 and c0[5] == 1.0 and over0 > 0 and np.max(c0) == gain
    assert counts[2] == counts[3] == counts[4] == 0
    # the gather: S with stride 1, the real parts of c with stride 2
    bins = np.array([1, 2, nb - 2, 5, 0, nb - 1, 5])
    g = _host(eng.eq_gather(c_dev, 2 * off, 2, bins, n))
    for r in range(5):
        assert same(g[r], R.correction(s[r], ref[r], t, beta, gain)[0][bins])
    s_dev = eng.to_dev(s.reshape(-1).copy())
    g = _host(eng.eq_gather(s_dev, np.arange(5, dtype=np.int64) * nb, 1, bins, n))
    assert same(g, s[:, bins])


@pytest.mark.parametrize("taps,n", [(16, 32), (2048, 4096), (5, 64)])
def test_taper(taps, n):
    eng = _eng()
    rng = np.random.default_rng(taps)
    g = (rng.standard_normal((3, n)) * 10.0 ** rng.uniform(-30, 3, (3, n))).astype(np.float32)
    g[1, 0] = np.float32(2.0 ** -140)                                        # a subnormal tap
    v = R.taper(taps, 0.25)
    off = np.array([2 * n, 0, n], dtype=np.int64)
    got = _host(eng.eq_taper(eng.to_dev(g.reshape(-1).copy()), off, v, n))
    assert got.dtype == np.float32 and got.shape == (3, taps)
    for r, src in enumerate((2, 0, 1)):
        assert np.array_equal(got[r].view(np.uint32), R.apply_taper(g[src], v).view(np.uint32)), (taps, r)


def test_empty_calls_and_refusals():
    eng = _eng()
    t = eng.torch
    n = 64
    spec, off = upload(eng, spectra(n))
    pyr = eng.eq_power(spec, off, [], n)
    assert tuple(pyr.shape) == (0, n + 6)
    eng.eq_pyramid(pyr, n)
    lo, hi = R.windows(n, 3)
    s = eng.eq_smooth(pyr, lo, hi, n)
    assert tuple(s.shape) == (0, 33)
    tt, beta = R.tables(n, FS)
    c, clamped = eng.eq_invert(s, np.zeros(0), tt, beta, 4.0, np.zeros(0, dtype=np.int64), n)
    assert clamped.numel() == 0
    assert tuple(eng.eq_gather(c, np.zeros(0, dtype=np.int64), 2, np.array([1, 2]), n).shape) == (0, 2)
    assert tuple(eng.eq_gather(spec, off[:2] * 2, 2, np.zeros(0, dtype=np.int64), n).shape) == (2, 0)
    assert tuple(eng.eq_taper(eng.empty(4, t.float32), np.zeros(0, dtype=np.int64), R.taper(16), n).shape) == (0, 16)
    real, _ = device_pyramid(eng, n)
    for bad in (lambda: eng.eq_power(spec, off, [[6]], n), lambda: eng.eq_power(spec, off, [[]], n),
                lambda: eng.eq_power(spec, off, [[0]], 48), lambda: eng.eq_power(spec, off, [[0] * 257], n),
                lambda: eng.eq_smooth(real, lo[:-1], hi[:-1], n), lambda: eng.eq_smooth(real, hi + 1, hi, n),
                lambda: eng.eq_smooth(real, lo, hi + 1, n), lambda: eng.eq_smooth(real, lo, hi, 128),
                lambda: eng.eq_gather(spec, off * 2, 2, np.array([33]), n), lambda: eng.eq_gather(spec, off * 2, 3, np.array([1]), n),
                lambda: eng.eq_gather(spec, off * 2 + 400, 2, np.array([1]), n),
                lambda: eng.eq_taper(eng.empty(64, t.float32), np.array([0]), R.taper(33), n),
                lambda: eng.eq_taper(eng.empty(64, t.float32), np.array([60]), R.taper(16), n),
                lambda: eng.eq_invert(eng.eq_smooth(real, lo, hi, n), np.ones(3), tt, beta, 0.0, np.arange(3) * 33, n),
                lambda: eng.eq_invert(eng.eq_smooth(real, lo, hi, n), np.ones(3), tt, beta, 4.0, np.arange(3) * 32, n),
                lambda: eng.eq_invert(eng.eq_smooth(real, lo, hi, n), np.ones(3), tt[:-1], beta, 4.0, np.arange(3) * 33, n)):
        with pytest.raises(ValueError):
            bad()
