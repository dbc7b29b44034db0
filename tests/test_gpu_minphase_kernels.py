"""ira_minphase_logmag, ira_minphase_excess, ira_minphase_gather and ira_minphase_spectrum (the five kernels of
ira_minphase.hip) called through the C-ABI, on float64 buffers this file owns, against the long-double restatements of
tests/minphase_kernels_ref.py (whose case tables tests/test_minphase_kernels_ref_cpu.py shows to reject the subtly wrong
kernels).  tests/test_gpu_minphase.py holds the whole chain to bounds the float32 cepstrum dominates (1e-7 rad); here each
kernel answers for its own arithmetic, at every bin.

Every buffer a launch writes is a guarded flat buffer (tests/guard_buffers.py): every guard and gap must come back
untouched, and every input buffer unchanged.  Every element of a ragged launch (max_nfft = 32768 with elements of 32 ..
32768 points; max_nfft = 131072 with elements of at most 4096, where most workgroups own no bin) is also launched alone,
in buffers of its own at another phase of the gaps, and must give the same bytes.  One ragged launch goes through the
engine's wrappers and must return the bytes the C-ABI gave.

Held exactly: P (numpy.max of the float64 powers, NaN and inf included), the floored count at floor_db = -120, -60, 0 and
-300 with bins planted a few float64 steps either side of the floor, every gathered field, Im G, Im M at the edge bins,
the zeros of an element without values, and the wrap where d is exact (d = +-pi, 3 pi: the tie).  Held to derived bounds
(the restatement's docstring): G within LIB_ULP ulp, the wrapped excess phase within u (11 pi + 2 |d|), M within 9 u |M|.

test_zz_report prints the worst error over bound per kernel and the worst error of each library function in ulp.
Measured on an MI355X, worst over every case: ln 0.63 ulp, atan2 1.33 ulp, exp 0.85 ulp, sincos 0.64 ulp (LIB_ULP = 2
assumed); G at 0.31 of its bound, the wrapped excess phase at 0.85 of its bound (12 bins of the tables compared modulo
2 pi, all of them planted on odd multiples of pi), M at 0.26 of its bound (2.3 u |M|); P and the floored count exact,
854 960 gathered fields bit-equal, every element the same bytes alone and in the batch, no guard or input touched.

What these tests found: no fault in ira_minphase.hip.  The suspicion that a -0.0 in the transforms' Im X_0 turns the
excess-phase curve of a channel with a negative sample sum by 360 degrees is settled at the chain level
(tests/test_gpu_minphase.py::test_polarity_and_a_negative_sample_sum): Bluestein, the full-length and the half-length
direct transforms all leave +0.0 there, so mp_excess reads Im X as it stands, as the restatement does.  One wrong kernel
of the CPU table cannot be rejected and is recorded there as such: k p in wrapped int32 is the same function for a
power-of-two N.
"""
import numpy as np
import pytest

import minphase_kernels_ref as K
from guard_buffers import Flat, to_device as _dev, untouched, words as _words

pytestmark = pytest.mark.gpu
IRA_OK, IRA_E_SIZE = 0, -2
STATS = {}


@pytest.fixture(scope="module")
def eng():
    K.need_longdouble()
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def _stat(name, value):
    STATS[name] = max(STATS.get(name, 0.0), float(value))


def _nbins(els):
    return [e["n"] // 2 + 1 for e in els]


def _tables(eng, els, layout):
    return (_dev(eng, np.array(layout.off, np.int64)), _dev(eng, np.array([e["n"] for e in els], np.int32)))


def _same(dev, host, what):
    assert np.array_equal(_words(dev.cpu().numpy()), _words(host.view(np.float64) if host.dtype == np.complex128 else host)), \
        f"{what}: an input buffer was written"


def _pmax_host(els):
    return np.array([e["P"] for e in els], np.float64)


# -------------------------------------------------------------------------------------------------------------- logmag
def logmag(eng, els, floor_db, max_nfft, phase=0):
    """One launch: (G per element complex128, P (nb,), count (nb,))."""
    nb = len(els)
    lay, lp, lc = Flat(_nbins(els), np.complex128, phase), Flat([nb], np.float64, phase), Flat([nb], np.int64, phase)
    x_host = lay.filled([e["X"] for e in els])
    x, g, pm, cnt = _dev(eng, x_host), _dev(eng, lay.filled()), _dev(eng, lp.filled()), _dev(eng, lc.filled())
    off, nf = _tables(eng, els, lay)
    rc = eng.lib.ira_minphase_logmag(x.data_ptr(), off.data_ptr(), nf.data_ptr(), nb, int(max_nfft), float(floor_db), g.data_ptr(),
                                     pm.data_ptr() + 8 * lp.off[0], cnt.data_ptr() + 8 * lc.off[0], eng.stream)
    assert rc == IRA_OK
    G = lay.split(g.cpu().numpy(), "ira_minphase_logmag G")
    P = lp.split(pm.cpu().numpy(), "ira_minphase_logmag pmax")[0]
    C = lc.split(cnt.cpu().numpy().view(np.int64), "ira_minphase_logmag floored")[0]
    _same(x, x_host, "ira_minphase_logmag")
    return G, P, C


@pytest.mark.parametrize("floor_db", K.FLOORS_DB)
def test_logmag_exact_p_and_count_and_g_against_long_double(eng, floor_db):
    for els, max_nfft in ((K.elements(), K.MAIN_MAX_NFFT), (K.sparse_elements(), K.SPARSE_MAX_NFFT)):
        G, P, C = logmag(eng, els, floor_db, max_nfft)
        for i, e in enumerate(els):
            what = f"floor {floor_db:g} dB, max_nfft {max_nfft}, element {e['name']} (N = {e['n']})"
            ratio, lib = K.check_logmag(G[i], P[i], C[i], e["X"], floor_db, what)
            _stat("G: |dG| / (LIB_ULP ulp)", ratio), _stat("ln, ulp", lib)
            Ga, Pa, Ca = logmag(eng, [e], floor_db, e["n"], phase=i + 1)
            assert np.array_equal(_words(Ga[0]), _words(G[i])) and _words(Pa)[0] == _words(P[i:i + 1])[0] and Ca[0] == C[i], \
                f"{what}: alone and in the batch differ"


def test_logmag_refusals(eng):
    e = K.elements()[0]
    lay = Flat([17], np.complex128)
    x, g, sc = _dev(eng, lay.filled([e["X"]])), _dev(eng, lay.filled()), _dev(eng, Flat([2], np.float64).filled())
    off, nf = _tables(eng, [e], lay)

    def call(nb, max_nfft, floor_db):
        return eng.lib.ira_minphase_logmag(x.data_ptr(), off.data_ptr(), nf.data_ptr(), nb, max_nfft, floor_db, g.data_ptr(),
                                           sc.data_ptr() + 128, sc.data_ptr() + 136, eng.stream)

    assert call(0, 32, -120.0) == IRA_OK
    for bad in ((-1, 32, -120.0), (1, 16, -120.0), (1, 48, -120.0), (1, 1 << 22, -120.0), (1, 32, 1.0), (1, 32, -301.0),
                (1, 32, float("nan"))):
        assert call(*bad) == IRA_E_SIZE, bad
    assert untouched(g.cpu().numpy()) and untouched(sc.cpu().numpy())


# -------------------------------------------------------------------------------------------------------------- excess
def excess(eng, els, max_nfft, phase=0):
    nb = len(els)
    lay, lo = Flat(_nbins(els), np.complex128, phase), Flat(_nbins(els), np.float64, phase)
    assert lay.off == lo.off                                              # one table of offsets serves X, T and the output
    x_host, t_host = lay.filled([e["X"] for e in els]), lay.filled([e["T"] for e in els])
    p_host, c_host = _pmax_host(els), np.array([e["p"] for e in els], np.int64)
    x, t, out, pm, c = _dev(eng, x_host), _dev(eng, t_host), _dev(eng, lo.filled()), _dev(eng, p_host), _dev(eng, c_host)
    off, nf = _tables(eng, els, lay)
    rc = eng.lib.ira_minphase_excess(x.data_ptr(), t.data_ptr(), off.data_ptr(), nf.data_ptr(), c.data_ptr(), pm.data_ptr(), nb,
                                     int(max_nfft), out.data_ptr(), eng.stream)
    assert rc == IRA_OK
    got = lo.split(out.cpu().numpy(), "ira_minphase_excess")
    _same(x, x_host, "ira_minphase_excess X"), _same(t, t_host, "ira_minphase_excess T")
    _same(pm, p_host, "ira_minphase_excess pmax"), _same(c, c_host, "ira_minphase_excess centre")
    return got


def _held_excess(got, e, what):
    ratio, near, lib = K.check_excess(got, e["X"], e["T"], e["p"], e["n"], e["valid"], what)
    _stat("excess: error / (u (11 pi + 2 |d|))", ratio), _stat("atan2, ulp", lib)
    STATS["excess: bins compared modulo 2 pi"] = STATS.get("excess: bins compared modulo 2 pi", 0) + near


def test_excess_against_long_double(eng):
    for els, max_nfft in ((K.elements(), K.MAIN_MAX_NFFT), (K.sparse_elements(), K.SPARSE_MAX_NFFT)):
        got = excess(eng, els, max_nfft)
        for i, e in enumerate(els):
            what = f"max_nfft {max_nfft}, element {e['name']} (N = {e['n']}, p = {e['p']})"
            _held_excess(got[i], e, what)
            alone = excess(eng, [e], e["n"], phase=i + 1)
            assert np.array_equal(_words(alone[0]), _words(got[i])), f"{what}: alone and in the batch differ"


def test_excess_at_two_to_the_21_points_and_the_largest_centre(eng):
    """One launch, one long-double pass over 2^20 + 1 bins: k p reaches 2^51."""
    e = K.big_element()
    _held_excess(excess(eng, [e], e["n"])[0], e, "N = 2^21, p = 2^31 - 1")


# -------------------------------------------------------------------------------------------------------------- gather
def gather(eng, els, bins, phase=0):
    nb, npts = bins.shape
    lay, lu, lr = Flat(_nbins(els), np.complex128, phase), Flat(_nbins(els), np.float64, phase), \
        Flat([nb * npts * K.FIELDS], np.float64, phase)
    hosts = [lay.filled([e["X"] for e in els]), lay.filled([e["T"] for e in els]), lu.filled([e["u"] for e in els]),
             _pmax_host(els), np.ascontiguousarray(bins, np.int32)]
    x, t, u, pm, b = (_dev(eng, h) for h in hosts)
    out = _dev(eng, lr.filled())
    off, nf = _tables(eng, els, lay)
    rc = eng.lib.ira_minphase_gather(x.data_ptr(), t.data_ptr(), u.data_ptr(), off.data_ptr(), nf.data_ptr(), b.data_ptr(),
                                     pm.data_ptr(), nb, npts, out.data_ptr() + 8 * lr.off[0], eng.stream)
    assert rc == IRA_OK
    rec = lr.split(out.cpu().numpy(), "ira_minphase_gather")[0].reshape(nb, npts, K.FIELDS)
    for d, h, name in zip((x, t, u, pm), hosts, ("X", "T", "unwrapped", "pmax")):
        _same(d, h, f"ira_minphase_gather {name}")
    assert np.array_equal(b.cpu().numpy(), hosts[4])
    return rec


@pytest.mark.parametrize("npts", K.NPTS)
def test_gather_bits(eng, npts):
    els = K.elements()
    for abi in ((False, True) if npts >= 6 else (False,)):
        bins = K.gather_bins(npts, abi)
        rec = gather(eng, els, bins)
        for i, e in enumerate(els):
            what = f"npts {npts}{', bins 0, -5, N/2, 2^30 among them' if abi else ''}, element {e['name']} (N = {e['n']})"
            K.check_gather(rec[i], e["X"], e["T"], e["u"], bins[i], e["n"], e["valid"], what)
            if not abi and npts in (1, 257):
                alone = gather(eng, [e], bins[i:i + 1], phase=i + 1)
                assert np.array_equal(_words(alone[0]), _words(rec[i])), f"{what}: alone and in the batch differ"
    STATS["gather: fields compared, all bit-equal"] = STATS.get("gather: fields compared, all bit-equal", 0) + \
        (2 if npts >= 6 else 1) * len(els) * npts * K.FIELDS


# ------------------------------------------------------------------------------------------------------------ spectrum
def spectrum(eng, els, max_nfft, phase=0):
    nb = len(els)
    lay = Flat(_nbins(els), np.complex128, phase)
    t_host, p_host = lay.filled([e["T"] for e in els]), _pmax_host(els)
    g, t, pm = _dev(eng, lay.filled([e["G"] for e in els])), _dev(eng, t_host), _dev(eng, p_host)
    off, nf = _tables(eng, els, lay)
    rc = eng.lib.ira_minphase_spectrum(g.data_ptr(), t.data_ptr(), off.data_ptr(), nf.data_ptr(), pm.data_ptr(), nb, int(max_nfft),
                                       eng.stream)
    assert rc == IRA_OK
    M = lay.split(g.cpu().numpy(), "ira_minphase_spectrum")
    _same(t, t_host, "ira_minphase_spectrum T"), _same(pm, p_host, "ira_minphase_spectrum pmax")
    return M


def test_spectrum_against_long_double(eng):
    for els, max_nfft in ((K.elements(), K.MAIN_MAX_NFFT), (K.sparse_elements(), K.SPARSE_MAX_NFFT)):
        M = spectrum(eng, els, max_nfft)
        for i, e in enumerate(els):
            what = f"max_nfft {max_nfft}, element {e['name']} (N = {e['n']})"
            ratio, lib_exp, lib_sc = K.check_spectrum(M[i], e["G"], e["T"], e["valid"], what)
            _stat(f"spectrum: |dM| / ({K.SPEC_C:g} u |M|)", ratio), _stat("exp, ulp", lib_exp), _stat("sincos, ulp", lib_sc)
            alone = spectrum(eng, [e], e["n"], phase=i + 1)
            assert np.array_equal(_words(alone[0]), _words(M[i])), f"{what}: alone and in the batch differ"


# -------------------------------------------------------------------------------------------------- the engine wrappers
def test_the_engine_wrappers_return_the_bytes_of_the_c_abi(eng):
    """The ragged launch through Engine.minphase_logmag / _excess / _gather / _spectrum, on tightly packed buffers (the
    wrappers size their outputs by the bins), against the guarded C-ABI launches above."""
    els = K.elements()
    nbins = np.array(_nbins(els), np.int64)
    off = np.concatenate([[0], np.cumsum(nbins)[:-1]]).astype(np.int64)
    n_fft = np.array([e["n"] for e in els], np.int32)
    cut = lambda flat, width=1: [flat[int(o) * width:int(o + n) * width] for o, n in zip(off, nbins)]
    x, t, u, gin = (_dev(eng, np.concatenate([e[q] for e in els])) for q in ("X", "T", "u", "G"))
    pm = _dev(eng, _pmax_host(els))
    floor_db = -60.0
    g, p, c = eng.minphase_logmag(x, off, n_fft, floor_db)
    G, P, C = logmag(eng, els, floor_db, K.MAIN_MAX_NFFT)
    for got, want in zip(cut(g.cpu().numpy(), 2), G):
        assert np.array_equal(_words(got), _words(want))
    assert np.array_equal(_words(p.cpu().numpy()), _words(P)) and np.array_equal(c.cpu().numpy(), C)
    centre = np.array([e["p"] for e in els], np.int64)
    ex = eng.minphase_excess(x, t, off, n_fft, centre, pm).cpu().numpy()
    for got, want in zip(cut(ex), excess(eng, els, K.MAIN_MAX_NFFT)):
        assert np.array_equal(_words(got), _words(want))
    bins = K.gather_bins(479)
    rec = eng.minphase_gather(x, t, u, off, n_fft, bins, pm).cpu().numpy()
    assert np.array_equal(_words(rec), _words(gather(eng, els, bins)))
    with pytest.raises(ValueError):
        eng.minphase_gather(x, t, u, off, n_fft, K.gather_bins(479, True), pm)
    eng.minphase_spectrum(gin, t, off, n_fft, pm)
    for got, want in zip(cut(gin.cpu().numpy(), 2), spectrum(eng, els, K.MAIN_MAX_NFFT)):
        assert np.array_equal(_words(got), _words(want))


def test_zz_report():
    for name, worst in sorted(STATS.items()):
        print(f"ira_minphase {name}: {worst:.4g}" if isinstance(worst, float) else f"ira_minphase {name}: {worst}")
    print(f"P and the floored count exact at every element and floor; LIB_ULP = {K.LIB_ULP:g}")
