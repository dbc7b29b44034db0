"""ira_waterfall_rel and both layouts of ira_logbin_aggregate (ira_modal.hip) called through the C-ABI, on buffers this
file owns, against the restatements of tests/modal_ref.py (whose case tables tests/test_modal_ref_cpu.py shows to reject
the subtly wrong kernels).

Every input and output of a launch lies in one guarded flat buffer (tests/guard_buffers.py); every guard and gap of
every output must come back untouched.  Every element of a ragged launch is also launched alone, in buffers of its own,
and must give the same bytes.

ira_waterfall_rel is held to the restatement exactly (a maximum, one float32 subtraction, two comparisons); the log-bin
curves to |got - long double| <= ulp32 / 2 + modal_ref.logbin_bound_db(count), with the same NaN cells and infinities.
test_zz_report prints the largest error / bound per layout.  Measured on an MI355X: 0.9998 for both layouts, i.e. every
value is the float32 nearest to the long-double one (half a float32 ulp is all but the whole bound: the float64
allowance is eight orders of magnitude smaller and only matters next to a rounding boundary).

What these tests found (fixed with them): both log-bin kernels clamped a NaN mean to 1e-30 (fmax), so a (bin, frame)
cell whose rows hold a NaN came out as -600 dB where the reference (numpy.maximum) and the fused ira_stft_logbin give NaN.
"""
import numpy as np
import pytest

import modal_ref as R
from guard_buffers import Flat, to_device as _dev, untouched, words

pytestmark = pytest.mark.gpu
IRA_OK, IRA_E_SIZE = 0, -2
STATS = {}


@pytest.fixture(scope="module")
def eng():
    R.need_longdouble()
    from audio_analysis_amd.engine import get_engine
    return get_engine()


# ----------------------------------------------------------------------------------------------------------- waterfall
def waterfall(eng, mats, k_lo, nsel, slice_max, dyn, phase=0):
    """One launch over the (F, S) matrices; the (S, nsel) float32 results."""
    lin, lout = Flat([m.size for m in mats], phase=phase), Flat([m.shape[1] * nsel for m in mats], phase=phase + 3)
    mag, out = _dev(eng, lin.filled([m.ravel() for m in mats])), _dev(eng, lout.filled())
    moff, ooff = _dev(eng, np.array(lin.off, np.int64)), _dev(eng, np.array(lout.off, np.int64))
    nsl = _dev(eng, np.array([m.shape[1] for m in mats], np.int32))
    rc = eng.lib.ira_waterfall_rel(mag.data_ptr(), moff.data_ptr(), nsl.data_ptr(), len(mats), k_lo, nsel, int(slice_max),
                                   float(dyn), out.data_ptr(), ooff.data_ptr(), eng.stream)
    assert rc == IRA_OK
    segs = lout.split(out.cpu().numpy(), "ira_waterfall_rel")
    assert np.array_equal(words(mag.cpu().numpy()), words(lin.filled([m.ravel() for m in mats]))), "the input was written"
    return [s.reshape(m.shape[1], nsel) for s, m in zip(segs, mats)]


@pytest.mark.parametrize("slice_max", [False, True], ids=["global", "slice_max"])
@pytest.mark.parametrize("k_lo,nsel", R.WF_SELECTIONS)
def test_waterfall_rel_is_exact(eng, k_lo, nsel, slice_max):
    for dyn in R.WF_DYN:
        mats = R.waterfall_case(k_lo, nsel, slice_max, dyn)
        got = waterfall(eng, mats, k_lo, nsel, slice_max, dyn)
        for e, (m, g) in enumerate(zip(mats, got)):
            what = f"k_lo {k_lo} nsel {nsel} slice_max {slice_max} dyn {dyn} element {e} (S = {m.shape[1]})"
            R.check_waterfall(g, R.waterfall_rel(m, k_lo, nsel, slice_max, dyn), what)
            alone = waterfall(eng, [m], k_lo, nsel, slice_max, dyn, phase=e + 1)[0]
            assert np.array_equal(words(alone), words(g)), f"{what}: alone and in the batch differ"


def test_waterfall_rel_refusals(eng):
    m = R.waterfall_case(3, 5, False, 60.0)[3]
    lay = Flat([m.shape[1] * 5])
    mag, out = _dev(eng, m.ravel()), _dev(eng, lay.filled())
    z64, nsl = _dev(eng, np.zeros(1, np.int64)), _dev(eng, np.array([m.shape[1]], np.int32))
    ooff = _dev(eng, np.array(lay.off, np.int64))

    def call(nb, k_lo, nsel):
        return eng.lib.ira_waterfall_rel(mag.data_ptr(), z64.data_ptr(), nsl.data_ptr(), nb, k_lo, nsel, 0, 60.0,
                                         out.data_ptr(), ooff.data_ptr(), eng.stream)

    assert call(0, 3, 5) == IRA_OK and call(-1, 3, 5) == IRA_E_SIZE
    assert call(1, -1, 5) == IRA_E_SIZE and call(1, 3, 0) == IRA_E_SIZE
    assert untouched(out.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------- log bins
def logbin(eng, mats, k_base, first, count, frame_major, phase=0, rows=None, max_frames=None, nb=None, nbins=None):
    """One launch over the (F, T) matrices (handed over as (T, F) when frame_major).  (rc, the (nbins, T) float32 results,
    or the untouched buffer when nothing was to be written)."""
    segs = [np.ascontiguousarray(m.T).ravel() if frame_major else m.ravel() for m in mats]
    lin, lout = Flat([s.size for s in segs], phase=phase), Flat([count.size * m.shape[1] for m in mats], phase=phase + 2)
    mag, out = _dev(eng, lin.filled(segs)), _dev(eng, lout.filled())
    moff, ooff = _dev(eng, np.array(lin.off, np.int64)), _dev(eng, np.array(lout.off, np.int64))
    nfr = _dev(eng, np.array([m.shape[1] for m in mats], np.int32))
    fi, co = _dev(eng, first.astype(np.int32)), _dev(eng, count.astype(np.int32))
    rc = eng.lib.ira_logbin_aggregate(mag.data_ptr(), moff.data_ptr(), nfr.data_ptr(), len(mats) if nb is None else nb,
                                      max(m.shape[1] for m in mats) if max_frames is None else max_frames, k_base,
                                      fi.data_ptr(), co.data_ptr(), count.size if nbins is None else nbins, out.data_ptr(),
                                      ooff.data_ptr(), (mats[0].shape[0] if rows is None else rows) if frame_major else 0,
                                      eng.stream)
    back = out.cpu().numpy()
    if rc != IRA_OK or 0 in (nb, nbins, max_frames):
        return rc, back
    return rc, [s.reshape(count.size, m.shape[1]) for s, m in zip(lout.split(back, "ira_logbin_aggregate"), mats)]


@pytest.mark.parametrize("frame_major", [False, True], ids=["ft", "frame_major"])
@pytest.mark.parametrize("nrows,k_base", R.LB_GEOMETRIES)
def test_logbin_aggregate_against_long_double(eng, nrows, k_base, frame_major):
    first, count, mats, refs = R.logbin_case(nrows, k_base)
    rc, got = logbin(eng, mats, k_base, first, count, frame_major)
    assert rc == IRA_OK
    layout = "frame-major" if frame_major else "(F, T)"
    for e, (m, g, ref) in enumerate(zip(mats, got, refs)):
        what = f"{layout} rows {nrows} k_base {k_base} element {e} (T = {m.shape[1]})"
        worst = R.check_logbin(g, ref, count, what)
        STATS[layout] = max(STATS.get(layout, 0.0), worst)
        assert np.all(g[list(count).index(8)] == np.float32(-600.0)), f"{what}: the bin below 1e-30 is not exactly -600 dB"
        rc, alone = logbin(eng, [m], k_base, first, count, frame_major, phase=e + 1)
        assert rc == IRA_OK and np.array_equal(words(alone[0]), words(g)), \
            f"{what}: alone and in the batch differ"


def test_logbin_aggregate_refusals(eng):
    first, count, mats, _ = R.logbin_case(420, 37)
    one = [mats[3]]
    assert logbin(eng, one, 37, first, count, True, rows=8194)[0] == IRA_E_SIZE
    assert logbin(eng, one, 420, first, count, True)[0] == IRA_E_SIZE
    assert logbin(eng, one, 421, first, count, True)[0] == IRA_E_SIZE
    assert logbin(eng, one, -1, first, count, True)[0] == IRA_E_SIZE
    for frame_major in (False, True):
        for kw in (dict(nb=0), dict(nbins=0), dict(max_frames=0)):
            rc, back = logbin(eng, one, 37, first, count, frame_major, **kw)
            assert rc == IRA_OK and untouched(back), (frame_major, kw)


def test_zz_report():
    for layout, worst in sorted(STATS.items()):
        print(f"ira_logbin_aggregate {layout}: largest error / bound {worst:.4f}")
