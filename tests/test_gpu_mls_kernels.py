"""ira_mls_fold, ira_mls_hadamard and ira_mls_finish (ira_mls.hip) called through the C-ABI, each alone, on buffers this file
owns, against the restatement of tests/mls_ref.py.  Every buffer a launch writes is a guarded flat buffer
(tests/guard_buffers.py): every guard must come back untouched, and every input buffer unchanged.

Held to the bit: the transform of random float64 rows (signed zeros, denormals, a row with a NaN) at every pass count of the
plan (T = 12: orders up to 12 one pass, 13 two, 21 three); Y through G and w[0] = 0; the float32 response.  E and D are held
to the long-double sums of the float64 terms the kernel forms (restated one by one, so only the order of the additions is
open) within gamma_c times the sum of the terms, c = engine.mls_sum_chain: the longest chain of additions of the kernel's
reduction, restated below from its block sizes.

Measured on an MI355X: every transform, fold and response equal to the bit (orders 2 .. 13 at 1, 3 and 65 channels, order
21 at one), no guard touched; E at 0.119 and D at 0.083 of their bounds at worst (the test prints each).
"""
import numpy as np
import pytest

import mls_ref as R
from guard_buffers import Flat, to_device as _dev, words as _words

pytestmark = pytest.mark.gpu
IRA_OK = 0
T = 12                                            # the tile order of ira_mls_hadamard


@pytest.fixture(scope="module")
def eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def _rows(rng, nb, order):
    """Random float64 rows over many binades with signed zeros and denormals; the last row of a batch of 3 holds a NaN."""
    n = 1 << order
    w = rng.standard_normal((nb, n)) * np.exp2(rng.integers(-40, 40, (nb, n)).astype(np.float64))
    w[:, 0] = 0.0
    w[:, 1 % n] = -0.0
    if n >= 8:
        w[:, 5] = 5e-324
        w[:, 6] = -2.5e-310
        w[:, 7] = 0.0
    if nb == 3:
        w[2, n // 2] = np.nan
    return w


def hadamard(eng, w, order):
    nb = w.shape[0]
    lay = Flat([w.size], np.float64, phase=order)
    buf = _dev(eng, lay.filled([w.reshape(-1)]))
    rc = eng.lib.ira_mls_hadamard(buf.data_ptr() + 8 * lay.off[0], nb, order, eng.stream)
    assert rc == IRA_OK
    return lay.split(buf.cpu().numpy(), f"ira_mls_hadamard order {order} nb {nb}")[0].reshape(nb, -1)


@pytest.mark.parametrize("nb", [1, 3, 65])
@pytest.mark.parametrize("order", [2, 3, 4, 6, T - 1, T, T + 1])
def test_hadamard_bit_for_bit(eng, order, nb):
    from audio_analysis_amd.engine import mls_pass_plan
    assert len(mls_pass_plan(order)) == (1 if order <= T else 2)
    w = _rows(np.random.default_rng(100 * order + nb), nb, order)
    got = hadamard(eng, w, order)
    ref = R.fwht(w)
    same = (_words(got) == _words(ref)) | (np.isnan(got) & np.isnan(ref))
    assert same.all(), f"order {order}, nb {nb}: {int((~same).sum())} values differ, first at {int(np.argmax(~same))}"
    if nb == 3:
        assert np.isnan(got[2]).all() and np.isfinite(got[:2]).all()       # the NaN fills its row and no other


def test_hadamard_three_passes(eng):
    from audio_analysis_amd.engine import mls_pass_plan
    assert mls_pass_plan(21) == [(0, 12), (12, 5), (17, 4)]                # the smallest order with three passes
    w = _rows(np.random.default_rng(21), 1, 21)
    got = hadamard(eng, w, 21)
    assert np.array_equal(_words(got), _words(R.fwht(w)))


# ---------------------------------------------------------------------------------------------------------------- fold
def fold(eng, chans, begins, order, periods, phase=0):
    """One launch over channels laid out with guards and gaps: (w rows, sums (nb, 2))."""
    from audio_analysis_amd.engine import mls_fold_blocks, mls_tables
    nb = len(chans)
    g, _ = mls_tables(order)
    lx = Flat([c.size for c in chans], np.float32, phase)
    lw, ls = Flat([nb << order], np.float64, phase), Flat([2 * nb], np.float64, phase + 1)
    lsc = Flat([2 * nb * mls_fold_blocks(order)], np.float64, phase + 2)
    x_host = lx.filled(chans)
    x, w, s, sc = _dev(eng, x_host), _dev(eng, lw.filled()), _dev(eng, ls.filled()), _dev(eng, lsc.filled())
    beg = _dev(eng, np.array([o + b for o, b in zip(lx.off, begins)], np.int64))
    gd = _dev(eng, np.ascontiguousarray(g))
    rc = eng.lib.ira_mls_fold(x.data_ptr(), beg.data_ptr(), nb, order, periods, gd.data_ptr(), w.data_ptr() + 8 * lw.off[0],
                              s.data_ptr() + 8 * ls.off[0], sc.data_ptr() + 8 * lsc.off[0], eng.stream)
    assert rc == IRA_OK
    what = f"ira_mls_fold order {order} R {periods}"
    rows = lw.split(w.cpu().numpy(), what + " w")[0].reshape(nb, -1)
    sums = ls.split(s.cpu().numpy(), what + " sums")[0].reshape(nb, 2)
    lsc.split(sc.cpu().numpy(), what + " scratch")
    assert np.array_equal(_words(x.cpu().numpy()), _words(x_host)), what + ": the samples were written"
    return rows, sums


@pytest.mark.parametrize("periods", [1, 2, 5])
@pytest.mark.parametrize("order", [2, 5, T + 1])
def test_fold_bits_and_sums(eng, order, periods):
    from audio_analysis_amd.engine import MLS_FOLD_BLOCKS, MLS_FOLD_THREADS, mls_fold_blocks, mls_sum_chain, mls_tables
    p = (1 << order) - 1
    rng = np.random.default_rng(10 * order + periods)
    begins = [1, 3, 0, 7]                                      # with the gaps of the layout: every alignment of the loads
    chans = [rng.standard_normal(b + periods * p + 2).astype(np.float32) for b in begins]
    rows, sums = fold(eng, chans, begins, order, periods)
    g, _ = mls_tables(order)
    # the longest chain of additions, from the kernel's block sizes: a thread's own terms, the wave tree (6), the 4 waves
    # (3), the workgroups of the channel
    blocks = min(-(-p // MLS_FOLD_THREADS), MLS_FOLD_BLOCKS)
    chain = -(-p // (blocks * MLS_FOLD_THREADS)) * periods + 6 + 3 + blocks
    assert blocks == mls_fold_blocks(order) and chain == mls_sum_chain(order, periods)
    for c, (x, b) in enumerate(zip(chans, begins)):
        y = R.fold(x, b, p, periods)
        assert np.array_equal(_words(rows[c]), _words(R.scatter(y, g, order))), f"channel {c}: Y through G"
        assert _words(rows[c, :1])[0] == 0                                     # w[0] = +0.0
        e_ld, d_ld, e_abs, d_abs = R.sums_ld(x, b, p, periods)
        e_err, d_err = abs(np.longdouble(sums[c, 0]) - e_ld), abs(np.longdouble(sums[c, 1]) - d_ld)
        print(f"order {order} R {periods} channel {c}: E err/bound {float(e_err / (R.gamma(chain) * e_abs)):.3f}"
              + (f", D err/bound {float(d_err / (R.gamma(chain) * d_abs)):.3f}" if periods > 1 else ""))
        assert e_err <= R.gamma(chain) * e_abs
        assert d_err <= R.gamma(chain) * d_abs
        if periods == 1:
            assert sums[c, 1] == 0.0
    # the same bytes from a second call, and from every channel run alone in buffers at another phase of the gaps
    rows2, sums2 = fold(eng, chans, begins, order, periods)
    assert np.array_equal(_words(sums2), _words(sums)) and np.array_equal(_words(rows2), _words(rows))
    for c in range(len(chans)):
        ra, sa = fold(eng, [chans[c]], [begins[c]], order, periods, phase=c + 1)
        assert np.array_equal(_words(sa[0]), _words(sums[c])) and np.array_equal(_words(ra[0]), _words(rows[c])), \
            f"channel {c}: alone and in the batch differ"


# -------------------------------------------------------------------------------------------------------------- finish
@pytest.mark.parametrize("periods", [1, 2, 5])
@pytest.mark.parametrize("order", [2, 5, T + 1])
def test_finish_bit_for_bit(eng, order, periods):
    from audio_analysis_amd.engine import mls_tables
    p, nb = (1 << order) - 1, 3
    _, out = mls_tables(order)
    rng = np.random.default_rng(7 * order + periods)
    wt = rng.standard_normal((nb, 1 << order)) * np.exp2(rng.integers(-30, 30, (nb, 1 << order)).astype(np.float64))
    wt[1, 3] = np.nan
    lh = Flat([p] * nb, np.float32, phase=order)               # exactly P floats a channel: the gaps must stay untouched
    w, h = _dev(eng, wt.reshape(-1)), _dev(eng, lh.filled())
    od, hoff = _dev(eng, np.ascontiguousarray(out)), _dev(eng, np.array(lh.off, np.int64))
    rc = eng.lib.ira_mls_finish(w.data_ptr(), od.data_ptr(), nb, order, periods, h.data_ptr(), hoff.data_ptr(), eng.stream)
    assert rc == IRA_OK
    got = lh.split(h.cpu().numpy(), f"ira_mls_finish order {order} R {periods}")
    assert np.array_equal(_words(w.cpu().numpy()), _words(wt.reshape(-1)))
    for c in range(nb):
        ref = R.finish(wt[c], out, order, periods)[1]
        same = (_words(got[c]) == _words(ref)) | (np.isnan(got[c]) & np.isnan(ref))
        assert same.all(), f"channel {c}: {int((~same).sum())} samples differ"
