"""ira_mls_fold, ira_mls_hadamard and ira_mls_finish (ira_mls.hip) called through the C-ABI, each alone, on buffers this file
owns, against the restatement of tests/mls_ref.py.  Every buffer a launch writes is a guarded flat buffer
(tests/guard_buffers.py): every guard must come back untouched, and every input buffer unchanged.  The cases, their inputs
and the assertions live in tests/mls_kernels_ref.py; tests/test_mls_kernels_ref_cpu.py shows there, without a GPU, that an
emulation of the kernels as written passes them and that named wrong kernels (a stage dropped or run out of turn at a round
boundary, a missing hi term, a wrong row offset, a missing stride loop ..) fall at cases of these tables.

Held to the bit: the transform of random float64 rows (signed zeros, denormals, a row with a NaN) at every order 2 .. 21,
i.e. every way the plan splits the stages into rounds (T = 12: orders up to 12 one pass, 13 .. 20 two with a = 1 .. 8 high
bits, 21 three), and of unit impulses, whose transforms are Walsh rows exactly; Y through G and w[0] = 0; the float32
response; all of it again with tables that carry a stray bit above the mask.  E and D are held to the long-double sums of the
float64 terms the kernel forms (restated one by one, so only the order of the additions is open) within gamma_c times the
sum of the terms, c = engine.mls_sum_chain: the longest chain of additions of the kernel's reduction, restated in
mls_kernels_ref.sum_chain from its block sizes.

Not launched: r P >= 2^31 in the fold's sample offset needs order 21 with more than 1000 periods, 8 GB of samples.  The
offset is formed as (int64_t)r * p_len + n in both sweeps of mls_fold_kernel, and the rows as (int64_t)e << order in all
four kernels; that was verified by reading only.

Measured on an MI355X: every transform equal to the bit (orders 2 .. 20 at 1 and 3 channels, 2 .. 13 at 65 as well, order 21 at
1 and 2) and every unit impulse's transform its Walsh row (m + 1 impulses an order); every fold and response equal to the
bit (the fold at orders 2, 5, 13, 16, 17 at 4 channels, 21 at 2, 3 at 65 and 130, R up to 1024; the finish at orders 2, 5,
13, 16 at 3 channels and 21 at 1, R up to 1024), the stray-bit tables included; no guard and no spare row touched; E at
0.149 and D at 0.158 of their bounds at worst, both at order 3 with 130 channels (0.119 and 0.083 over the 4-channel
cases; the test prints each).
"""
import numpy as np
import pytest

import mls_kernels_ref as K
import mls_ref as R
from guard_buffers import Flat, to_device as _dev, words as _words

pytestmark = pytest.mark.gpu
IRA_OK = 0
T = K.T                                           # the tile order of ira_mls_hadamard
_rows = K.rows


@pytest.fixture(scope="module")
def eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def _case_id(case, usual_nb):
    """order-periods, with the channel count behind it where it is not the usual one."""
    return "-".join(str(v) for v in (case[:2] if case[2] == usual_nb else case))


def hadamard(eng, w, order):
    nb = w.shape[0]
    lay = Flat([w.size], np.float64, phase=order)
    buf = _dev(eng, lay.filled([w.reshape(-1)]))
    rc = eng.lib.ira_mls_hadamard(buf.data_ptr() + 8 * lay.off[0], nb, order, eng.stream)
    assert rc == IRA_OK
    return lay.split(buf.cpu().numpy(), f"ira_mls_hadamard order {order} nb {nb}")[0].reshape(nb, -1)


@pytest.mark.parametrize("order,nb", K.HADAMARD_CASES)
def test_hadamard_bit_for_bit(eng, order, nb):
    from audio_analysis_amd.engine import mls_pass_plan
    assert T == 12 and len(mls_pass_plan(order)) == (1 if order <= T else 2 if order <= T + 8 else 3)
    w = K.hadamard_input(order, nb)
    K.check_hadamard(hadamard(eng, w, order), w, order)


def test_hadamard_three_passes(eng):
    from audio_analysis_amd.engine import mls_pass_plan
    assert mls_pass_plan(21) == [(0, 12), (12, 5), (17, 4)]                # the smallest order with three passes
    w = _rows(np.random.default_rng(21), 1, 21)
    got = hadamard(eng, w, 21)
    assert np.array_equal(_words(got), _words(R.fwht(w)))


@pytest.mark.parametrize("order", K.ORDERS)
def test_hadamard_of_unit_impulses_gives_walsh_rows(eng, order):
    """The impulse at i transforms to (-1)^popcount(i & k) exactly, a reference that owes nothing to mls_ref.fwht; i runs
    over 1, every power of two and 2^m - 1, at most 32 MB of rows a launch."""
    idx = K.probe_indices(order)
    per = max(1, (1 << 22) >> order)
    for at in range(0, len(idx), per):
        part = idx[at : at + per]
        K.check_probes(hadamard(eng, K.probe_rows(order, part), order), order, part, "ira_mls_hadamard")


# ---------------------------------------------------------------------------------------------------------------- fold
def fold(eng, chans, begins, order, periods, phase=0, g=None, spare=0):
    """One launch over channels laid out with guards and gaps: (w rows, sums (nb, 2)).  `spare` rows lie behind the
    workspace inside its segment; no launch may write them."""
    from audio_analysis_amd.engine import mls_fold_blocks, mls_tables
    nb = len(chans)
    g = mls_tables(order)[0] if g is None else g
    lx = Flat([c.size for c in chans], np.float32, phase)
    lw, ls = Flat([(nb + spare) << order], np.float64, phase), Flat([2 * nb], np.float64, phase + 1)
    lsc = Flat([2 * nb * mls_fold_blocks(order)], np.float64, phase + 2)
    x_host = lx.filled(chans)
    x, w, s, sc = _dev(eng, x_host), _dev(eng, lw.filled()), _dev(eng, ls.filled()), _dev(eng, lsc.filled())
    beg = _dev(eng, np.array([o + b for o, b in zip(lx.off, begins)], np.int64))
    gd = _dev(eng, np.ascontiguousarray(g))
    rc = eng.lib.ira_mls_fold(x.data_ptr(), beg.data_ptr(), nb, order, periods, gd.data_ptr(), w.data_ptr() + 8 * lw.off[0],
                              s.data_ptr() + 8 * ls.off[0], sc.data_ptr() + 8 * lsc.off[0], eng.stream)
    assert rc == IRA_OK
    what = f"ira_mls_fold order {order} R {periods}"
    rows = lw.split(w.cpu().numpy(), what + " w")[0].reshape(nb + spare, -1)
    sums = ls.split(s.cpu().numpy(), what + " sums")[0].reshape(nb, 2)
    lsc.split(sc.cpu().numpy(), what + " scratch")
    assert np.array_equal(_words(x.cpu().numpy()), _words(x_host)), what + ": the samples were written"
    return rows, sums


@pytest.mark.parametrize("order,periods,nb", K.FOLD_CASES, ids=[_case_id(c, 4) for c in K.FOLD_CASES])
def test_fold_bits_and_sums(eng, order, periods, nb):
    """Orders 16, 17 and 21 give a thread 2, 4 and 64 samples of the grid-stride loop; 1024 is the most periods a call takes;
    65 and 130 channels reach the second and third workgroup of the sums kernel.  r P >= 2^31 is not launched (8 GB of
    samples): the (int64_t) cast of that offset was verified by reading only."""
    from audio_analysis_amd.engine import MLS_FOLD_BLOCKS, MLS_FOLD_THREADS, mls_fold_blocks, mls_sum_chain, mls_tables
    p = (1 << order) - 1
    chans, begins = K.fold_input(order, periods, nb)
    rows, sums = fold(eng, chans, begins, order, periods)
    g, _ = mls_tables(order)
    # the longest chain of additions, from the kernel's block sizes: a thread's own terms, the wave tree (6), the 4 waves
    # (3), the workgroups of the channel
    blocks = min(-(-p // MLS_FOLD_THREADS), MLS_FOLD_BLOCKS)
    chain = -(-p // (blocks * MLS_FOLD_THREADS)) * periods + 6 + 3 + blocks
    assert blocks == mls_fold_blocks(order) and chain == mls_sum_chain(order, periods)
    assert (blocks, chain) == K.sum_chain(order, periods)
    e_rel, d_rel = K.check_fold(rows, sums, chans, begins, order, periods, g)
    print(f"order {order} R {periods} nb {nb}: worst E err/bound {e_rel:.3f}, worst D err/bound {d_rel:.3f}")
    # the same bytes from a second call, and from every channel run alone in buffers at another phase of the gaps
    rows2, sums2 = fold(eng, chans, begins, order, periods)
    assert np.array_equal(_words(sums2), _words(sums)) and np.array_equal(_words(rows2), _words(rows))
    for c in range(len(chans)):
        ra, sa = fold(eng, [chans[c]], [begins[c]], order, periods, phase=c + 1)
        assert np.array_equal(_words(sa[0]), _words(sums[c])) and np.array_equal(_words(ra[0]), _words(rows[c])), \
            f"channel {c}: alone and in the batch differ"


# -------------------------------------------------------------------------------------------------------------- finish
def finish(eng, wt, out, nb, order, periods):
    """One launch on the first nb rows of wt: [P float32 per channel], exactly P floats a channel in a guarded buffer."""
    p = (1 << order) - 1
    lh = Flat([p] * nb, np.float32, phase=order)               # exactly P floats a channel: the gaps must stay untouched
    w, h = _dev(eng, wt.reshape(-1)), _dev(eng, lh.filled())
    od, hoff = _dev(eng, np.ascontiguousarray(out)), _dev(eng, np.array(lh.off, np.int64))
    rc = eng.lib.ira_mls_finish(w.data_ptr(), od.data_ptr(), nb, order, periods, h.data_ptr(), hoff.data_ptr(), eng.stream)
    assert rc == IRA_OK
    got = lh.split(h.cpu().numpy(), f"ira_mls_finish order {order} R {periods}")
    assert np.array_equal(_words(w.cpu().numpy()), _words(wt.reshape(-1)))
    return got


@pytest.mark.parametrize("order,periods,nb", K.FINISH_CASES, ids=[_case_id(c, 3) for c in K.FINISH_CASES])
def test_finish_bit_for_bit(eng, order, periods, nb):
    """From order 16 on the stride loop iterates (P > 128 x 256)."""
    from audio_analysis_amd.engine import mls_tables
    _, out = mls_tables(order)
    wt = K.finish_input(order, periods, nb)
    K.check_finish(finish(eng, wt, out, nb, order, periods), wt, out, order, periods)


# ------------------------------------------------------------------------------------------------------- table masking
@pytest.mark.parametrize("order,nb", K.MASK_CASES)
def test_stray_table_bits_are_masked(eng, order, nb):
    """The promise of the file's header: every table value is masked to m bits before it indexes a row.  Bit m alone is
    set in a seeded third of G's and out's entries; an unmasked index then lands one row further, at worst in the spare
    row this test owns behind the workspace, inside the allocation and in front of the guard.  The results equal the
    clean-table launch to the bit and the spare row keeps its sentinel."""
    from audio_analysis_amd.engine import mls_tables
    g, out = mls_tables(order)
    gs, outs = K.stray(g, order, order), K.stray(out, order, order + 1)
    assert (gs != g).any() and (outs != out).any() and np.array_equal(gs & ((1 << order) - 1), g)
    chans, begins = K.fold_input(order, 2, nb)
    rows, sums = fold(eng, chans, begins, order, 2, spare=1)
    rows_s, sums_s = fold(eng, chans, begins, order, 2, g=gs, spare=1)
    assert np.array_equal(_words(rows_s), _words(rows)) and np.array_equal(_words(sums_s), _words(sums))
    K.check_guard(rows_s[nb], "ira_mls_fold: the spare row behind the workspace")
    K.check_fold(rows_s[:nb], sums_s, chans, begins, order, 2, g)
    wt = np.concatenate([K.finish_input(order, 2, nb), K.rows(np.random.default_rng(order), 1, order)])
    clean, masked = finish(eng, wt, out, nb, order, 2), finish(eng, wt, outs, nb, order, 2)
    assert all(np.array_equal(_words(a), _words(b)) for a, b in zip(clean, masked))
    K.check_finish(masked, wt[:nb], out, order, 2)
