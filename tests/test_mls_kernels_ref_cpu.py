"""tests/mls_kernels_ref.py on a machine without a GPU: the schedule of ira_mls_hadamard stages every bit once, ascending,
at every order; an honest NumPy emulation of the kernels of ira_mls.hip passes every case of the tables
tests/test_gpu_mls_kernels.py launches; every subtly wrong kernel modelled there is rejected by the case named beside it;
and the one deviation no case can reject -- the nine high bits of order 21 split 8 + 1 -- is asserted to give the same bits."""
import numpy as np
import pytest

import mls_kernels_ref as K
import mls_ref as R
from guard_buffers import words


def tables(order):
    from audio_analysis_amd.engine import mls_tables
    return mls_tables(order)


# -------------------------------------------------------------------------------------------------------- the schedule
@pytest.mark.parametrize("order", K.ORDERS)
def test_schedule_stages_every_bit_once_ascending(order):
    from audio_analysis_amd.engine import mls_pass_plan
    sched = K.schedule(order)
    assert [b for _, _, bits in sched for b in bits] == list(range(order))
    assert [k for k, _, _ in sched] == sorted(k for k, _, _ in sched) and {k for k, _, _ in sched} == set(range(len(mls_pass_plan(order))))
    assert all(1 <= len(bits) <= K.REG_BITS and base <= K.COAL for _, base, bits in sched)


def test_the_rounds_of_the_further_pass_differ_with_a():
    """What makes orders 14 .. 20 worth launching: almost every a splits its stages into rounds of its own."""
    shape = {a: [(base, len(regs)) for base, regs in K.rounds(K.T - a, K.T)] for a in range(1, 9)}
    assert shape == {1: [(8, 1)], 2: [(8, 2)], 3: [(8, 3)], 4: [(8, 4)], 5: [(7, 4), (8, 1)], 6: [(6, 4), (8, 2)],
                     7: [(5, 4), (8, 3)], 8: [(4, 4), (8, 4)]}
    low = {m: [(base, len(regs)) for base, regs in K.rounds(0, m)] for m in (5, 7, 9, 10, 12)}
    assert low == {5: [(0, 4), (4, 1)], 7: [(0, 4), (4, 3)], 9: [(0, 4), (4, 4), (8, 1)], 10: [(0, 4), (4, 4), (8, 2)],
                   12: [(0, 4), (4, 4), (8, 4)]}
    assert (K.T, K.THREADS, K.FOLD_THREADS, K.FOLD_BLOCKS, K.MAX_PERIODS) == (12, 256, 256, 128, 1024)


# ------------------------------------------------------------------------------------------------------- the transform
def judge_hadamard(order, nb, wrong=None, plan=None):
    w = K.hadamard_input(order, nb)
    got, tail = K.emulate(w, order, wrong, plan)
    K.check_guard(tail, f"ira_mls_hadamard order {order} nb {nb}")
    K.check_hadamard(got, w, order)


def rejected(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("order", K.ORDERS)
def test_the_honest_transform_equals_fwht_on_every_case(order):
    cases = [c for c in K.HADAMARD_CASES if c[0] == order]
    assert cases
    for m, nb in cases:
        judge_hadamard(m, nb)


@pytest.mark.parametrize("order", K.ORDERS)
def test_the_honest_transform_gives_the_walsh_rows(order):
    idx = K.probe_indices(order)
    assert len(idx) == order + 1 and idx[0] == 1 and idx[-1] == (1 << order) - 1
    if order > 17:                                     # the emulation is slow there: the lowest bit, the highest and all of them
        idx = [1, 1 << (order - 1), (1 << order) - 1]
    per = max(3, (1 << 22) >> order)                                       # 32 MB of rows at a time
    for at in range(0, len(idx), per):
        got, _ = K.emulate(K.probe_rows(order, idx[at : at + per]), order)
        K.check_probes(got, order, idx[at : at + per])
    assert np.array_equal(K.walsh_row(3, 5), [1, -1, 1, -1, -1, 1, -1, 1])
    assert np.array_equal(K.walsh_row(order, idx[-1]), R.fwht(K.probe_rows(order, idx[-1:]))[0])


# (wrong, (order, nb), why): each case is one HADAMARD_CASES holds, i.e. one the GPU file launches
HADAMARD_REJECTS = (
    [("drop_top", (m, 1), "a partial round of the first pass without its top stage") for m in (5, 7, 9, 10)]
    + [("drop_top", (K.T + a, 1), f"a partial round of the further pass, a = {a}, without its top stage") for a in (2, 3, 6, 7)]
    + [("guard_dropped", (5, 65), "had_stage<3> without `base + 3 < end`: bit 7 of a tile of order-5 rows"),
       ("guard_dropped", (10, 3), "had_stage<3> without `base + 3 < end`: bit 11 joins rows 0 and 2"),
       ("descending", (12, 1), "the stages of a round descending: equal values, other roundings"),
       ("descending", (16, 1), "the stages of a round descending: equal values, other roundings"),
       ("unclamped_base", (14, 1), "the further pass's round at base 10"),
       ("unclamped_base", (15, 1), "the further pass's round at base 9"),
       ("ignore_hi", (21, 1), "no hi << (lo + a): every group of 32 points lands on the first"),
       ("row_shift_12", (14, 3), "rows offset by << 12"),
       ("row_shift_12", (21, 2), "rows offset by << 12"),
       ("store_whole_tile", (5, 3), "the first pass stores its zero fill behind the rows"),
       ("store_whole_tile", (11, 65), "the first pass stores its zero fill behind the rows")])


@pytest.mark.parametrize("wrong,case,why", HADAMARD_REJECTS, ids=[f"{w}-{c[0]}x{c[1]}" for w, c, _ in HADAMARD_REJECTS])
def test_a_wrong_transform_is_rejected_by_its_case(wrong, case, why):
    assert wrong in K.HADAMARD_WRONG and case in K.HADAMARD_CASES
    assert rejected(judge_hadamard, *case, wrong=wrong), why


def test_where_a_wrong_transform_cannot_show():
    """Why the case lists are what they are: the deviations below are invisible at the cases named here, so the cases above
    are the ones that carry them."""
    judge_hadamard(5, 3, wrong="guard_dropped")        # bit 7 of a tile with 96 doubles in it pairs every value with a zero
    judge_hadamard(12, 65, wrong="guard_dropped")      # no partial round
    judge_hadamard(16, 1, wrong="drop_top")            # a = 4: one full round
    judge_hadamard(20, 3, wrong="ignore_hi")           # two passes: hi is 0 by construction
    judge_hadamard(16, 3, wrong="unclamped_base")      # cbits <= 8: the clamp does nothing
    judge_hadamard(14, 1, wrong="row_shift_12")        # one row: no offset
    judge_hadamard(13, 1, wrong="store_whole_tile")    # nb 2^m a multiple of the tile


def test_descending_stages_differ_by_rounding_alone():
    w = K.hadamard_input(12, 1)
    a, b = K.emulate(w, 12)[0], K.emulate(w, 12, "descending")[0]
    differ = words(a) != words(b)
    assert differ.any()
    assert np.max(np.abs(a - b)) <= 2.0 * R.gamma(12) * np.abs(w).sum()
    ints = np.rint(w * 2.0 ** 20) % 1024.0                                  # integers: nothing rounds, nothing differs
    assert np.array_equal(K.emulate(ints, 12)[0], K.emulate(ints, 12, "descending")[0])


def test_the_probes_name_the_missing_stage():
    for order, bit in ((5, 4), (10, 9), (15, 14)):
        idx = K.probe_indices(order)
        got, _ = K.emulate(K.probe_rows(order, idx), order, "drop_top")
        # a missing stage spoils every probe, bit 0's first; the butterfly relations of that probe name the stage
        with pytest.raises(AssertionError, match=rf"lowest bit whose probe differs: 0; stages broken in the probe at 1: \[{bit}\]$"):
            K.check_probes(got, order, idx)


def test_splitting_nine_high_bits_8_and_1_cannot_be_rejected():
    """(12, 8), (20, 1) in place of (12, 5), (17, 4) runs the same stages in the same order on the same pairs: the bits are
    the same, so no case pins the split.  What the suite pins is the stage order; the split is a matter of speed."""
    from audio_analysis_amd.engine import mls_pass_plan
    other = [(0, 12), (12, 8), (20, 1)]
    assert mls_pass_plan(21) == [(0, 12), (12, 5), (17, 4)]
    assert [b for _, _, bits in K.schedule(21, other) for b in bits] == list(range(21))
    for nb in (1, 2):
        assert (21, nb) in K.HADAMARD_CASES
        w = K.hadamard_input(21, nb)
        a, b = K.emulate(w, 21)[0], K.emulate(w, 21, plan=other)[0]
        assert np.array_equal(words(a), words(b))              # and the honest bits are fwht's (tested above)


# ------------------------------------------------------------------------------------------------------ fold and finish
def judge_fold(order, periods, nb, wrong=None):
    from audio_analysis_amd.engine import mls_fold_blocks, mls_sum_chain
    chans, begins = K.fold_input(order, periods, nb)
    g, _ = tables(order)
    assert K.sum_chain(order, periods) == (mls_fold_blocks(order), mls_sum_chain(order, periods))
    rows, sums, tail = K.emu_fold(chans, begins, order, periods, g, wrong)
    K.check_guard(tail, f"ira_mls_fold order {order} R {periods}")
    return K.check_fold(rows, sums, chans, begins, order, periods, g, show=lambda s: None)


def judge_finish(order, periods, nb, wrong=None):
    _, out = tables(order)
    wt = K.finish_input(order, periods, nb)
    K.check_finish(K.emu_finish(wt, out, order, periods, wrong), wt, out, order, periods)


@pytest.mark.parametrize("case", K.FOLD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_the_honest_fold_passes_every_case(case):
    e, d = judge_fold(*case)
    assert e <= 1.0 and d <= 1.0


@pytest.mark.parametrize("case", K.FINISH_CASES, ids=lambda c: "x".join(map(str, c)))
def test_the_honest_finish_passes_every_case(case):
    judge_finish(*case)


def test_the_strided_cases_are_strided():
    """What the new cases are for: samples per thread, the first term of the chain, the workgroups of the sums kernel."""
    per_thread = lambda m: -(-((1 << m) - 1) // (K.FOLD_BLOCKS * K.FOLD_THREADS))
    assert [per_thread(m) for m in (13, 15, 16, 17, 21)] == [1, 1, 2, 4, 64]
    assert K.sum_chain(21, 2) == (128, 64 * 2 + 9 + 128) and K.sum_chain(2, 1024) == (1, 1024 + 9 + 1)
    assert {m for m, _, _ in K.FOLD_CASES} >= {16, 17, 21} and {m for m, _, _ in K.FINISH_CASES} >= {16, 21}
    assert -(-65 // K.WAVE) == 2 and -(-130 // K.WAVE) == 3
    assert max(r for _, r, _ in K.FOLD_CASES) == K.MAX_PERIODS == max(r for _, r, _ in K.FINISH_CASES)
    # nothing above 40 MB a buffer
    assert all(nb * (r * (1 << m) * 4) <= 40e6 and (nb << m) * 8 <= 40e6 for m, r, nb in K.FOLD_CASES)
    assert all((nb << m) * 8 <= 40e6 for m, nb in K.HADAMARD_CASES) and all((nb << m) * 8 <= 40e6 for m, _, nb in K.FINISH_CASES)


FOLD_REJECTS = (("block_stride", (K.T + 1, 2, 4), "n += 256: every workgroup folds the samples of those behind it into E and D"),
                ("uncapped_blocks", (16, 1, 4), "the sums kernel reads ceil(P / 256) = 256 partials a channel"),
                ("uncapped_blocks", (21, 2, 2), "the sums kernel reads ceil(P / 256) = 8192 partials a channel"))
FINISH_REJECTS = (("no_stride", (16, 2, 3), "k >= 32768 never written"), ("no_stride", (21, 1, 1), "k >= 32768 never written"))


@pytest.mark.parametrize("wrong,case,why", FOLD_REJECTS, ids=[f"{w}-{'x'.join(map(str, c))}" for w, c, _ in FOLD_REJECTS])
def test_a_wrong_fold_is_rejected_by_its_case(wrong, case, why):
    assert wrong in K.FOLD_WRONG and case in K.FOLD_CASES
    assert rejected(judge_fold, *case, wrong=wrong), why


@pytest.mark.parametrize("wrong,case,why", FINISH_REJECTS, ids=[f"{w}-{'x'.join(map(str, c))}" for w, c, _ in FINISH_REJECTS])
def test_a_wrong_finish_is_rejected_by_its_case(wrong, case, why):
    assert wrong in K.FINISH_WRONG and case in K.FINISH_CASES
    assert rejected(judge_finish, *case, wrong=wrong), why
    judge_finish(K.T + 1, 2, 3, wrong=wrong)                               # one sample a thread: nothing to see


def test_the_uncapped_block_count_needs_order_16():
    judge_fold(K.T + 1, 2, 4, wrong="uncapped_blocks")                     # 32 workgroups: the cap does nothing
    assert -(-((1 << 15) - 1) // K.FOLD_THREADS) == K.FOLD_BLOCKS < -(-((1 << 16) - 1) // K.FOLD_THREADS)


# ---------------------------------------------------------------------------------------------------- the table masking
@pytest.mark.parametrize("order,nb", K.MASK_CASES)
def test_stray_table_bits_change_nothing_unless_the_mask_is_missing(order, nb):
    """The launch of the GPU file: tables with bit m set in a third of their entries, a spare row behind the workspace.  The
    masked kernels give the clean launch's bits and leave the spare row alone; unmasked ones write into it (fold) or read
    from the next row (finish)."""
    g, out = tables(order)
    gs, outs = K.stray(g, order, order), K.stray(out, order, order + 1)
    p = (1 << order) - 1
    for tab, st in ((g, gs), (out, outs)):
        hit = st != tab
        assert 0.25 < hit.mean() < 0.42 and np.array_equal(st & p, tab) and np.all(st[hit] == tab[hit] + p + 1)
    chans, begins = K.fold_input(order, 2, nb)
    clean = K.emu_fold(chans, begins, order, 2, g, spare=1)
    masked = K.emu_fold(chans, begins, order, 2, gs, spare=1)
    assert all(np.array_equal(words(a), words(b)) for a, b in zip(clean, masked))
    K.check_guard(masked[0][nb], "the spare row")
    bare = K.emu_fold(chans, begins, order, 2, gs, "unmasked", spare=1)
    assert rejected(K.check_guard, bare[0][nb], "the spare row") and not np.array_equal(words(bare[0][:nb]), words(clean[0][:nb]))
    wt = np.concatenate([K.finish_input(order, 2, nb), K.rows(np.random.default_rng(order), 1, order)])
    clean = K.emu_finish(wt, out, order, 2, nb=nb)
    masked = K.emu_finish(wt, outs, order, 2, nb=nb)
    bare = K.emu_finish(wt, outs, order, 2, "unmasked", nb=nb)
    assert all(np.array_equal(words(a), words(b)) for a, b in zip(clean, masked))
    assert not all(np.array_equal(words(a), words(b)) for a, b in zip(clean, bare))
    K.check_finish(masked, wt[:nb], out, order, 2)
