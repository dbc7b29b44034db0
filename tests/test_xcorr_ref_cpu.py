"""
CPU-only tests of xcorr_ref.py, the references test_gpu_xcorr_kernels.py holds ira_xcorr.hip to: the exact integer sums
against the long-double restatement, the restatement against a closed form, the restated kernel shape against the facts
the kernel's LDS layout relies on, and the case builder against the row counts and loop branches it is there to reach.
The last group is the condition under which the GPU sweep cannot silently miss a shape; it reads no kernel output.
"""
import numpy as np
import pytest

import xcorr_ref as X

CH = X.CH
SWEEP = range(1, X.TREF + 1)


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("tmax", [1, 13, 128])
def test_exact_sums_equal_the_restatement_on_integer_data(tmax):
    rng = np.random.default_rng(7)
    for n, o, limits in ((300, 0, [1, 7, 7, 120]), (CH + 40, 5, [CH - 1, CH + 9]), (90, 89, [1]), (50, 3, [20, 400])):
        l = rng.integers(-127, 128, n).astype(np.float32)
        r = rng.integers(-127, 128, n).astype(np.float32)
        want = X.ref_sums(l, r, o, limits, tmax)
        got = X.exact_sums(l, r, o, limits, tmax)
        assert got.shape == want.shape == (len(limits) + 1, 2 * tmax + 3)
        assert np.array_equal(got.astype(X.LD), want), (tmax, n, o)
        pre = X.exact_prefix(l, r, o)
        assert np.array_equal(X.exact_sums(l, r, o, limits, tmax, prefix=pre), got)


def test_exact_sums_clamp_limits_and_onsets_as_the_header_states():
    rng = np.random.default_rng(8)
    n = 400
    l = rng.integers(-127, 128, n).astype(np.float32)
    r = rng.integers(-127, 128, n).astype(np.float32)
    whole = X.exact_sums(l, r, 3, [n], 5)[0]
    assert X.partition_edges([200, 50], 397) == [(0, 200), (200, 200), (50, 397)]
    assert X.partition_edges([-3, 100], 397) == [(0, 0), (0, 100), (100, 397)]
    assert X.partition_edges([500, 100], 397) == [(0, 397), (397, 397), (100, 397)]
    got = X.exact_sums(l, r, 3, [-3, 100], 5)
    assert not got[0].any() and np.array_equal(got[1] + got[2], whole)
    for o in (-1, n, n + 5, n + CH):                                      # no rows: every partition is zeros
        assert X.segment_rows(n, o) == 0 and not X.exact_sums(l, r, o, [1, 5], 5).any()
    last = X.exact_sums(l, r, n - 1, [1, 5], 2)                           # the last sample alone
    li, ri = l.astype(np.float64), r.astype(np.float64)
    assert list(last[0]) == [li[-1] * ri[-3], li[-1] * ri[-2], li[-1] * ri[-1], 0.0, 0.0, li[-1] ** 2, ri[-1] ** 2]
    assert not last[1:].any()


def test_restatement_of_a_delayed_copy_gives_the_closed_form():
    """r[n] = 0.5 l[n - d], the last T samples of l zero: C(d) = 0.5 El and Er = 0.25 El over the whole segment, and
    C(tau) of white integer l elsewhere is the autocorrelation at tau - d, far below El."""
    rng = np.random.default_rng(9)
    n, d, tmax = 3000, 17, 48
    l = rng.integers(-127, 128, n).astype(np.float32)
    l[-tmax:] = 0.0
    r = np.zeros_like(l)
    r[d:] = np.float32(0.5) * l[:-d]
    s = X.ref_sums(l, r, 0, [1000], tmax)
    tot = s[0] + s[1]
    el = np.sum(l.astype(X.LD) ** 2)
    assert tot[tmax + d] == X.LD(0.5) * el and tot[2 * tmax + 1] == el and tot[2 * tmax + 2] == X.LD(0.25) * el
    iacc, tau, _ = X.ref_coefficient(tot.astype(np.float64))
    assert tau == d and abs(iacc - 1.0) <= 4 * np.finfo(np.float64).eps
    # the same pair through the bound: the reference is the restatement, the bound scales with the rows of a partition
    ref, bnd = X.bounds(l, r, 0, [1000], tmax)
    assert np.array_equal(ref, s)
    mag = X.ref_sums(np.abs(l), np.abs(r), 0, [1000], tmax)
    assert np.array_equal(bnd[0], X.LD(1004 * X.U) * mag[0]) and np.array_equal(bnd[1], X.LD(2004 * X.U) * mag[1])
    with pytest.raises(AssertionError):
        X.bounds(np.ones(9000, np.float32), np.ones(9000, np.float32), 0, [8999], 1)   # a partition above 8192 rows


# ------------------------------------------------------------------------------------------------ the kernel's shape
def test_shape_sweep_has_61_shapes_inside_the_lds_layout():
    shapes = [X.shape(t) for t in SWEEP]
    assert len({s.key for s in shapes}) == 61
    for s in shapes:
        assert s.lpt in (9, 11, 13) and s.w >= s.nlag and s.w - s.nlag < s.lpt
        assert s.ngroups <= 29                                            # the kernel's comment on nsub
        assert s.nsub * s.w <= 512 * 13                                   # the partials fit below wsum
        assert 0 <= s.idle <= 26 and s.idle == X.THREADS - s.ngroups * s.nsub
    assert X.CH == 4096 and X.THREADS == 512
    assert [X.shape(t).key for t in (1, 48, 128)] == [(9, 1, 512), (11, 9, 56), (13, 20, 25)]   # what test_gpu_iacc.py runs
    assert [X.shape(t).key for t in (44, 96, 13, 121)] == [(9, 10, 51), (13, 15, 34), (9, 3, 170), (9, 27, 18)]
    assert X.shape(121).idle == 26 and X.shape(13).idle == 2
    s = X.shape(48)
    assert s.sub_len(1) == 1 and s.sub_len(56) == 1 and s.sub_len(57) == 3 and s.sub_len(4096) == 75
    rows = s.sub_ranges(4096)
    assert len(rows) == 56 and sum(n for n, _, _ in rows) == 4096 and rows[0] == (75, 6, 9) and rows[54] == (46, 4, 2)
    assert rows[55] == (0, 0, 0)


# ------------------------------------------------------------------------------------------------ the case builder
def _segment_pieces(tmax):
    for launch in X.cases(tmax):
        for seg in launch.segments:
            o = X.segment_onset(launch, seg)
            yield launch, seg, o, X.pieces(seg.l.size - o, seg.limits)


def test_cases_meet_every_required_row_count_limit_and_onset():
    for tmax in SWEEP:
        launches = X.cases(tmax)
        assert [la.nlim for la in launches] == [1, 2, 3, 4] and all(la.segments for la in launches)
        rows, onsets, flags = set(), set(), set()
        for launch, seg, o, pcs in _segment_pieces(tmax):
            n = seg.l.size
            length = n - o
            assert seg.r.size == n <= 2 * CH + tmax + 1 and len(seg.limits) == launch.nlim and 0 <= o < n
            assert seg.l.dtype == seg.r.dtype == np.float32
            assert all(b - a <= X.MAX_ROWS_BOUND for a, b in X.partition_edges(seg.limits, length))
            rows |= {p[3] for p in pcs}
            onsets.add((int(launch.onsets[seg.lchan]), int(launch.onsets[seg.rchan])))
            lim = seg.limits
            flags |= {("limit", v - CH) for v in lim if abs(v - CH) <= 1}
            flags |= {"past L"} if lim[-1] > length else set()
            flags |= {"equal"} if any(a == b for a, b in zip(lim, lim[1:])) else set()
            flags |= {"mid-chunk piece"} if any(p[2] > 0 and p[3] > 1 for p in pcs) else set()
            flags |= {"second chunk"} if any(p[0] == 1 for p in pcs) else set()
        assert set(X.required_rows(tmax)) <= rows, (tmax, sorted(set(X.required_rows(tmax)) - rows))
        assert {(0, 0), (1, 1), (CH - 1, CH - 1), (CH, CH)} <= onsets and any(a != b for a, b in onsets)
        assert flags >= {("limit", -1), ("limit", 0), ("limit", 1), "past L", "equal", "mid-chunk piece", "second chunk"}
        used = [(s.lchan, s.rchan) for s in launches[3].segments]           # a channel entry shared by two segments
        assert len(used) > len(set(used))


def test_cases_meet_every_branch_of_every_lags_per_thread_variant():
    seen = {9: set(), 11: set(), 13: set()}
    nsubs = set()
    for tmax in SWEEP:
        s = X.shape(tmax)
        nsubs.add(s.nsub)
        for _, _, _, pcs in _segment_pieces(tmax):
            for _, _, _, rows in pcs:
                sl = s.sub_len(rows)
                for n, bodies, rem in s.sub_ranges(rows):
                    if n == 0:
                        seen[s.lpt].add("empty sub-range")
                        continue
                    seen[s.lpt].add("body and remainder" if bodies and rem else "body only" if bodies else "remainder only")
                    if n < sl:
                        seen[s.lpt].add("cut short")
    want = {"remainder only", "body only", "body and remainder", "cut short", "empty sub-range"}
    for lpt, got in seen.items():
        assert got == want, (lpt, want - got)
    assert any(n < 64 for n in nsubs) and any(n > 64 for n in nsubs)
    assert any(n % 8 == 0 for n in nsubs) and any(n % 8 for n in nsubs)
    assert any(n > 64 and n % 8 for n in nsubs) and any(n < 64 and n % 8 for n in nsubs)


def test_integer_cases_stay_below_2_53_and_are_deterministic():
    for tmax in (1, 44, 128):
        for launch, again in zip(X.cases(tmax), X.cases(tmax)):
            for seg, twin in zip(launch.segments, again.segments):
                assert np.array_equal(seg.l, twin.l) and np.array_equal(seg.r, twin.r) and seg.limits == twin.limits
                assert max(np.max(np.abs(seg.l)), np.max(np.abs(seg.r))) <= X.MAX_INT
                assert np.array_equal(seg.l, np.rint(seg.l)) and seg.l.size <= X.MAX_ROWS_EXACT
                # the largest magnitude any partial sum of any subset of the rows can take
                assert seg.l.size * X.MAX_INT ** 2 < 1 << 53
    noise = X.cases(13, "noise")[3].segments[1]
    assert noise.l.size == 2 * CH + 14 and not np.array_equal(noise.l, np.rint(noise.l))
