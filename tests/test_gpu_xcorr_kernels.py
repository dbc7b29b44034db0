"""
The two kernels of audio_analysis_amd/csrc/ira_xcorr.hip (ira_xcorr_windows: xcorr_partial_kernel at every max lag T,
xcorr_fold_kernel) on buffers the test owns, against the references of xcorr_ref.py.  test_gpu_iacc.py holds the feature at
T = 1, 48 and 128 to 1e-12 through the engine's pooled scratch; here every one of the 61 (LPT, ngroups, nsub) shapes runs,
and integer-valued samples are held bit for bit (exact_sums), rounding-sensitive ones to a derived bound (bounds).

Every launch (run below): the samples lie in one buffer with runs of NaN in front of, between and behind the channels,
at offsets of every residue mod 4; the scratch is exactly ira_xcorr_scratch_doubles(...) doubles at the front of a larger
NaN-filled tensor; out is NaN-filled between sentinel guards; all of them are made afresh for the launch.  Afterwards the
guards and the tensor past the scratch must be untouched and out must hold no NaN: one there is a record that was read but
never written, or a sample read from outside its file (test_cases_meet_* in test_xcorr_ref_cpu.py is the condition under
which the sweep reaches every loop branch of every shape).

Measured on an MI355X, worst |error| / bound of the rounding-sensitive test: see DESIGN.md 4.8.
"""
import numpy as np
import pytest

import guard_buffers as G
import xcorr_ref as X

pytestmark = pytest.mark.gpu

CH = X.CH
PAST = 1024                    # doubles behind the scratch, more than the three records of T = 128 an unclamped fold reads
Seg = X.Segment


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run(eng, tmax, nlim, onsets, segments, max_len=None, finite=True):
    """ira_xcorr_windows through the bound library.  Returns out (nseg, nlim + 1, 2T + 3) float64."""
    from audio_analysis_amd.engine import _ptr, check
    t = eng.torch
    nseg, nrec = len(segments), 2 * tmax + 3
    parts, offs, pos = [], [], 0
    for k, x in enumerate(c for s in segments for c in (s.l, s.r)):
        gap = 5 + (k * 7 + k // 4) % 4                        # offsets take every residue mod 4
        parts += [np.full(gap, np.nan, np.float32), np.asarray(x, dtype=np.float32)]
        offs.append(pos + gap)
        pos += gap + x.size
    parts.append(np.full(9, np.nan, np.float32))
    lens = [s.l.size for s in segments]
    assert all(s.r.size == n and len(s.limits) == nlim for s, n in zip(segments, lens))
    max_len = max(lens) if max_len is None else max_len
    nsc = int(eng.lib.ira_xcorr_scratch_doubles(nseg, max_len, nlim, tmax))
    assert nsc == nseg * (-(-max_len // CH) + nlim) * nrec
    dev = lambda a, dt: t.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(eng.device)   # noqa: E731
    x = dev(np.concatenate(parts), np.float32)
    d_lo, d_ro, d_len = dev(offs[0::2], np.int64), dev(offs[1::2], np.int64), dev(lens, np.int64)
    d_lc, d_rc = dev([s.lchan for s in segments], np.int32), dev([s.rchan for s in segments], np.int32)
    d_on, d_lim = dev(onsets, np.int64), dev([v for s in segments for v in s.limits], np.int64)
    big = t.full((nsc + PAST,), float("nan"), dtype=t.float64, device=eng.device)
    nout = nseg * (nlim + 1) * nrec
    host = np.concatenate([G.sentinel(G.GUARD, np.float64), np.full(nout, np.nan), G.sentinel(G.GUARD, np.float64)])
    out = dev(host, np.float64)
    check(eng.lib.ira_xcorr_windows(_ptr(x), _ptr(d_lo), _ptr(d_ro), _ptr(d_len), _ptr(d_lc), _ptr(d_rc), _ptr(d_on), nseg,
                                    max_len, _ptr(d_lim), nlim, tmax, _ptr(big), _ptr(out[G.GUARD:]), eng.stream),
          "ira_xcorr_windows")
    t.cuda.synchronize()
    back = out.cpu().numpy()
    assert G.untouched(back[: G.GUARD]) and G.untouched(back[G.GUARD + nout :]), "written outside out"
    assert bool(t.isnan(big[nsc:]).all()), "written past the scratch"
    res = back[G.GUARD : G.GUARD + nout].reshape(nseg, nlim + 1, nrec)
    if finite:
        assert not np.isnan(res).any(), ("NaN in out", np.argwhere(np.isnan(res))[:4].tolist())
    return res


def run_launch(eng, launch, **kw):
    return run(eng, launch.tmax, launch.nlim, launch.onsets, launch.segments, **kw)


def _ints(rng, n):
    return rng.integers(-X.MAX_INT, X.MAX_INT + 1, n).astype(np.float32)


# ------------------------------------------------------------------------------------------------ every max lag, exact
@pytest.mark.parametrize("t_first", range(1, X.TREF + 1, 8))
def test_every_max_lag_exact_on_integer_samples(t_first):
    eng = _eng()
    for tmax in range(t_first, t_first + 8):
        for launch in X.cases(tmax, "int"):
            got = run_launch(eng, launch)
            for i, seg in enumerate(launch.segments):
                want = X.exact_sums(seg.l, seg.r, X.segment_onset(launch, seg), seg.limits, tmax)
                bad = np.argwhere(_bits(got[i]) != _bits(want))
                assert bad.size == 0, (tmax, X.shape(tmax).key, launch.nlim, i, seg.limits, bad[:4].tolist())


# ------------------------------------------------------------------------------------------------ impulse rows, exact
@pytest.mark.parametrize("tmax", [1, 13, 44, 48, 96, 121, 128])
def test_impulse_rows_return_the_right_channel_sample_by_sample(tmax):
    """l a unit impulse at row i, r integer noise: C(tau) = r[o + i + tau] exactly, 0.0 outside the file, El = 1, Er the
    integer sum, in the partition that holds row i; zeros in the other.  Twelve one-impulse segments in one launch."""
    eng = _eng()
    rng = np.random.default_rng(100 + tmax)
    length, limit = CH + 2, CH + 1
    s0 = X.shape(tmax).sub_len(CH)                           # the sub-range length of the full first chunk
    rows = [0, s0 - 1, s0, CH - 1, CH, length - 1]           # ... the last row: its lags run off the end of the file
    onsets, segs, want = [], [], []
    for o in (0, tmax + 3):                                  # lags below 0 run off the front / read samples before the onset
        for i in rows:
            n = o + length
            l, r = np.zeros(n, np.float32), _ints(rng, n)
            l[o + i] = 1.0
            segs.append(Seg(l, r, len(onsets), len(onsets) + 1, [limit]))
            onsets += [o, o]
            rec = np.zeros((2, 2 * tmax + 3))
            j = int(i >= limit)
            r64 = r.astype(np.float64)
            for k, tau in enumerate(range(-tmax, tmax + 1)):
                rec[j, k] = r64[o + i + tau] if 0 <= o + i + tau < n else 0.0
            rec[j, -2] = 1.0
            rec[0, -1], rec[1, -1] = np.sum(r64[o : o + limit] ** 2), r64[o + limit] ** 2
            want.append(rec)
    got = run(eng, tmax, 1, onsets, segs)
    for k, rec in enumerate(want):
        assert np.array_equal(_bits(got[k]), _bits(rec)), (tmax, k, np.argwhere(_bits(got[k]) != _bits(rec))[:4].tolist())


# ------------------------------------------------------------------------------------------------ rounding-sensitive data
@pytest.mark.parametrize("tmax", [1, 13, 44, 48, 96, 128])
def test_gaussian_noise_within_the_derived_rounding_bound(tmax):
    """Stationary noise (no decaying tail for an error to hide under) through cases(T), entry by entry inside
    xcorr_ref.bounds: (rows + 4) 2^-53 sum |l r| per partition and lag."""
    eng = _eng()
    worst = 0.0
    for launch in X.cases(tmax, "noise"):
        got = run_launch(eng, launch)
        for i, seg in enumerate(launch.segments):
            ref, bnd = X.bounds(seg.l, seg.r, X.segment_onset(launch, seg), seg.limits, tmax)
            err = np.abs(got[i].astype(X.LD) - ref)
            assert np.all(err[bnd == 0] == 0)
            ratio = float(np.max(err[bnd > 0] / bnd[bnd > 0]))
            worst = max(worst, ratio)
            assert np.all(err <= bnd), (tmax, launch.nlim, i, ratio)
    print(f"T = {tmax} {X.shape(tmax).key}: worst |error| / bound {worst:.3e}")


# ------------------------------------------------------------------------------------------------ onsets and limits at their edges
def test_onsets_and_limits_outside_the_segment():
    """Onsets -1, N, N + 5 (and a chunk or more past N) give zeros in every partition, N - 1 the last sample alone; limits
    that are negative or below the limit before them are clamped as include/ira.h states."""
    eng = _eng()
    rng = np.random.default_rng(5)
    tmax, n = 48, CH + 50
    onset_pairs = [(-1, -1), (-1, 5), (n, n), (n + 5, n + 5), (n + CH, n + CH), (n + 2 * CH + 1, 7 * n), (n - 1, n - 1),
                   (n + 5, n - 1), (3, 3)]
    specs = [(p, [1, 5]) for p in range(8)] + [(8, lim) for lim in ([-3, 100], [200, 50], [-7, -2], [2 * n, 100], [n - 3, n - 3])]
    segs = [Seg(_ints(rng, n), _ints(rng, n), 2 * p, 2 * p + 1, lim) for p, lim in specs]
    onsets = [v for pair in onset_pairs for v in pair]
    got = run(eng, tmax, 2, onsets, segs)
    for i, (p, lim) in enumerate(specs):
        o = min(onset_pairs[p])
        want = X.exact_sums(segs[i].l, segs[i].r, o, lim, tmax)
        assert np.array_equal(_bits(got[i]), _bits(want)), (i, o, lim)
    assert not _bits(got[:6]).any()                          # +0.0 everywhere
    l, r = segs[6].l.astype(np.float64), segs[6].r.astype(np.float64)
    last = np.concatenate([l[-1] * r[n - 1 - tmax :], np.zeros(tmax), [l[-1] ** 2, r[-1] ** 2]])
    assert np.array_equal(got[6, 0], last) and np.array_equal(got[7, 0][-2:], [segs[7].l[-1] ** 2.0, segs[7].r[-1] ** 2.0])
    assert not got[6, 1:].any() and not got[7, 1:].any()
    whole = [X.exact_sums(s.l, s.r, 3, [n, n], tmax)[0] for s in segs[8:]]
    assert not got[8, 0].any() and np.array_equal(got[8, 1] + got[8, 2], whole[0])          # [-3, 100]: [0, 0), [0, 100), [100, L)
    assert not got[9, 1].any() and np.array_equal(got[9, 2], whole[1] - X.exact_sums(segs[9].l, segs[9].r, 3, [50, n], tmax)[0])
    assert not got[10, :2].any() and np.array_equal(got[10, 2], whole[2])                   # [-7, -2]: all of it in the last
    assert np.array_equal(got[11, 0], whole[3]) and not got[11, 1].any()                    # [2N, 100]: [0, L), empty, [100, L)


# ------------------------------------------------------------------------------------------------ non-finite samples
@pytest.mark.parametrize("tmax", [48, 128])
def test_a_non_finite_sample_reaches_exactly_the_sums_it_enters(tmax):
    """A NaN in l: C(.) and El of the partition that holds its row.  A NaN (or an infinity) in r at sample p: C(tau) of the
    partitions with a row n, o + n + tau = p, at those lags, and Er of the partition that holds p.  Everything else keeps
    the bits of the clean run."""
    eng = _eng()
    rng = np.random.default_rng(tmax)
    o, n = 5, 2 * CH + tmax + 1
    length = n - o
    limits = [1000, CH + 10, CH + 2000]
    edges = X.partition_edges(limits, length)
    l0, r0 = _ints(rng, n), _ints(rng, n)
    taus = np.arange(-tmax, tmax + 1)
    segs, masks = [Seg(l0, r0, 0, 1, limits)], [np.zeros((4, 2 * tmax + 3), bool)]
    for row in (0, 999, 1000, CH + 5, length - 1):
        l = l0.copy()
        l[o + row] = np.nan
        m = np.zeros((4, 2 * tmax + 3), bool)
        for j, (a, b) in enumerate(edges):
            if a <= row < b:
                m[j, : 2 * tmax + 2] = True
        segs.append(Seg(l, r0, 0, 1, limits))
        masks.append(m)
    for p, bad in ((2, np.nan), (o + 1003, np.nan), (o + CH + 10, np.inf), (o + 2 * CH - 1, np.nan), (n - 1, -np.inf)):
        r = r0.copy()
        r[p] = bad
        m = np.zeros((4, 2 * tmax + 3), bool)
        for j, (a, b) in enumerate(edges):
            m[j, : 2 * tmax + 1] = (a <= p - o - taus) & (p - o - taus < b)
            m[j, 2 * tmax + 2] = a <= p - o < b
        segs.append(Seg(l0, r, 0, 1, limits))
        masks.append(m)
    got = run(eng, tmax, 3, [o, o], segs, finite=False)
    assert np.array_equal(_bits(got[0]), _bits(X.exact_sums(l0, r0, o, limits, tmax)))
    for k in range(1, len(segs)):
        assert masks[k].any() and np.array_equal(~np.isfinite(got[k]), masks[k]), (tmax, k)
        assert np.array_equal(_bits(got[k])[~masks[k]], _bits(got[0])[~masks[k]]), (tmax, k)


# ------------------------------------------------------------------------------------------------ batch invariance at the new shapes
@pytest.mark.parametrize("tmax", [13, 44, 96, 121])
def test_bit_identical_alone_in_the_middle_and_last(tmax):
    eng = _eng()
    for kind in ("int", "noise"):
        launch = X.cases(tmax, kind)[3]                      # nlim = 4; segment 1 is the one of two chunks + T + 1 samples
        segs = launch.segments
        assert len(segs) >= 3 and segs[1].l.size == 2 * CH + tmax + 1
        many = run_launch(eng, launch)
        alone = run(eng, tmax, 4, launch.onsets, [segs[1]])
        last = run(eng, tmax, 4, launch.onsets, segs[:1] + segs[2:] + [segs[1]])
        assert np.array_equal(_bits(many[1]), _bits(alone[0])) and np.array_equal(_bits(last[-1]), _bits(alone[0]))
        assert np.array_equal(_bits(last[: len(segs) - 1]), _bits(np.delete(many, 1, axis=0)))


# ------------------------------------------------------------------------------------------------ max_len below a segment's length
@pytest.mark.parametrize("long_first", [True, False])
def test_fold_reads_only_the_records_max_len_paid_for(long_first):
    """The arrangement of the test of this name in test_gpu_sti.py.  A segment of three chunks in a launch whose max_len
    states two comes out cut at two chunks of rows (the right channel still read from the whole file), its neighbour is
    untouched and nothing past the scratch is written.  Before the fold clamped its chunk range to the records the
    stride holds, the long segment's last partition added the neighbour's first record when it came first and the NaN
    past the scratch when it came last (the tensor the scratch is carved from)."""
    eng = _eng()
    rng = np.random.default_rng(61)
    tmax, limits = 48, [100, CH + 5]
    long_seg = Seg(_ints(rng, 3 * CH), _ints(rng, 3 * CH), 0, 1, limits)
    short = Seg(_ints(rng, CH), _ints(rng, CH), 2, 3, [100, 200])
    onsets = [0, 0, 0, 0]
    segs = [long_seg, short] if long_first else [short, long_seg]
    both = run(eng, tmax, 2, onsets, segs, max_len=2 * CH)
    solo = run(eng, tmax, 2, onsets, [short], max_len=CH)
    k = 0 if long_first else 1
    cut = X.exact_sums(long_seg.l, long_seg.r, 0, limits + [2 * CH], tmax)[:3]
    assert np.array_equal(_bits(both[k]), _bits(cut)), np.argwhere(_bits(both[k]) != _bits(cut))[:4].tolist()
    assert np.array_equal(_bits(both[1 - k]), _bits(solo[0]))
    assert np.array_equal(_bits(solo[0]), _bits(X.exact_sums(short.l, short.r, 0, short.limits, tmax)))
