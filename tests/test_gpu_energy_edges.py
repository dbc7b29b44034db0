"""
ira_onset_index and ira_energy_windows (ira_energy.hip) at the edges of their chunks, through Engine.onset_index and
Engine.energy_windows.

The partial kernel of the window sums works on chunks of EW_CHUNK samples counted from the segment's onset and takes one of
two routines per chunk: a per-sample partition test when a limit falls strictly inside the chunk, one plain sum placed by
the number of limits at or below the chunk's start otherwise.  The tests put limits on a chunk boundary and one sample
either side of it, in later chunks, in the last, partial chunk, at and past the segment's end, twice at the same place, and
use 1, 2, 3 and 4 limits.  Where the samples are 0.5 (or a single power of two) every product and every partial sum is a
small multiple of a power of two, exact in float64 in ANY order of summation: those results are compared with ==, so one
sample on the wrong side of a limit fails them.  Decaying noise is held to the long-double restatement of
tests/energy_ref.py at 1e-12, the tolerance of tests/test_gpu_energy.py.

The onset search works on chunks of ON_CHUNK samples that meet in an atomicMin; its tests put the peak and the first
qualifying sample on those boundaries.

Rows lie in one flat buffer with 0.5 in gaps of 1 to 7 samples, so that row offsets take every residue mod 4 and a read
outside a row changes a sum.  tests/test_energy_ref_cpu.py checks EW_CHUNK and ON_CHUNK against the kernel source.
"""
import numpy as np
import pytest

import energy_ref as ER

pytestmark = pytest.mark.gpu

EW_CHUNK = 16384
ON_CHUNK = 4096
C = EW_CHUNK
TOL = 1e-12                                   # relative, as in tests/test_gpu_energy.py
FILL = 0.5
LENGTHS = (1, 3, 4, 5, C - 1, C, C + 1, 2 * C, 2 * C + 5, 65 * C + 3)     # 65 chunks: the fold's lanes wrap past 64


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def pack(rows):
    """(flat float32, offsets, lengths): the rows in one buffer, FILL in the gaps.  The gap in front of row i has 1 to 7
    samples and puts the row at residue i mod 4; 8 samples of FILL follow the last row."""
    off, pos = [], 0
    for i, r in enumerate(rows):
        g = (i - pos) % 4 or 4
        if i % 2 and g <= 3:
            g += 4
        pos += g
        off.append(pos)
        pos += len(r)
    flat = np.full(pos + 8, FILL, np.float32)
    for o, r in zip(off, rows):
        flat[o : o + len(r)] = r
    return flat, np.array(off, np.int64), np.array([len(r) for r in rows], np.int64)


def limit_sets(length):
    """The limit sets for a row of `length` samples: one limit around the first chunk boundary and around the row's end, four
    across the boundaries, two in the partial chunk behind the second boundary, two equal ones, four up to the 65th chunk, three
    (a boundary, the next one and a sample behind it).  Every set goes to every length: a limit at or past the end leaves empty
    partitions behind it, which is part of what is tested.  Only a limit of 0 (length - 1 of a one-sample row) is left out:
    the host never forms one."""
    sets = [(C - 1,), (C,), (C + 1,), (C - 1, C, C + 1, 2 * C), (2 * C + 1, 2 * C + 3), (length - 1,), (length,),
            (length + 7,), (5, 5), (1, C, 2 * C, 64 * C + 1), (C, 2 * C, 2 * C + 4)]
    return [s for s in dict.fromkeys(sets) if s[0] >= 1]


def counts(length, limits):
    """Samples per partition, one sample at a time: sample n belongs to partition #{k : N_k <= n}."""
    part = np.searchsorted(np.asarray(limits, np.int64), np.arange(length, dtype=np.int64), side="right")
    return [int(v) for v in np.bincount(part, minlength=len(limits) + 1)]


def windows(eng, x_dev, off, lens, segs, onset_dev, chan=None):
    """Engine.energy_windows over the segments segs = [(row, limits)]: ONE launch per number of limits, a ragged batch each.
    onset_dev holds one onset per row; segment j starts at the onset of row chan[j] (its own row when chan is None).
    Returns the records (numpy, nlim + 2 doubles) in the order of segs."""
    out = [None] * len(segs)
    for nlim in sorted({len(s) for _, s in segs}):
        idx = [j for j, (_, s) in enumerate(segs) if len(s) == nlim]
        rows = np.array([segs[j][0] for j in idx], np.int64)
        ch = rows if chan is None else np.array([chan[j] for j in idx], np.int64)
        got = eng.energy_windows(x_dev, off[rows], lens[rows], ch.astype(np.int32), onset_dev,
                                 np.array([segs[j][1] for j in idx], np.int64)).cpu().numpy()
        assert got.shape == (len(idx), nlim + 2)
        for j, g in zip(idx, got):
            out[j] = g
    return out


def zero_onsets(eng, n):
    return eng.to_dev(np.zeros(n, np.int64))


# ------------------------------------------------------------------------------------------------ a. exact membership
def test_constant_rows_count_every_sample_in_its_partition():
    """Rows of 0.5: e = 0.25, so P_j = 0.25 count_j and S1 = 0.25 L (L - 1) / 2, exactly, whatever the order of the sums."""
    eng = _eng()
    rows = [np.full(n, 0.5, np.float32) for n in LENGTHS]
    flat, off, lens = pack(rows)
    assert set((off % 4).tolist()) == {0, 1, 2, 3}
    segs = [(i, s) for i, n in enumerate(LENGTHS) for s in limit_sets(n)]
    assert {len(s) for _, s in segs} == {1, 2, 3, 4}
    got = windows(eng, eng.to_dev(flat), off, lens, segs, zero_onsets(eng, len(rows)))
    for (i, s), g in zip(segs, got):
        n = LENGTHS[i]
        want = [0.25 * c for c in counts(n, s)] + [0.25 * (n * (n - 1) // 2)]
        assert g.tolist() == want, (n, s, g.tolist(), want)


# ------------------------------------------------------------------------------------------------ b. a non-zero onset
def test_constant_rows_from_a_non_zero_onset():
    """Rows of 0.5 with a 10.0 at index d: the -20 dB threshold is 100 * 0.01 == 1.0 > 0.25, so the onset is d and the segment
    starts misaligned to the row's own chunk grid; its 2 C + 5 samples put the limits on the chunk edges counted from the
    onset.  P_0 carries the spike (100, exact), S1 does not (n = 0).  The last row is a "band" row without a spike that
    starts at the onset of row 3 (chan_of_seg)."""
    eng = _eng()
    assert 100.0 * 0.01 == 1.0
    n = 2 * C + 5
    onsets = (1, 4095, 4096, 4097, C + 3)
    rows = []
    for d in onsets:
        r = np.full(d + n, 0.5, np.float32)
        r[d] = 10.0
        rows.append(r)
    band_of = 3
    rows.append(np.full(onsets[band_of] + n, 0.5, np.float32))
    flat, off, lens = pack(rows)
    b = eng.wrap(eng.to_dev(flat), off, lens)
    on, _, _ = eng.onset_index(b, 0.01)
    assert on.cpu().tolist() == list(onsets) + [0]
    sets = [(C - 1, C, C + 1, 2 * C), (2 * C + 1, 2 * C + 3), (C,), (C, 2 * C, 2 * C + 4), (n - 1,), (n,)]
    segs = [(i, s) for i in range(len(rows)) for s in sets]
    chan = [band_of if i == len(rows) - 1 else i for i, _ in segs]
    got = windows(eng, b.x, off, lens, segs, on, chan)
    for (i, s), g in zip(segs, got):
        want = [0.25 * c for c in counts(n, s)] + [0.25 * (n * (n - 1) // 2)]
        if i < len(onsets):
            want[0] += 100.0 - 0.25
        assert g.tolist() == want, (i, s, g.tolist(), want)


# ------------------------------------------------------------------------------------------------ c. single impulses
def test_a_single_impulse_lands_in_exactly_one_partition():
    """Zero rows of 2 C + 5 samples with 2^-3 at one index n, one limit N: the impulse's 2^-6 is in P_0 when n < N, in P_1
    otherwise, and S1 = n 2^-6."""
    eng = _eng()
    length = 2 * C + 5
    cases = sorted({(lim, n) for lim in (C - 1, C, C + 1) for n in (0, lim - 1, lim, C - 1, C, 2 * C + 4)})
    rows = []
    for _, n in cases:
        r = np.zeros(length, np.float32)
        r[n] = 2.0 ** -3
        rows.append(r)
    flat, off, lens = pack(rows)
    segs = [(i, (lim,)) for i, (lim, _) in enumerate(cases)]
    got = windows(eng, eng.to_dev(flat), off, lens, segs, zero_onsets(eng, len(rows)))
    for (lim, n), g in zip(cases, got):
        want = [2.0 ** -6 if n < lim else 0.0, 2.0 ** -6 if n >= lim else 0.0, n * 2.0 ** -6]
        assert g.tolist() == want, (lim, n, g.tolist(), want)


# ------------------------------------------------------------------------------------------------ d, e. decaying noise
@pytest.fixture(scope="module")
def noise():
    """(rows, segs, device records): decaying noise of every length, the limit sets of (a) on all but the longest row, which
    gets the limits 64 C and 64 C + 1 (the chunk the fold's lane 0 takes second)."""
    eng = _eng()
    rng = np.random.default_rng(53)
    rows = [(rng.standard_normal(n) * np.exp(-4.0 * np.arange(n) / n)).astype(np.float32) for n in LENGTHS]
    segs = [(i, s) for i, n in enumerate(LENGTHS[:-1]) for s in limit_sets(n)] + [(len(LENGTHS) - 1, (64 * C, 64 * C + 1))]
    flat, off, lens = pack(rows)
    got = windows(eng, eng.to_dev(flat), off, lens, segs, zero_onsets(eng, len(rows)))
    return rows, segs, got


def test_decaying_noise_vs_the_long_double_restatement(noise):
    rows, segs, got = noise
    worst = 0.0
    for (i, s), g in zip(segs, got):
        want = ER.sums(rows[i], 0, s)
        e = ER.edges(rows[i].size, s)
        for k in range(len(s) + 2):
            if k <= len(s) and e[k + 1] <= e[k]:
                assert g[k] == 0.0, (rows[i].size, s, k, g[k])           # an empty partition: exactly zero
                continue
            err = float(abs(np.longdouble(g[k]) - want[k]))
            assert err <= TOL * float(want[k]), (rows[i].size, s, k, g[k], want[k])
            if want[k] > 0:
                worst = max(worst, err / float(want[k]))
    print(f"{len(segs)} segments: largest relative error {worst:.3e} (bound {TOL:.0e})")
    assert worst < TOL


def test_each_noise_row_alone_gives_the_same_bytes(noise):
    """Alone the row starts at offset 0 of a buffer of its own and the launch is sized for its length only (another chunk
    stride of the scratch): the records are the same bytes."""
    eng = _eng()
    rows, segs, got = noise
    for i, r in enumerate(rows):
        mine = [j for j, (ri, _) in enumerate(segs) if ri == i]
        b = eng.upload([r])
        alone = windows(eng, b.x, b.off, b.length, [(0, segs[j][1]) for j in mine], zero_onsets(eng, 1))
        for j, a in zip(mine, alone):
            assert a.tobytes() == got[j].tobytes(), (r.size, segs[j][1], a.tolist(), got[j].tolist())


# ------------------------------------------------------------------------------------------------ f. onset search
def onset_row(p, hits=(), peak=10.0, under=None, hit=1.0):
    """Background 0.1 (e = 0.01), the peak at p, `hit` (|hit| = 1.0: e == the threshold 100 * 0.01 exactly) at every index
    of hits, the float32 just under 1.0 at `under`.  Behind the peak: a 9.0 (qualifies at -20 dB, but lies past p), a sample
    of the peak's magnitude and the other sign (the FIRST maximum is the peak), one of background."""
    r = np.full(p + 4, 0.1, np.float32)
    for h in hits:
        r[h] = hit
    if under is not None:
        r[under] = np.nextafter(np.float32(1.0), np.float32(0.0))
    r[p] = peak
    r[p + 1 : p + 4] = (9.0, -peak, 0.1)
    return r


def test_onset_search_at_chunk_edges():
    """Expected onsets are energy_ref.onset's; at -20 dB each is also known by construction (the smallest hit, else the peak),
    at rel_energy 0 it is 0 and at 1 the peak."""
    eng = _eng()
    oc = ON_CHUNK
    cases = [  # (peak index, indices at the threshold, index just under it)
        (0, (), None),
        (oc - 1, (3,), None), (oc - 1, (oc - 2,), None), (oc - 1, (), None),
        (oc, (3,), None), (oc, (oc - 1,), None), (oc, (), None),
        (oc + 1, (oc,), None), (oc + 1, (oc - 1,), None), (oc + 1, (3, oc), None), (oc + 1, (), None),
        (oc + 1, (oc,), oc - 1),
        (2 * oc, (5000,), None), (2 * oc, (oc - 1,), None), (2 * oc, (oc,), None), (2 * oc, (2 * oc - 1,), None),
        (2 * oc, (), None), (2 * oc, (100, oc, 2 * oc - 1), None), (2 * oc, (oc, 2 * oc - 1), None),
        (2 * oc, (oc - 1, oc, oc + 1), None), (2 * oc, (oc,), oc - 1), (2 * oc, (oc - 1,), oc - 2),
        (2 * oc, (2 * oc - 1,), 3),
    ]
    rows, hand = [], []
    for j, (p, hits, under) in enumerate(cases):
        sign = -1.0 if j % 2 else 1.0                                    # every other row: a negative peak, negative hits
        rows.append(onset_row(p, hits, sign * 10.0, under, sign * 1.0))
        hand.append((p, min(hits) if hits else p))
    zero_at = len(rows) // 2
    rows.insert(zero_at, np.zeros(0, np.float32))                        # a zero-length row in the middle of the batch
    hand.insert(zero_at, None)
    flat, off, lens = pack(rows)
    b = eng.wrap(eng.to_dev(flat), off, lens)
    assert 100.0 * 0.01 == 1.0
    for rel in (0.0, 0.01, 1.0):
        on, pk, _ = eng.onset_index(b, rel)
        on, pk = on.cpu().tolist(), pk.cpu().tolist()
        for j, r in enumerate(rows):
            if hand[j] is None:
                assert on[j] == pk[j], (rel, on[j], pk[j])               # what ira_peak_index left
                continue
            p, first = hand[j]
            want = ER.onset(r, rel)
            assert want == {0.0: 0, 0.01: first, 1.0: p}[rel], (rel, j, want, hand[j])
            assert pk[j] == p and on[j] == want, (rel, j, pk[j], on[j], want)
