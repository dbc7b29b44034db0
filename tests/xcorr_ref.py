"""
References for the ISO 3382-1 lag sums of audio_analysis_amd/csrc/ira_xcorr.hip (ira_xcorr_windows), written from the
definitions in include/ira.h and sharing no code with the kernels.  Helper module, like sti_ref.py: it holds no tests.

  ref_onset, ref_sums, narrow, ref_coefficient   the long-double restatement test_gpu_iacc.py has always used
  exact_sums      integer-valued samples in int64: what the device must return bit for bit
  bounds          the restatement with a derived rounding bound per partition and lag
  shape           the decomposition xcorr_partial_kernel chooses for one max lag T, restated
  pieces          the (chunk, partition) pieces of a segment, i.e. the records pass 1 writes
  cases           a small ragged set of launches for one T that meets the row counts at which the kernel changes path
"""
import math
import re
from collections import namedtuple
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
LD = np.longdouble
U = 2.0 ** -53                       # unit roundoff of float64
TREF = 128                           # IRA_XCORR_MAX_LAG: exact prefix sums are formed at this T and narrowed
MAX_INT = 127                        # |sample| of the integer cases
MAX_ROWS_EXACT = 1 << 20
MAX_ROWS_BOUND = 8192

_SRC = (REPO / "audio_analysis_amd" / "csrc" / "ira_xcorr.hip").read_text()


def _constant(name):
    return int(re.search(rf"constexpr int {name} = (\d+);", _SRC).group(1))


CH = _constant("XC_CHUNK")           # rows (counted from the onset) per workgroup
THREADS = _constant("XC_THREADS")
LPT_CANDIDATES = (13, 11, 9)


# ------------------------------------------------------------------------------------------------ the restatement
def ref_onset(x, onset_db=-20.0):
    x = np.asarray(x, dtype=np.float32)
    e = x.astype(np.float64) ** 2
    p = int(np.argmax(np.abs(x)))
    return int(np.flatnonzero(e[: p + 1] >= e[p] * 10.0 ** (onset_db / 10.0))[0])


def ref_sums(l, r, o, limits, tmax):
    """(K + 1, 2T + 3) long double: per partition [a, b) of n = 0 .. L - 1 (counted from o; limits past L give empty
    partitions) C(tau) = sum l[o + n] r[o + n + tau] on a zero-padded right channel, tau = -T .. T, then El, Er."""
    l = np.asarray(l, dtype=np.float32).astype(LD)
    r = np.asarray(r, dtype=np.float32).astype(LD)
    n = l.size
    assert r.size == n
    length = n - o
    rp = np.zeros(n + 2 * tmax, dtype=LD)                # rp[m + T] = r[m], zeros for m < 0 and m >= N
    rp[tmax : tmax + n] = r
    edges = [0] + [min(int(v), length) for v in limits] + [length]
    out = np.zeros((len(edges) - 1, 2 * tmax + 3), dtype=LD)
    for j, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        if b <= a:
            continue
        ls = l[o + a : o + b]
        for k, tau in enumerate(range(-tmax, tmax + 1)):
            out[j, k] = np.sum(ls * rp[tmax + o + a + tau : tmax + o + b + tau])
        out[j, 2 * tmax + 1] = np.sum(ls * ls)
        out[j, 2 * tmax + 2] = np.sum(r[o + a : o + b] ** 2)
    return out


def narrow(ref, t_from, t_to):
    """The record of max lag t_to cut out of one of max lag t_from >= t_to (C(tau) does not depend on T)."""
    d = t_from - t_to
    return np.concatenate([ref[:, d : d + 2 * t_to + 1], ref[:, 2 * t_from + 1 :]], axis=1)


def ref_coefficient(rec):
    """(IACC, tau in samples, |IACF| of every lag) of one summed record, float64."""
    rec = np.asarray(rec, dtype=np.float64)
    tmax = (rec.size - 3) // 2
    iacf = np.abs(rec[: 2 * tmax + 1] / math.sqrt(rec[-2] * rec[-1]))
    k = int(np.argmax(iacf))
    return float(iacf[k]), k - tmax, iacf


# ------------------------------------------------------------------------------------------------ partitions
def segment_rows(n, o):
    """L of include/ira.h: the rows of a segment of n samples counted from its onset o; none for an onset outside 0 .. n."""
    return n - o if 0 <= o <= n else 0


def partition_edges(limits, length):
    """[(a, b)] of the nlim + 1 partitions as include/ira.h states them: every limit clamped to 0 .. L, an upper limit
    below its partition's lower one gives an empty partition.  For ascending limits these are [0, N_1), ..., [N_K, L)."""
    length = max(int(length), 0)
    clamp = lambda v: min(max(int(v), 0), length)                         # noqa: E731
    edges = []
    for j in range(len(limits) + 1):
        a = 0 if j == 0 else clamp(limits[j - 1])
        b = length if j == len(limits) else max(a, clamp(limits[j]))
        edges.append((a, b))
    return edges


def pieces(length, limits):
    """[(chunk, partition, first row within the chunk, rows)]: the non-empty intersections of the partitions with the
    chunks of CH rows, one record of pass 1 each."""
    out = []
    for j, (a, b) in enumerate(partition_edges(limits, length)):
        for c in range(a // CH, (b - 1) // CH + 1 if b > a else 0):
            lo, hi = max(a, c * CH), min(b, (c + 1) * CH)
            out.append((c, j, lo - c * CH, hi - lo))
    return out


# ------------------------------------------------------------------------------------------------ exact integer sums
def _as_int(x):
    x = np.asarray(x, dtype=np.float32)
    xi = x.astype(np.int64)
    assert np.array_equal(xi.astype(np.float32), x) and (xi.size == 0 or int(np.max(np.abs(xi))) <= MAX_INT)
    return xi


def exact_prefix(l, r, o):
    """(L + 1, 2 TREF + 3) int64: row m holds the sums over the rows n < m of l[o + n] r[o + n + tau], tau = -TREF .. TREF,
    then of l[o + n]^2 and r[o + n]^2."""
    li, ri = _as_int(l), _as_int(r)
    n = li.size
    assert ri.size == n
    length = segment_rows(n, o)
    assert length <= MAX_ROWS_EXACT
    pre = np.zeros((length + 1, 2 * TREF + 3), dtype=np.int64)
    if length:
        rp = np.zeros(n + 2 * TREF, dtype=np.int64)                       # rp[m + TREF] = r[m], zeros outside the file
        rp[TREF : TREF + n] = ri
        win = np.lib.stride_tricks.sliding_window_view(rp, 2 * TREF + 1)[o : o + length]   # win[n, k] = r[o + n + k - TREF]
        ls, rs = li[o : o + length], ri[o : o + length]
        prod = np.empty((length, 2 * TREF + 3), dtype=np.int64)
        prod[:, : 2 * TREF + 1] = ls[:, None] * win
        prod[:, 2 * TREF + 1] = ls * ls
        prod[:, 2 * TREF + 2] = rs * rs
        np.cumsum(prod, axis=0, out=pre[1:])
    return pre


def exact_sums(l, r, o, limits, tmax, prefix=None):
    """(K + 1, 2T + 3) float64 of integer-valued float32 samples, |sample| <= 127, at most 2^20 rows: every product and every
    partial sum of any subset of the rows is an integer below 127^2 2^20 < 2^34 < 2^53, so float64 addition is exact in any
    order and the device must return exactly these values.  Prefix sums over the rows at T = 128 (exact_prefix, which a
    caller may pass in), partitions as differences (partition_edges), smaller T cut out with narrow."""
    pre = exact_prefix(l, r, o) if prefix is None else prefix
    edges = partition_edges(limits, pre.shape[0] - 1)
    full = np.stack([pre[b] - pre[a] for a, b in edges])
    assert int(np.max(np.abs(full))) < 1 << 53
    return narrow(full, TREF, tmax).astype(np.float64)


# ------------------------------------------------------------------------------------------------ rounding bound
def bounds(l, r, o, limits, tmax):
    """(ref, bound), both (K + 1, 2T + 3) long double, for rounding-sensitive samples and ascending limits: ref is ref_sums
    and |dev - ref| <= bound must hold entry by entry.  Per partition j of n_j rows, with u = 2^-53:
        |C_dev(tau) - C_ref(tau)| <= (n_j + 4) u A_j(tau),  A_j(tau) = sum |l[o + n] r[o + n + tau]|,
        El and Er to (n_j + 4) u El and (n_j + 4) u Er.
    The product of two float32 values is exact in float64 and every addition rounds once, so any order of summation stays
    within gamma_(n-1) A; the + 4 covers gamma against (n - 1) u and the restatement's own error (n 2^-64 relative, at most
    4 u for n <= 8192).  CONDITION: every partition has at most 8192 rows (asserted)."""
    n = np.asarray(l).size
    length = segment_rows(n, o)
    assert 0 <= o and all(0 <= a <= b for a, b in zip([0] + list(limits), limits)), "ascending limits from a valid onset"
    ref = ref_sums(l, r, o, limits, tmax)
    mag = ref_sums(np.abs(np.asarray(l, dtype=np.float32)), np.abs(np.asarray(r, dtype=np.float32)), o, limits, tmax)
    rows = np.array([b - a for a, b in partition_edges(limits, length)])
    assert rows.max() <= MAX_ROWS_BOUND, rows
    return ref, (rows[:, None] + 4).astype(LD) * LD(U) * mag


# ------------------------------------------------------------------------------------------------ the kernel's shape
def lags_per_thread(nlag):
    """xc_lags_per_thread: the odd candidate that wastes the fewest lag slots (ties: the wider one)."""
    best, best_waste = 9, 1 << 30
    for c in LPT_CANDIDATES:
        waste = -(-nlag // c) * c - nlag
        if waste < best_waste:
            best, best_waste = c, waste
    return best


class Shape:
    """What xcorr_partial_kernel derives from T: lags per thread, lag groups, sub-ranges of the rows, lag slots W, idle
    threads; and from the rows of a (chunk, partition) piece the sub-range length and each sub-range's loop counts."""

    def __init__(self, tmax):
        self.tmax = int(tmax)
        self.nlag = 2 * self.tmax + 1
        self.lpt = lags_per_thread(self.nlag)
        self.ngroups = -(-self.nlag // self.lpt)
        self.nsub = THREADS // self.ngroups
        self.w = self.lpt * self.ngroups
        self.idle = THREADS - self.ngroups * self.nsub
        self.key = (self.lpt, self.ngroups, self.nsub)

    def sub_len(self, rows):
        return (-(-rows // self.nsub)) | 1

    def sub_ranges(self, rows):
        """[(rows, unrolled LPT-row bodies, remainder rows)] of the nsub sub-ranges of a piece of `rows` rows."""
        sl = self.sub_len(rows)
        out = []
        for s in range(self.nsub):
            n = max(0, min(s * sl + sl, rows) - s * sl)
            out.append((n, n // self.lpt, n % self.lpt))
        return out


def shape(tmax):
    return Shape(tmax)


# ------------------------------------------------------------------------------------------------ cases
Segment = namedtuple("Segment", "l r lchan rchan limits")                # l, r: float32 arrays of the segment's length
Launch = namedtuple("Launch", "tmax nlim onsets segments")               # onsets: one per channel entry

# (onset of l, onset of r) per channel pair; the pair's onset is the lower one
ONSET_PAIRS = ((0, 0), (1, 1), (CH - 1, CH - 1), (CH, CH), (0, 5), (CH + 3, CH - 1))


def required_rows(tmax):
    """The row counts a (chunk, partition) piece must take in cases(T): 1, nsub - 1, nsub, nsub + 1, one whose sub-range
    length is below LPT (remainder loop only), LPT nsub (every sub-range exactly one unrolled body) and (LPT + 2) nsub
    (a body and two remainder rows) where those fit a chunk, CH - 1 and CH."""
    s = shape(tmax)
    want = [1, s.nsub - 1, s.nsub, s.nsub + 1, 2 * s.nsub + 1]
    want += [k for k in (s.lpt * s.nsub, (s.lpt + 2) * s.nsub) if k <= CH]
    return want + [CH - 1, CH]


def case_specs(tmax):
    """[(nlim, onset pair, L, limits)] of cases(T).  Two fixed segments with four limits: the counts around nsub packed
    one after the other inside a chunk (pieces that start in the middle of a chunk), and a segment of two chunks + T + 1
    rows with a limit on the chunk boundary, one sample either side of it and one past L.  Then one segment per required
    count k with [0, k) as its first partition, nlim cycling through 1 .. 4, the other limits equal to k (an empty partition),
    k + 1, L itself or past L, and the onset pairs taken in turn."""
    s = shape(tmax)
    n = s.nsub
    specs = [(4, 0, 3 * n + 1 + 2 * n + 1, [1, n, 2 * n, 3 * n + 1]),
             (4, 0, 2 * CH + tmax + 1, [CH - 1, CH, CH + 1, 3 * CH])]
    for i, k in enumerate(required_rows(tmax)):
        nlim = 1 + i % 4
        length = k + 1 + i % 2
        fill = ([k, k + 1, length + 5], [k + 1, length, length + 5])[(i // 4) % 2]
        specs.append((nlim, (i + 1) % len(ONSET_PAIRS), length, [k] + fill[: nlim - 1]))
    return specs


def cases(tmax, kind="int"):
    """Four launches (nlim = 1, 2, 3, 4) of a few segments each, every segment at most 2 chunks + T + 1 samples; the
    same specs for every kind of samples: "int" integers in -127 .. 127 (exact_sums), "noise" stationary Gaussian (bounds)."""
    rng = np.random.default_rng([int(tmax), {"int": 0, "noise": 1}[kind]])
    onsets = np.array([v for pair in ONSET_PAIRS for v in pair], dtype=np.int64)
    by_nlim = {k: [] for k in (1, 2, 3, 4)}
    for nlim, pair, length, limits in case_specs(tmax):
        n = min(ONSET_PAIRS[pair]) + length
        assert n <= 2 * CH + tmax + 1 and len(limits) == nlim
        if kind == "int":
            l, r = (rng.integers(-MAX_INT, MAX_INT + 1, n).astype(np.float32) for _ in range(2))
        else:
            l, r = (rng.standard_normal(n).astype(np.float32) for _ in range(2))
        by_nlim[nlim].append(Segment(l, r, 2 * pair, 2 * pair + 1, list(limits)))
    return [Launch(int(tmax), nlim, onsets, segs) for nlim, segs in by_nlim.items()]


def segment_onset(launch, seg):
    return int(min(launch.onsets[seg.lchan], launch.onsets[seg.rchan]))
