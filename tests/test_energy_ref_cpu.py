"""Holds the energy-window restatement (tests/energy_ref.py) to a per-sample loop, to closed forms and to hand-written
onsets, and the chunk sizes tests/test_gpu_energy_edges.py is built around to the kernel source, on a machine without a GPU."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

import energy_ref as ER

REPO = Path(__file__).resolve().parent.parent
LD = np.longdouble


def loop_sums(y, onset, limits):
    """P_0 .. P_K, S1 one sample at a time: sample n (from the onset) goes to partition #{k : N_k <= n}.  Python floats; the
    callers use samples whose squares and sums are exact."""
    acc = [0.0] * (len(limits) + 1)
    s1 = 0.0
    for n, v in enumerate(np.asarray(y, dtype=np.float32)[onset:].tolist()):
        e = v * v
        acc[sum(1 for lim in limits if lim <= n)] += e
        s1 += n * e
    return acc + [s1]


@pytest.mark.parametrize("length", [1, 2, 7, 64, 300])
def test_sums_vs_a_per_sample_loop_for_every_limit_placement(length):
    """Samples are small integers / 8: every square, product and sum is exact in float64, so the comparison is ==.  One limit
    at every place 0 .. L + 1; two and three limits on a grid that includes equal ones and ones past the end."""
    rng = np.random.default_rng(length)
    y = (rng.integers(-24, 25, length) / 8.0).astype(np.float32)
    places = range(length + 2)
    for lim in places:
        assert ER.sums(y, 0, (lim,)).astype(np.float64).tolist() == loop_sums(y, 0, (lim,)), lim
    grid = sorted({0, 1, 2, length // 2, length - 1, length, length + 1}) if length > 64 else list(places)
    for a in grid:
        for b in grid:
            if b < a:
                continue
            assert ER.sums(y, 0, (a, b)).astype(np.float64).tolist() == loop_sums(y, 0, (a, b)), (a, b)
            for c in (b, b + 1, length + 1):
                assert ER.sums(y, 0, (a, b, c)).astype(np.float64).tolist() == loop_sums(y, 0, (a, b, c)), (a, b, c)
    for onset in {0, 1, length // 2, length - 1}:
        lims = (1, 3, 3, length + 3)
        assert ER.sums(y, onset, lims).astype(np.float64).tolist() == loop_sums(y, onset, lims), onset


def test_sums_shapes_types_and_empty_partitions():
    y = np.full(10, 0.5, np.float32)
    s = ER.sums(y, 2, (3, 3, 20, 25))
    assert s.dtype == LD and s.shape == (6,)
    assert s.astype(np.float64).tolist() == [0.75, 0.0, 1.25, 0.0, 0.0, 0.25 * 28]
    assert ER.edges(8, (3, 3, 20, 25)) == [0, 3, 3, 8, 8, 8]
    assert ER.sums(y, 10, (1,)).astype(np.float64).tolist() == [0.0, 0.0, 0.0]        # nothing behind the onset
    with pytest.raises(AssertionError):
        ER.sums(y, 0, (5, 4))


def test_sums_and_params_vs_the_geometric_series():
    """x[n] = float32(r^n): the partition sums and S1 from geometric series in q = r^2.  The float32 rounding of a sample
    moves its energy by at most 2^-23 relative (2 * 2^-24 and the second-order term), so every sum of these non-negative
    terms is within 2^-23 of its closed form; the long-double sums add ~2^-60 to that."""
    for r, m, limits in ((0.9995, 48000, (2400, 3840)), (0.99985, 96000, (2400, 3840)), (0.999, 40000, (1, 16384, 32768))):
        x = (r ** np.arange(m, dtype=np.float64)).astype(np.float32)
        q = LD(r) * LD(r)

        def geo(a, b):                                 # sum_{n=a}^{b-1} q^n
            return q ** a * (1 - q ** (b - a)) / (1 - q)

        got = ER.sums(x, 0, limits)
        e = [0, *limits, m]
        want = [geo(a, b) for a, b in zip(e[:-1], e[1:])]
        want.append(q * (1 - m * q ** (m - 1) + (m - 1) * q ** m) / (1 - q) ** 2)
        tol = 2.0 ** -23 * 1.001
        for g, w in zip(got, want):
            assert abs(g - w) <= tol * w, (r, float(g), float(w))
        c, d, ts = ER.params(got, 48000)
        for k, ck in enumerate(c):
            n_k = limits[k]
            w = 10.0 * math.log10(float(geo(0, n_k) / geo(n_k, m)))
            assert abs(ck - w) <= 20.0 / math.log(10.0) * tol + 1e-12, (r, k, ck, w)   # d(10 log10 (a / b)): both off by tol
        total = geo(0, m)
        assert abs(d - float(geo(0, limits[0]) / total)) <= 2.0 * tol
        assert abs(ts - float(want[-1] / (48000 * total))) <= 2.0 * tol * ts


def test_params_hand_values():
    c, d, ts = ER.params(np.array([3.0, 1.0, 4.0, 16.0], LD), 8.0)        # P_0 P_1 P_2, S1
    assert c == pytest.approx([10.0 * math.log10(3.0 / 5.0), 0.0], abs=1e-15) and d == 0.375 and ts == 0.25
    assert ER.params(np.array([3.0, 1.0, 4.0, 16.0], LD), 8.0, d_index=1)[1] == 0.5
    c, d, ts = ER.params(np.array([2.0, 0.0, 0.0], LD), 1.0)
    assert c == [math.inf] and d == 1.0 and ts == 0.0
    assert ER.params([1.0, 1.0, 0.0, 0.0], 1.0)[0] == [0.0, math.inf]
    assert all(isinstance(v, float) for v in (d, ts, *c))


def test_onset_hand_cases():
    f = np.float32
    assert 100.0 * 0.01 == 1.0                                           # peak 10 at -20 dB: the threshold is exactly 1.0
    below = np.nextafter(f(1.0), f(0.0))
    # a tie at the threshold (>=) and the float32 just below it
    assert ER.onset(np.array([0.0, 0.1, below, 1.0, 3.0, 10.0, 2.0], f), 0.01) == 3
    assert ER.onset(np.array([0.0, below, below, 10.0], f), 0.01) == 3
    # the first maximum among equal maxima is the peak: the later ones, and what qualifies behind it, do not count
    assert ER.onset(np.array([0.0, 0.2, -4.0, 4.0, 4.0, 0.1], f), 1.0) == 2
    assert ER.onset(np.array([0.1, 10.0, 1.0, 10.0], f), 0.01) == 1
    # rel_energy 0: every sample qualifies, 1: the peak itself (the first sample of its magnitude)
    x = np.array([0.0, 0.3, -0.2, 7.0, 0.5], f)
    assert ER.onset(x, 0.0) == 0 and ER.onset(x, 1.0) == 3
    assert ER.onset(np.array([0.0, 0.0], f), 0.5) == 0                   # silence: 0 >= 0
    # a negative peak, and negative samples in front of it: the squares decide
    assert ER.onset(np.array([0.1, -0.9, -1.0, 0.5, -10.0, 9.0], f), 0.01) == 2
    assert ER.onset(np.array([0.1, -0.9, 0.5, -10.0, 10.0], f), 0.01) == 3
    # the compare is on float64 squares of the float32 samples: float32(0.1)^2 = 0.010000000298 >= 100 * 1e-4
    assert ER.onset(np.array([0.0, 0.1, 10.0], f), 1e-4) == 1
    assert isinstance(ER.onset(x, 0.5), int)


def _constants(text):
    """The integer constexpr constants of a kernel source whose definitions are products of numbers and earlier constants."""
    vals = {}
    for name, expr in re.findall(r"constexpr\s+int\s+(\w+)\s*=\s*([^;]+);", text):
        prod = 1
        for tok in (t.strip() for t in expr.split("*")):
            if tok.isdigit():
                prod *= int(tok)
            elif tok in vals:
                prod *= vals[tok]
            else:
                prod = None
                break
        if prod is not None:
            vals[name] = prod
    return vals


def test_chunk_sizes_of_the_edge_tests_are_the_kernels():
    import test_gpu_energy_edges as G
    consts = _constants((REPO / "audio_analysis_amd" / "csrc" / "ira_energy.hip").read_text())
    assert consts["EW_CHUNK"] == G.EW_CHUNK == G.C == 16384
    assert consts["ON_CHUNK"] == G.ON_CHUNK == 4096
    assert consts["EW_MAX_LIMITS"] == 4 == max(len(s) for s in G.limit_sets(100))
    # the lengths and limit sets bracket the chunk boundaries, and the longest row has more chunks than the fold has lanes
    assert {G.C - 1, G.C, G.C + 1, 2 * G.C, 2 * G.C + 5}.issubset(G.LENGTHS) and max(G.LENGTHS) > 64 * G.C
    assert G.counts(7, (2, 2, 9)) == [2, 0, 5, 0] and G.counts(1, (1,)) == [1, 0]
    flat, off, lens = G.pack([np.zeros(n, np.float32) for n in (3, 0, 5, 8, 2, 1, 6, 9)])
    gaps = off - np.concatenate([[0], (off + lens)[:-1]])
    assert gaps.min() >= 1 and gaps.max() <= 7 and set((off % 4).tolist()) == {0, 1, 2, 3}
    assert flat.size == off[-1] + lens[-1] + 8 and np.count_nonzero(flat == np.float32(G.FILL)) == flat.size - lens.sum()
