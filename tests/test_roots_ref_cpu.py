"""tests/roots_ref.py (the yardsticks, generators and case lists of test_gpu_roots.py) pinned without a GPU: the backward error
accepts what a backward-stable method returns and rejects a root moved by 1e-9; its scaled evaluation agrees with the plain
one and survives where the plain one overflows; the completeness check rejects any single duplicated root on every case;
and a NumPy restatement of the kernel's iteration with the overflow-safe evaluation meets both bounds on every case, so the
bounds ask nothing the method cannot give.  The same restatement with plain Horner returns NaN for the whole polynomial
as soon as one root lies far enough outside the unit circle.
"""
import functools

import numpy as np
import pytest

import roots_ref as R
from oracle import ira_oracle as O


@pytest.fixture(autouse=True)
def _longdouble():
    R.need_longdouble()


CASES = dict(R.all_cases())


@functools.lru_cache(maxsize=None)
def _solved(name):
    """(roots of the safe restatement, completeness tolerance), computed once per case."""
    c = CASES[name]
    return R.aberth(c), R.completeness_tolerance(c)


def test_numpy_roots_is_backward_stable_at_low_degree():
    polys = [R.degree_case(n)[0] for n in R.DEGREES if n <= 64] + [R.outside_case(64, (-6e4,))[0]]
    for c in polys:
        be = R.backward_error(c, np.roots(c))
        assert np.all(np.isfinite(be)) and np.max(be) < 1e3 * R.U, (c.size - 1, np.max(be) / R.U)


@pytest.mark.parametrize("name", ["ring64", "ring129", "outside128"])
def test_a_root_moved_by_1e_9_is_rejected(name):
    c = CASES[name]
    n = c.size - 1
    z = _solved(name)[0]
    assert np.max(R.backward_error(c, z)) <= R.bound(n)
    for step in (1e-9, -1e-9j):
        assert np.min(R.backward_error(c, z + step)) > R.bound(n)


def test_scaled_evaluation_agrees_with_the_plain_one():
    rng = np.random.default_rng(3)
    for name in ("ring65", "outside64", "outside128", "outside257", "outside1000"):
        c = CASES[name]
        n = c.size - 1
        pts = np.concatenate([_solved(name)[0][:: max(1, n // 40)],
                              rng.uniform(0.5, 3.0, 40) * np.exp(2j * np.pi * rng.random(40))])
        a, b = R.backward_error(c, pts), R.backward_error_unscaled(c, pts)
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
        # both are Horner sums in long double: each within 2 n 2^-64 of the exact ratio, then rounded to float64
        assert np.all(np.abs(a - b) <= 4 * n * 2.0 ** -64 + 2.0 ** -52 * np.maximum(a, b)), name
    c = CASES["outside1000"]
    far = np.array([1e6 + 0j, -3e5j])                           # |z|^1000 overflows long double
    assert not np.all(np.isfinite(R.backward_error_unscaled(c, far)))
    assert np.all(np.abs(R.backward_error(c, far) - 1.0) < 1e-4)   # far outside every root: p(z) ~ z^n, the ratio tends to 1


@pytest.mark.parametrize("name", list(CASES))
def test_restated_iteration_meets_both_bounds_and_a_duplicate_does_not(name):
    c = CASES[name]
    n = c.size - 1
    z, tol = _solved(name)
    assert np.all(np.isfinite(z))
    assert np.max(R.backward_error(c, z)) <= R.bound(n)
    assert R.completeness(c, z) <= tol
    if n > 1:
        assert R.worst_duplicate(c, z) > tol, (R.worst_duplicate(c, z), tol)


def test_plain_horner_loses_the_whole_polynomial_to_one_outside_root():
    c = CASES["outside256"]
    assert np.sum(np.isfinite(R.aberth(c, safe=False))) <= 1        # the NaN reaches every other root's pair sum
    assert np.all(np.isfinite(R.aberth(c, safe=True)))


def test_badly_scaled_ring_meets_the_backward_bound_but_not_the_completeness_tolerance():
    c = R.badly_scaled_case()
    assert np.abs(c).max() > 1e8
    z = R.aberth(c)
    assert np.all(np.isfinite(z)) and np.max(R.backward_error(c, z)) <= R.bound(c.size - 1)
    assert R.completeness(c, z) > (c.size - 1) * R.U          # why the selected seeds are the well scaled ones


def test_multiple_roots_stay_finite_and_backward_stable():
    for name, c, root, m in R.multiple_cases():
        z = R.aberth(c)
        assert np.all(np.isfinite(z)), name
        assert np.max(R.backward_error(c, z)) <= R.bound(c.size - 1), name
        assert R.multiple_root_distance(z, root, m) < (c.size * R.U) ** (1.0 / m) * 100, name


def test_trim_follows_the_oracle_and_every_trimmed_row_is_solvable():
    rows = R.trim_rows()
    seen = set()
    for i, row in enumerate(rows):
        core, tz = R.trim(row)
        count = 0 if core is None else core.size - 1 + tz
        assert count == O.poly_roots(row).size, i
        seen.add(count)
        if core is not None:
            z = R.aberth(core)
            assert np.max(R.backward_error(core, z)) <= R.bound(core.size - 1), i
            assert R.completeness(core, z) <= R.completeness_tolerance(core), i
        core0, tz0 = R.trim(row, 0.0)
        assert (0 if core0 is None else core0.size - 1 + tz0) == np.roots(row).size, i
    assert seen == {0, 40, 62, 63, 64, 65}
    c, tz = R.trim(np.array([0.0, 2.0, -3.0, 1.0, 0.0, 0.0]), 0.0)
    assert tz == 2 and c.tolist() == [2.0, -3.0, 1.0]


def test_numerator_reference_agrees_with_the_oracle():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(300).astype(np.float32)
    a = R.ring(8, 708)[0]
    for n_len in (1, 5, 300):
        b, s = R.fir_numerator(a, x, n_len, 0.37, 200)
        ref = O.fir_numerator(a, x[:n_len].astype(np.float64) / 0.37, 200)
        assert np.all(np.abs(b - ref.astype(R.LD)) <= (8 + 3) * R.U * s)
        assert np.all(b[n_len + 8 :] == 0)
