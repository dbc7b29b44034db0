"""
The AR restatement (tests/ar_ref.py) tested without a GPU: its two formulations of the Gram matrix against each other, the
exact rational solve against lstsq where lstsq is good, the TEETH of the backward-error yardstick on the very grid the GPU
module runs, and the float64 emulation of the condition estimate on every input family.

Measured (float64 NumPy, this grid): the honest normal-equation solution uses at most 2.6 % of eta_allowance; a restatement
with the first row, the last row or row 4096 removed exceeds the allowance at least 3.1e5 fold.  Emulated estimate /
cond_2(G): minimum 0.305 (order 12, Butterworth-8 high-pass at 0.2 Nyquist; 0.385 at order 8), 2.1 on the class inputs of the
GPU module, maximum 72 (order 129): within [0.25, p].
"""
import numpy as np
import pytest

import ar_ref as R


def test_definition_agrees_with_the_lag_sum_formulation():
    R.need_longdouble()
    worst = 0.0
    for p, rows, f64 in ((1, 3, False), (2, 5, False), (12, 25, True), (13, 300, False), (64, 129, False), (65, 4097, False),
                         (33, 8193, True), (65, 1000, True)):
        s = R.samples(R.grid_signal(p, rows, f64=f64), 0.3 if f64 else None, f64)
        Gd, rd = R.gram_ld(s, p, method="definition")
        Gl, rl = R.gram_ld(s, p, method="lag")
        scale = np.max(np.abs(Gd))
        d = float(max(np.max(np.abs(Gd - Gl)), np.max(np.abs(rd - rl))) / scale)
        worst = max(worst, d)
        assert d <= 1e-17, (p, rows, d)
        assert np.array_equal(Gd, Gd.T)
        # and both are the float64 Gram matrix to float64 accuracy
        A, y = R.design(s, p)
        assert np.max(np.abs((A.T @ A).astype(R.LD) - Gd)) <= 4 * rows * R.U * float(scale)
    print(f"AR-REF definition vs lag sums: worst {worst:.2e} of the largest entry")
    G0, _ = R.gram_ld(s, p)
    G1, _ = R.gram_ld(s, p, ridge=1e-3)
    assert np.array_equal(np.diag(G1), np.diag(G0) + R.LD(1e-3)) and np.array_equal(np.triu(G1, 1), np.triu(G0, 1))


def test_samples_round_the_division_in_float64():
    x = R.stationary(3, 64, 0.5, f64=True)
    s = R.samples(x, 0.3, True)
    assert s.dtype == np.float64 and np.array_equal(s, x / 0.3)
    x32 = R.stationary(3, 64, 0.5)
    assert x32.dtype == np.float32 and np.array_equal(R.samples(x32), x32.astype(np.float64))
    with pytest.raises(AssertionError):
        R.samples(x32, None, True)


def test_exact_fit_against_lstsq_on_a_well_conditioned_case():
    for p, rows, f64 in ((8, 200, False), (33, 400, True)):
        s = R.samples(R.grid_signal(p, rows, f64=f64), 0.3 if f64 else None, f64)
        A, y = R.design(s, p)
        ref = np.linalg.lstsq(A, y, rcond=None)[0]
        a = R.exact_fit(s, p)
        assert np.max(np.abs(a - ref)) / np.max(np.abs(ref)) <= 1e-13
        if R.LONGDOUBLE_OK:                                  # the exact solution leaves nothing but its own rounding
            G, r = R.gram_ld(s, p)
            assert R.eta(G, r, a) <= 2 * R.U


def test_pivots_and_estimate_on_a_known_matrix():
    G = np.diag([4.0, 9.0, 1.0, 16.0])
    assert R.pivots_ld(G) == (4.0, 1.0)
    # diagonal G: G^-2 applied to the normalised alternating vector, times the trace
    v = np.array([1, -1, 1, -1]) / 2.0 / np.diag(G)
    v = v / np.linalg.norm(v) / np.diag(G)
    assert abs(R.estimate_f64(G) - 30.0 * np.linalg.norm(v)) <= 1e-13 * 30.0


def _grid():
    return [(p, rows) for p in R.ORDERS_A for rows in sorted(R.rows_for(p))]


def test_eta_has_teeth_on_the_gpu_grid():
    """On every (order, rows) case of tests/test_gpu_ar.py (a): the float64 normal equations stay under 5 % of the allowance,
    and the solution of the problem with the first row, the last row or row 4096 (the first of the second chunk) removed
    exceeds the allowance at least 100 fold."""
    R.need_longdouble()
    worst_share, least_excess = 0.0, np.inf
    for p, rows in _grid():
        assert rows >= 2
        s = R.samples(R.grid_signal(p, rows))
        G, r = R.gram_ld(s, p)
        allow = R.eta_allowance(rows, p)
        A, y = R.design(s, p)
        share = R.eta(G, r, np.linalg.solve(A.T @ A, A.T @ y)) / allow
        worst_share = max(worst_share, share)
        assert share <= 0.05, (p, rows, share)
        for which in (0, rows - 1) + ((R.LAG_CHUNK,) if rows > R.LAG_CHUNK else ()):
            excess = R.eta(G, r, R.drop_row_solution(s, p, which)) / allow
            least_excess = min(least_excess, excess)
            assert excess >= 100.0, (p, rows, which, excess)
    print(f"AR-REF teeth: float64 NumPy uses at most {100 * worst_share:.2f} % of the allowance; "
          f"a dropped boundary row exceeds it at least {least_excess:.1e} fold")


def test_emulated_condition_estimate_against_cond2():
    """estimate_f64 / cond_2(G) on every input family: one-pole noise (the grid, orders <= 129), and the low- and high-passed
    classes R and D.  Upper bound p (rigorous); the minimum is PRINTED and recorded in the module docstring: the device
    tests hold info[3] above 0.25 cond_2."""
    ratios = {}
    for p, rows in _grid():
        if p > 129:
            continue
        s = R.samples(R.grid_signal(p, rows))
        A, _ = R.design(s, p)
        ratios[("pole", p, rows)] = R.estimate_f64(A.T @ A) / R.cond2(s, p)
    for p, rows, kind, cls, width in R.CLASS_CASES:
        s = R.samples(R.class_signal(p, rows, kind, width))
        A, _ = R.design(s, p)
        sv = np.linalg.svd(A, compute_uv=False)
        assert R.in_class(cls, p, rows, (sv[0] / sv[-1]) ** 2, sv[-1] / sv[0]), (p, kind, cls, (sv[0] / sv[-1]) ** 2)
        if cls == "R":                                       # (class D: a float64 Cholesky factor of G is noise)
            ratios[(kind, cls, p)] = R.estimate_f64(A.T @ A) / R.cond2(s, p)
        else:
            # the same two inverse iterations through the SVD of A (G^-1 v = V diag(1/sigma^2) V^T v)
            _, sg, Vt = np.linalg.svd(A, full_matrices=False)
            v = np.where(np.arange(p) & 1, -1.0, 1.0)
            for _ in range(2):
                v = v / np.linalg.norm(v)
                v = Vt.T @ ((Vt @ v) / sg ** 2)
            ratios[(kind, cls, p)] = float(np.sum(sg ** 2) * np.linalg.norm(v)) / R.cond2(s, p)
    # mildly high-passed noise at EVEN order: the alternating start vector is orthogonal to the constant vector, the weak
    # direction there, and two iterations recover only part of it -- the estimate falls BELOW cond_2(G)
    for p, order, cutoff in ((8, 8, 0.2), (64, 4, 0.05), (12, 8, 0.2), (64, 8, 0.1)):
        s = R.samples(R.band_limited(11 * p, p + 2400, "high", cutoff, order=order))
        A, _ = R.design(s, p)
        ratios[("high-mild", f"butter{order}@{cutoff}", p)] = R.estimate_f64(A.T @ A) / R.cond2(s, p)
    lo = min(ratios, key=ratios.get)
    hi = max(ratios, key=ratios.get)
    for k, v in ratios.items():
        if k[0] != "pole":
            print(f"AR-REF est/cond {k}: {v:.3f}")
    print(f"AR-REF est/cond minimum {ratios[lo]:.3f} at {lo}, maximum {ratios[hi]:.3f} at {hi}")
    for k, v in ratios.items():
        p = k[1] if k[0] == "pole" else k[2]
        assert 0.25 <= v <= p * (1 + 1e-6), (k, v)
