"""Holds the echo-criterion restatement (tests/echo_ref.py) to closed forms, on a machine without a GPU."""
import numpy as np
import pytest

import echo_ref as R

FS = 48000.0


@pytest.mark.parametrize("n", [2.0 / 3.0, 1.0, 2.0, 0.5])
@pytest.mark.parametrize("d", [1, 7, 432])
def test_constant_magnitude_gives_a_ramp_then_one_half(n, d):
    """|y| = a: W[m] = (m + 1) a^n, V[m] = a^n m (m + 1) / 2, ts[m] = m / (2 fs): EK[m] = m / (2 D) for m < D, 0.5 after."""
    m = 3000
    rng = np.random.default_rng(1)
    y = (0.37 * rng.choice([-1.0, 1.0], m)).astype(np.float32)
    ek, ts, w, v = R.ek_curve(y, 0, n, d, FS, m)
    tol = R.tolerance(m, ts, d, FS)
    k = np.arange(m)
    want = np.where(k < d, k / (2.0 * d), 0.5)
    assert np.max(np.abs(ek - want)) <= tol
    assert abs(ts[-1] - (m - 1) / (2.0 * FS)) <= tol * d / FS
    assert tol < 1e-8


@pytest.mark.parametrize("n", [2.0 / 3.0, 1.0])
@pytest.mark.parametrize("g", [0.11, 0.5, 1.0])
@pytest.mark.parametrize("k,d,m", [(700, 432, 2000), (100, 672, 500), (5, 3, 40)])
def test_two_impulses(n, g, k, d, m):
    """A unit impulse at 0 and g at sample k: EK = k g^n / ((1 + g^n) D) for k <= m < min(k + D, M), 0 elsewhere."""
    y = np.zeros(m + 50, np.float32)
    y[0], y[k] = 1.0, g
    ek, ts, w, v = R.ek_curve(y, 0, n, d, FS, m)
    gn = float(np.float32(g)) ** n
    want = np.zeros(m)
    want[k : min(k + d, m)] = k * gn / ((1.0 + gn) * d)
    tol = R.tolerance(m, ts, d, FS)
    assert np.max(np.abs(ek - want)) <= tol + 4e-16 * want.max()
    assert R.first_at_or_above(ek, 0.5 * want.max()) == k
    assert R.first_at_or_above(ek, 2.0 * want.max() + 1.0) == -1
    assert int(np.argmax(ek)) == k


def test_onset_shift_zero_samples_and_helpers():
    y = np.zeros(400, np.float32)
    y[37], y[137] = -2.0, 1.0
    assert R.onset(y) == 37
    ek, ts, w, v = R.ek_curve(y, 37, 2.0 / 3.0, 10, FS, 300)
    assert w[0] == 2.0 ** (2.0 / 3.0) and v[0] == 0.0 and ts[50] == 0.0 and ek[99] == 0.0 and ek[100] > 0.0
    silent, _, ws, _ = R.ek_curve(np.zeros(64, np.float32), 0, 2.0 / 3.0, 10, FS, 64)
    assert not silent.any() and not ws.any()                        # W == 0: ts = 0, no NaN
    assert [R.lag(9.0, fs) for fs in (22050, 44100, 48000, 96000)] == [198, 397, 432, 864]
    assert R.lag(14.0, 96000) == 1344 and R.lag(0.001, 8000) == 1
    assert R.guard(50.0, 44100) == 2205 and R.mmax(1000.0, 48000) == 48001 and R.mmax(None, 48000) is None
    assert R.eval_len(48000, 100, 48000) == 48000 - 100 - 2400 and R.eval_len(480000, 0, 48000) == 48001
    assert R.eval_len(2000, 0, 48000, max_tau_ms=None) == -400
    sm = R.step_max(np.array([0.0, 3.0, 1.0, 2.0, 5.0]), 2)
    assert sm.dtype == np.float32 and list(sm) == [3.0, 2.0, 5.0]
    assert [R.rating(v, 0.9, 1.0) for v in (0.89, 0.9, 0.99, 1.0)] == ["inaudible", "marginal", "marginal", "audible"]


def test_interval_contains_the_point_values():
    rng = np.random.default_rng(5)
    y = (rng.standard_normal(4000) * np.exp(-np.arange(4000) / 600.0)).astype(np.float32)
    y[2000:] += 1.5 * y[:2000]
    for n in (2.0 / 3.0, 1.0):
        ek, _, _, _ = R.ek_curve(y, 3, n, 432, FS, 3500)
        lo, hi = R.ek_interval(y, 0.0, 3, n, 432, FS, 3500)
        assert np.max(np.abs(lo - ek)) <= 1e-12 and np.max(np.abs(hi - ek)) <= 1e-12
        lo, hi = R.ek_interval(y, 1e-6, 3, n, 432, FS, 3500)
        assert np.all(lo <= ek) and np.all(ek <= hi) and np.max(hi - lo) < 0.05
