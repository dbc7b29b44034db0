"""
Restatement of the MLS measurement (audio_analysis_amd/analyse/mls.py, audio_analysis_amd/csrc/ira_mls.hip) in NumPy, for
the tests; nothing of the package is used: the bits come from the plain recurrence, the tables from their definitions.
Helper module, like minphase_ref.py / fdw_ref.py: it holds no tests.

What is here
  * bits / sequence / tables(order, taps): a[n], s[n] = 1 - 2 a[n], G and out by the plain loops of the definition;
  * fold(x, b, P, R): Y in float64, r ascending from 0.0; fold_terms: the float64 squares whose sums are E and D, restated
    term by term so that only the ORDER of the device's additions is left open, and sums_ld their long-double sums;
  * fwht(w): the natural-order transform, stages h = 1, 2, 4 .. in that order, (lo, hi) -> (lo + hi, lo - hi);
  * fast_chain: fold -> scatter through G -> fwht -> (W[out] - W[0]) / float64(2^m R), the float64 value and its float32;
  * direct_ld: c[k] = sum over n of s[n] Y[(n + k) mod P] and h = (c - sum Y) / (2^m R) in numpy.longdouble, O(P^2), from
    the same float64 Y;
  * grid_int64: the same in int64 for samples on the PCM16 grid k / 32768, exact up to the one division;
  * sampled_ld: the same h at chosen positions from math.fsum sums, O(P) a position, for the orders direct_ld cannot afford;
  * sparse_response / sparse_period: twelve taps k / 256 and their period under the amplitude-0.5 sequence, for which the
    chain is exact and gives 0.5 h back;
  * bound(m, R, Y) for inputs off the grid.

The bound (u = 2^-53, gamma_k = k u / (1 - k u)).  Every W[i] is a signed sum of the 2^m entries of w formed by m stages of
one addition or subtraction each, so the computed value is sum_j +-w[j] (1 + theta_ij) with |theta_ij| <= gamma_m (Higham,
Accuracy and Stability of Numerical Algorithms, lemma 3.1), i.e. |W^[i] - W[i]| <= gamma_m sum |Y|.  The subtraction
W[out[k]] - W[0] and the division by 2^m R (a product of exact values: no error of its own) add one rounding each, which
turns gamma_m into gamma_(m+2):
    |h_float64 - h_true| <= gamma_(m+2) sum |Y| / (2^m R)
This is the figure the tests assert.  It charges the transform's error once: a worst-case analysis that lets the errors of
W[out[k]] and of W[0] take opposite signs in every term doubles the first factor.  The two values share every stage below
the lowest set bit of out[k] and their remaining errors are rounding errors of unrelated partial sums; the tests print the
largest observed error over the bound (0.24 over the cases of tests/test_mls_cpu.py, reached at order 2).
h_true is taken from the float64 Y: the fold's own rounding (gamma_(R-1) per sample) belongs to the definition of Y.
"""
import numpy as np

U = 2.0 ** -53

TAPS = {2: (2, 1), 3: (3, 2), 4: (4, 3), 5: (5, 3), 6: (6, 5), 7: (7, 6), 8: (8, 6, 5, 4), 9: (9, 5), 10: (10, 7),
        11: (11, 9), 12: (12, 6, 4, 1), 13: (13, 4, 3, 1), 14: (14, 5, 3, 1), 15: (15, 14), 16: (16, 15, 13, 4),
        17: (17, 14), 18: (18, 11), 19: (19, 6, 2, 1), 20: (20, 17), 21: (21, 19)}


def gamma(k):
    return k * U / (1.0 - k * U)


def bits(order, taps=None, count=None):
    """a[n] = XOR over t of a[n - t], a[0 .. order-1] = 1: the plain recurrence, one step at a time."""
    taps = TAPS[order] if taps is None else tuple(taps)
    count = (1 << order) - 1 if count is None else count
    a = [1] * order
    for n in range(order, count):
        v = 0
        for t in taps:
            v ^= a[n - t]
        a.append(v)
    return np.array(a[:count], dtype=np.uint8)


def sequence(order, taps=None):
    return 1 - 2 * bits(order, taps).astype(np.int64)


def tables(order, taps=None):
    """(G, out) int64 by their definitions: G[j] = 1 << j for j < m, XOR over t of G[j - t] after; S[i] = sum a[i + q] << q;
    out[k] = S[(P - k) mod P]."""
    taps = TAPS[order] if taps is None else tuple(taps)
    p = (1 << order) - 1
    g = [1 << j for j in range(order)]
    for j in range(order, p):
        v = 0
        for t in taps:
            v ^= g[j - t]
        g.append(v)
    a = bits(order, taps, p + order).astype(np.int64)
    s = np.zeros(p, dtype=np.int64)
    for q in range(order):
        s += a[q : q + p] << q
    return np.array(g[:p], dtype=np.int64), s[(p - np.arange(p)) % p]


def fold(x, b, p, periods):
    """Y[n] = sum over r ascending, from 0.0, of float64(x[b + r P + n])."""
    x = np.asarray(x, dtype=np.float32)
    y = np.zeros(p, dtype=np.float64)
    for r in range(periods):
        y = y + x[b + r * p : b + (r + 1) * p].astype(np.float64)
    return y


def fold_terms(x, b, p, periods):
    """(Y, Y^2 (P,), the residual squares (P, R)) in float64, each term formed as the kernel forms it: q = Y / float64(R),
    d = float64(x) - q, d * d; no residual terms when R = 1."""
    x = np.asarray(x, dtype=np.float32)
    y = fold(x, b, p, periods)
    with np.errstate(all="ignore"):
        if periods > 1:
            q = y / np.float64(periods)
            d = x[b : b + periods * p].astype(np.float64).reshape(periods, p).T - q[:, None]
            res = d * d
        else:
            res = np.zeros((p, 0))
        return y, y * y, res


def sums_ld(x, b, p, periods):
    """(E, D, sum |terms of E|, sum |terms of D|) as long-double sums of fold_terms' float64 terms."""
    _, e, d = fold_terms(x, b, p, periods)
    e, d = e.astype(np.longdouble), d.astype(np.longdouble)
    return e.sum(), d.sum(), np.abs(e).sum(), np.abs(d).sum()


def fwht(w):
    """The transform of the last axis (a power of two), natural order, stages h = 1, 2, 4 .. in that order."""
    w = np.array(w, dtype=np.float64)
    n = w.shape[-1]
    lead = w.shape[:-1]
    h = 1
    with np.errstate(all="ignore"):
        while h < n:
            v = w.reshape(*lead, n // (2 * h), 2, h)
            lo, hi = v[..., 0, :].copy(), v[..., 1, :].copy()
            v[..., 0, :] = lo + hi
            v[..., 1, :] = lo - hi
            h *= 2
    return w


def scatter(y, g, order):
    w = np.zeros(1 << order, dtype=np.float64)
    w[np.asarray(g)] = y
    return w


def finish(wt, out, order, periods):
    """(h float64, h float32) = (W[out] - W[0]) / float64(2^m R) and its rounding to float32."""
    with np.errstate(all="ignore"):
        h64 = (wt[np.asarray(out)] - wt[0]) / np.float64((1 << order) * periods)
        return h64, h64.astype(np.float32)


def fast_chain(x, b, order, periods, taps=None, tabs=None):
    """dict(Y, w, W, h64, h) of the stage-ordered float64 chain."""
    p = (1 << order) - 1
    g, out = tabs if tabs is not None else tables(order, taps)
    y = fold(x, b, p, periods)
    w = scatter(y, g, order)
    wt = fwht(w)
    h64, h = finish(wt, out, order, periods)
    return dict(Y=y, w=w, W=wt, h64=h64, h=h)


def _correlate(s, y):
    """c[k] = sum over n of s[n] y[(n + k) mod P], in y's dtype."""
    p = y.size
    return np.correlate(np.concatenate([y, y[: p - 1]]), s.astype(y.dtype), mode="valid")


def direct_ld(y, order, periods, taps=None):
    """h in long double from the float64 Y: (c[k] - sum Y) / (2^m R), c by the direct O(P^2) sums."""
    y = np.asarray(y, dtype=np.float64).astype(np.longdouble)
    c = _correlate(sequence(order, taps), y)
    return (c - y.sum()) / np.longdouble((1 << order) * periods)


def grid_int64(x, b, order, periods, taps=None):
    """The chain for samples on the PCM16 grid, in int64: K = 32768 x exactly, Y, c and sum Y as integers; the only rounding
    is the division by 2^m R (the division by 32768 is exact).  Returns (h float64, h float32)."""
    p = (1 << order) - 1
    x = np.asarray(x, dtype=np.float32)
    k = np.rint(x.astype(np.float64) * 32768.0).astype(np.int64)
    assert np.array_equal(k.astype(np.float64) / 32768.0, x.astype(np.float64)), "samples are not on the PCM16 grid"
    y = k[b : b + periods * p].reshape(periods, p).sum(axis=0)
    num = _correlate(sequence(order, taps), y) - y.sum()
    assert np.abs(num).max() < 1 << 53
    h64 = (num.astype(np.float64) / 32768.0) / np.float64((1 << order) * periods)
    return h64, h64.astype(np.float32)


def bound(order, periods, y):
    """gamma_(m+2) sum |Y| / (2^m R): see the module's docstring."""
    return gamma(order + 2) * float(np.sum(np.abs(np.asarray(y, dtype=np.float64)))) / float((1 << order) * periods)


def sparse_response(order, seed, taps=12):
    """A response of `taps` non-zero values k / 256, 0 < |k| <= 255, at seeded indices with 0 and P - 1 among them."""
    p = (1 << order) - 1
    rng = np.random.default_rng(seed)
    idx = np.concatenate([[0, p - 1], 1 + rng.choice(p - 2, taps - 2, replace=False)])
    h = np.zeros(p)
    h[idx] = rng.integers(1, 256, taps) * rng.choice([-1, 1], taps) / 256.0
    return h


def sparse_period(h, s, amplitude=0.5):
    """One steady-state period y[n] = sum over j of h[j] amplitude s[(n - j) mod P] of a sparse h, tap by tap.  For
    sparse_response and amplitude 0.5 every partial sum is a multiple of 2^-9 below 2^3: exact, in float32 as well."""
    s = np.asarray(s, dtype=np.float64)
    y = np.zeros(h.size)
    for j in np.flatnonzero(h):
        y += h[j] * amplitude * np.roll(s, j)
    return y


def sample_positions(order, seed, count):
    """k = 0, 1, P - 1 and count - 3 seeded ones."""
    p = (1 << order) - 1
    rng = np.random.default_rng(seed)
    return sorted({0, 1, p - 1} | {int(k) for k in 2 + rng.choice(p - 3, count - 3, replace=False)})


def sampled_ld(y, s, order, periods, ks):
    """h[k] at the positions ks from correctly rounded sums: c[k] = math.fsum of the signed Y (each term s[n] Y[(n + k) mod P]
    is +-Y, exact), sum Y by math.fsum, then (c - sum Y) / (2^m R) in long double.  O(P) a position, any order."""
    import math
    y = np.asarray(y, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    sy = np.longdouble(math.fsum(y.tolist()))
    scale = np.longdouble((1 << order) * periods)
    return np.array([(np.longdouble(math.fsum((s * np.roll(y, -k)).tolist())) - sy) / scale for k in ks], dtype=np.longdouble)


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)
