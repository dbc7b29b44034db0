"""
Reference for the AR normal-equation kernels (ira_ar.hip: ar_lag_kernel, ar_gram_kernel, ar_solve_wave_kernel,
ar_solve_kernel, ar_grad_kernel, ar_lag_dd_kernel / ar_solve_dd_kernel, ar_minnorm_kernel): the yardsticks, the input
families and the case grid of tests/test_gpu_ar.py.  Helper module, like roots_ref.py / decay_ref.py: it holds no tests and
imports nothing of the product; tests/test_ar_ref_cpu.py pins it without a GPU.

Why not numpy.linalg.lstsq at a fixed tolerance: at cond(G) ~ 1e8 .. 1e15 float64 lstsq itself sits 1e-9 .. 1e-6 from the exact
solution, so "within 1e-6 of lstsq" passes a solver that is a thousand times worse than it should be, and on well-conditioned
inputs 1e-7 is nine orders above what the kernels deliver.  The yardsticks here are

  eta(G, r, a)         normwise backward error of the normal equations, ||G a - r||_inf / (||G||_inf ||a||_inf + ||r||_inf),
                       with G and r restated in long double BY DEFINITION (gram_ld) from the float64 samples the device uses
                       (samples()).  Bound eta_allowance(rows, p).  It sees every kernel in front of the root finder at once:
                       a lag sum that loses or doubles a row, a wrong head / tail correction, a panel of the blocked Cholesky
                       that misses a column all move G or the solution by far more than rounding.
  exact_fit(s, p)      the exact rational solution (integer Gram matrix, 90-digit solve): the forward-error reference where
                       refinement and the double-double path claim more than lstsq can certify.
  pivots_ld, cond2, estimate_f64   the info record: Cholesky pivots in long double, cond_2(G) from the singular values of A,
                       and a float64 restatement of the kernel's condition estimate (two inverse iterations from the
                       alternating vector, times the trace).
"""
import math

import numpy as np

LD = np.longdouble
LONGDOUBLE_OK = bool(np.finfo(LD).eps < 2e-19)
U = 2.0 ** -53
LAG_CHUNK = 4096            # rows per workgroup of ar_lag_kernel / ar_grad_kernel / ar_lag_dd_kernel
DEFINITION_MAX_P = 130      # gram_ld: above this order the lag-sum formulation (the definition costs O(p^2 rows))


def need_longdouble():
    import pytest
    if not LONGDOUBLE_OK:
        pytest.skip("np.longdouble has no 64-bit mantissa on this machine: no reference more precise than float64")


# ------------------------------------------------------------------------------------------------------- the samples
def samples(x, divisor=None, is_f64=False):
    """The float64 values every AR kernel uses: (double)x / divisor, the division ROUNDED in float64 (the device rounds there
    too: lds[m] = (double)v / div), so that the references start from identical numbers."""
    x = np.asarray(x)
    assert x.dtype == (np.float64 if is_f64 else np.float32), x.dtype
    s = x.astype(np.float64)
    if divisor is not None:
        s = s / np.float64(divisor)
    return s


def design(s, p, dtype=np.float64):
    """A[n - p, k - 1] = s[n - k] and y[n - p] = -s[n], n = p .. N-1, k = 1 .. p  (min ||A a - y||: the covariance method)."""
    s = np.asarray(s).astype(dtype)
    n = np.arange(p, s.size)
    A = np.stack([s[n - k] for k in range(1, p + 1)], axis=1) if n.size else np.zeros((0, p), dtype)
    return A, -s[n]


# ------------------------------------------------------------------------------------------------------- G and r
def _gram_definition(s, p):
    A, y = design(s, p, LD)
    At = np.ascontiguousarray(A.T)                       # sums along the contiguous axis are pairwise in NumPy
    G = np.empty((p, p), LD)
    for k in range(p):
        G[k, k:] = (At[k][None, :] * At[k:]).sum(axis=1)
        G[k:, k] = G[k, k:]
    r = (At * y[None, :]).sum(axis=1)
    return G, r


def _gram_lag(s, p):
    """Phi[a][b] = sum_{n=p}^{N-1} s[n-a] s[n-b]: row 0 by p+1 lag sums, then down every diagonal with the shift identity
    Phi[a+1][b+1] = Phi[a][b] + s[p-1-a] s[p-1-b] - s[N-1-a] s[N-1-b], all in long double: O(p N + p^2)."""
    s = np.asarray(s, np.float64).astype(LD)
    N = s.size
    phi0 = np.array([(s[p:] * s[p - d : N - d]).sum() for d in range(p + 1)], LD)
    Phi = np.zeros((p + 1, p + 1), LD)
    for d in range(p + 1):
        a = np.arange(p - d)                              # steps (a, a+d) -> (a+1, a+d+1)
        step = s[p - 1 - a] * s[p - 1 - a - d] - s[N - 1 - a] * s[N - 1 - a - d]
        diag = phi0[d] + np.concatenate([np.zeros(1, LD), np.cumsum(step)])
        idx = np.arange(p + 1 - d)
        Phi[idx, idx + d] = diag
        Phi[idx + d, idx] = diag
    return Phi[1:, 1:].copy(), -Phi[0, 1:].copy()


def gram_ld(s, p, ridge=0.0, method=None):
    """(G, r) in long double: G = A^T A + ridge I, r = A^T y = -A^T s[n].  method "definition" forms the products row by row
    (pairwise sums), "lag" uses the shift structure; None picks the definition up to order DEFINITION_MAX_P.  The two agree to
    1e-17 of the largest entry (tests/test_ar_ref_cpu.py)."""
    if method is None:
        method = "definition" if p <= DEFINITION_MAX_P else "lag"
    G, r = _gram_definition(s, p) if method == "definition" else _gram_lag(s, p)
    if ridge:
        G = G + LD(ridge) * np.eye(p, dtype=LD)
    return G, r


# ------------------------------------------------------------------------------------------------------- backward error
def eta(G, r, a):
    """Normwise backward error of a (the p coefficients a_1 .. a_p) as a solution of G a = r, evaluated in long double."""
    a = np.asarray(a, np.float64).astype(LD)
    res = np.max(np.abs(G @ a - r))
    den = np.max(np.sum(np.abs(G), axis=1)) * np.max(np.abs(a)) + np.max(np.abs(r))
    return float(res / den) if den > 0 else float(res)


def eta_allowance(rows, p):
    """(rows + 4 p + 8) u, u = 2^-53: what a float64 solver of the normal equations may leave as eta against the EXACT G, r.

      rows u   forming an entry of G or r: a sum of `rows` products in float64 in ANY order is off by at most gamma_rows ~
               rows u of the sum of their moduli (Higham, Accuracy and Stability, 3.1; fused multiply-adds and blocked or
               chunked orders only lower it), and ||.||_inf of the perturbation is bounded the same way row by row;
      3 p u    Cholesky plus the two triangular solves: (G + dG) a = r with |dG| <= gamma_{3p+1} |L| |L^T| (Higham 10.4),
               and || |L| |L^T| || <= p ||G|| in the worst case only -- measured factors are ~1, so 3 p u stands for it;
      p u      the head / tail corrections of the shift identity: 2 p further terms per entry (compensated on the device);
      8 u      the division by the divisor, the final rounding of a, and the reduction over chunks.

    This is a worst-case budget, not a fit to any solver: float64 NumPy normal equations use at most 2.6 % of it on the grid of
    tests/test_gpu_ar.py (order 1, where it is smallest), and a restatement that drops ONE boundary row exceeds it at least
    3e5 fold on stationary inputs (tests/test_ar_ref_cpu.py asserts 5 % and 100 x)."""
    return (rows + 4 * p + 8) * U


# ------------------------------------------------------------------------------------------------------- exact solution
def _to_int(x, shift):
    m, e = math.frexp(float(x))
    mi = int(m * 9007199254740992.0)                      # m * 2^53, exact
    sh = e - 53 - shift
    return mi << sh if sh >= 0 else mi >> -sh            # the right shift drops zeros only (shift = the smallest exponent)


def exact_fit(s, p, dps=90):
    """The exact least-squares coefficients a_1 .. a_p of the float64 samples s, rounded once to float64: the samples are scaled
    to integers (a common power of two cancels from G a = r), G = A^T A and r = A^T y are formed in Python integers (exactly),
    and G a = r is solved by mpmath.lu_solve with `dps` digits (raised when the integers need more).  A full-rank problem is
    the caller's business."""
    from mpmath import mp
    s = np.asarray(s, np.float64)
    nz = s[s != 0.0]
    shift = min(math.frexp(float(v))[1] for v in nz) - 53
    z = np.array([_to_int(v, shift) for v in s], dtype=object)
    assert all(math.ldexp(float(v), shift) == float(x) for v, x in zip(z[:64], s[:64]))
    n = np.arange(p, s.size)
    A = np.stack([z[n - k] for k in range(1, p + 1)], axis=1)
    G = A.T.dot(A)
    r = -A.T.dot(z[n])
    bits = max(int(v).bit_length() for v in np.diag(G))
    saved = mp.dps
    try:
        mp.dps = max(dps, int(2 * bits * 0.30103) + 20)
        x = mp.lu_solve(mp.matrix(G.tolist()), mp.matrix([int(v) for v in r]))
        return np.array([float(v) for v in x], np.float64)
    finally:
        mp.dps = saved


# ------------------------------------------------------------------------------------------------------- the info record
def pivots_ld(G):
    """(largest, smallest) diagonal entry of the Cholesky factor of G in long double (info[1], info[2])."""
    G = np.asarray(G, LD)
    p = G.shape[0]
    L = np.zeros((p, p), LD)
    for k in range(p):
        v = G[k:, k] - L[k:, :k] @ L[k, :k]
        d = np.sqrt(v[0])
        L[k:, k] = v / d
        L[k, k] = d
    dg = np.diag(L)
    return float(dg.max()), float(dg.min())


def cond2(s, p, ridge=0.0):
    """cond_2(G) = (sigma_max^2 + ridge) / (sigma_min^2 + ridge) from the singular values of A in float64 (accurate to
    cond(A) u, where the eigenvalues of a float64 G would only be good to cond(G) u)."""
    A, _ = design(s, p)
    sv = np.linalg.svd(A, compute_uv=False)
    return float((sv[0] ** 2 + ridge) / (sv[-1] ** 2 + ridge))


def estimate_f64(G):
    """The kernels' condition estimate restated in float64: trace(G) * ||G^-1 G^-1 v|| with v the normalised alternating
    vector and a renormalisation in between (two inverse iterations on the Cholesky factor)."""
    from scipy.linalg import cho_factor, cho_solve
    G = np.asarray(G, np.float64)
    p = G.shape[0]
    c = cho_factor(G, lower=True)
    v = np.where(np.arange(p) & 1, -1.0, 1.0)
    for _ in range(2):
        v = v / np.sqrt(np.sum(v * v))
        v = cho_solve(c, v)
    return float(np.trace(G) * np.sqrt(np.sum(v * v)))


# ------------------------------------------------------------------------------------------------------- inputs
def stationary(seed, n, pole, f64=False):
    """Seeded white noise through y[n] = x[n] + pole y[n-1] (cond(G) <= ~1e3 for pole <= 0.9), the start-up transient cut off:
    STATIONARY, so that the first and the last row weigh as much as any other (on a decaying response a dropped last row
    hides in the float64 noise).  float32, or genuinely 53-bit float64 samples for the x_is_f64 path."""
    from scipy.signal import lfilter
    w = np.random.default_rng(seed).standard_normal(n + 256)
    y = lfilter([1.0], [1.0, -pole], w)[256:]
    y = y / np.max(np.abs(y)) * 0.9
    return y.astype(np.float64) if f64 else y.astype(np.float32)


def band_limited(seed, n, kind, cutoff, order=8):
    """Stationary noise through a Butterworth low-pass ("low") or high-pass ("high") at `cutoff` (fraction of Nyquist), float32:
    the ill-conditioned inputs.  Low-passed: weak direction at Nyquist (the alternating vector).  High-passed: weak direction
    at DC (the constant vector, orthogonal to the alternating one for even p)."""
    from scipy.signal import butter, sosfilt
    w = np.random.default_rng(seed).standard_normal(n + 4096)
    y = sosfilt(butter(order, cutoff, btype=kind + "pass", output="sos"), w)[4096:]
    return (y / np.max(np.abs(y)) * 0.9).astype(np.float32)


# ------------------------------------------------------------------------------------------------------- the case grid
ORDERS_A = (1, 2, 7, 9, 11, 12, 15, 63, 64, 65, 128, 129, 384, 385, 513, 1023, 1024)
POLES = (0.0, 0.5, 0.9)


def rows_for(p):
    """Row counts N - p of the backward-error grid: 2p+1 (short), 4095 / 4096 / 4097 (one chunk, exactly one, one row into the
    second), 8193 (one row into the third); from order 384 on only the shortest and 4097."""
    return (4097, 2 * p + 1) if p >= 384 else (4095, 8193, 2 * p + 1, 4096, 4097)       # the longest is never last


def grid_signal(p, rows, f64=False):
    """The element of the (order, rows) case: seed and pole follow from the case, so that every test sees the same samples."""
    return stationary(1000 * p + rows % 997, p + rows, POLES[(p + rows) % 3], f64=f64)


def drop_row_solution(s, p, which):
    """float64 normal-equation solution of the problem with ONE row removed (which = row index n - p): the mistake a lag-sum
    kernel makes when a chunk is a row short or a boundary row is counted for nobody."""
    A, y = design(s, p)
    keep = np.ones(A.shape[0], bool)
    keep[which] = False
    A, y = A[keep], y[keep]
    return np.linalg.solve(A.T @ A, A.T @ y)


# ---- the ill-conditioned classes (forward error against exact_fit) ----------------------------------------------------------
# class R (refined by ira_ar_refine):      4e9 < cond(G)  and  p cond(G) < 1e13: the estimate info[3] lies in [0.25 cond, p cond]
#                                          (measured lower, rigorous upper bound), i.e. surely in (1e9, 1e13]
# class D (double-double, ira_ar_exact):   cond(G) > 4e13  and  sigma_min / sigma_max > 10 eps max(rows, p) (lstsq's rank cut is
#                                          a decade away: a full-rank fit for the reference and for the device)
# (order, rows, kind, class, stop-band width as a fraction of Nyquist): Butterworth-8 cutoffs found by bisection on cond2
# for the geometric middle of class R and cond(G) = 1e15 (order 130 high-passed: 4e15 -- at 1e15 two refinement steps on the
# float64 factor still came within 1.6 x of the bound, too narrow a margin for the teeth); the tests ASSERT the class before
# they ask the device.
CLASS_CASES = (
    (33, 2436, "low", "R", 0.427), (33, 2436, "low", "D", 0.658), (33, 2436, "high", "R", 0.433), (33, 2436, "high", "D", 0.661),
    (64, 2436, "low", "R", 0.238), (64, 2436, "low", "D", 0.452), (64, 2436, "high", "R", 0.240), (64, 2436, "high", "D", 0.455),
    (96, 2400, "low", "R", 0.160), (96, 2400, "low", "D", 0.333), (96, 2400, "high", "R", 0.159), (96, 2400, "high", "D", 0.329),
    (130, 800, "low", "R", 0.114), (130, 800, "low", "D", 0.247), (130, 800, "high", "R", 0.116), (130, 800, "high", "D", 0.310),
)


def class_signal(p, rows, kind, width):
    return band_limited(7 * p, p + rows, kind, width if kind == "high" else 1.0 - width)


def in_class(cls, p, rows, cond, sv_ratio):
    if cls == "R":
        return 4e9 < cond and p * cond < 1e13
    return cond > 4e13 and sv_ratio > 10 * np.finfo(np.float64).eps * max(rows, p)
