"""
Reference for the polynomial root finder and the FIR numerator (ira_roots.hip: poly_roots_kernel, fir_numerator_kernel): the
yardsticks, the polynomial generators and the case lists of tests/test_gpu_roots.py.  Helper module, like decay_ref.py /
sti_ref.py: it holds no tests and imports nothing of the product; tests/test_roots_ref_cpu.py pins it without a GPU.

Why not numpy.roots: at degree 512 the roots of a float64-rounded polynomial move by 1e-2 and the companion-matrix
eigenvalues carry a backward error of 1e3 .. 1e15 u where an Aberth iteration leaves tens of u.  The yardsticks are

  backward_error(c, z)   |p(z)| / sum_k |c_k| |z|^(n-k) per root, in long double, evaluated SCALED (Horner on c at z for
                         |z| <= 1, on the reversed coefficients at 1/z otherwise: the same ratio without overflow).
                         Bound 4 n u, u = 2^-53, n the degree after trimming: Horner's own float64 rounding error is
                         gamma_2n ~ 2 n u of that same sum (Higham, Accuracy and Stability of Numerical Algorithms, 5.1), no
                         float64 root finder that evaluates the polynomial can certify less, and 2x covers the last update.
  completeness(c, z)     |sum z_k + c_1 / c_0| / max(1, sum |z_k|) in long double (Vieta): a duplicated or missing root, which
                         n copies of one root would hide from the backward error.  Tolerance: 100 x what numpy.roots leaves
                         on the same polynomial, floored at n u.  The companion matrix keeps its trace, so numpy.roots
                         leaves 1e-18 .. 1e-15 on every case here and the tolerance is in effect the floor n u.

aberth() restates the kernel's iteration in NumPy (start circle, Jacobi sweeps, stop rule, sweep cap); safe=False evaluates
p and p' by plain Horner everywhere, which overflows for |z|^n > 1.8e308.
"""
import functools

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
LONGDOUBLE_OK = bool(np.finfo(LD).eps < 2e-19)
U = 2.0 ** -53
MAX_SWEEPS = 200
TRAIL_EPS = 1e-14


def need_longdouble():
    import pytest
    if not LONGDOUBLE_OK:
        pytest.skip("np.longdouble has no 64-bit mantissa on this machine: no reference more precise than float64")


# ------------------------------------------------------------------------------------------------------- the yardsticks
def _horner(coef, x):
    acc = np.zeros(x.shape, dtype=np.result_type(coef.dtype, x.dtype)) + coef[0]
    for ck in coef[1:]:
        acc = acc * x + ck
    return acc


def backward_error(c, z):
    """Per root |p(z)| / sum_k |c_k| |z|^(n-k), float64 values computed in long double.  A root at exactly 0 of a polynomial
    whose constant term is 0 has error 0 (0 / 0 otherwise)."""
    c = np.asarray(c, dtype=np.float64).astype(LD)
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128)).astype(CLD)
    out = np.full(z.shape, np.nan, dtype=LD)
    ok = np.isfinite(z.real) & np.isfinite(z.imag)
    mod = np.abs(z)
    with np.errstate(all="ignore"):
        for inside in (True, False):
            m = ok & ((mod <= 1) if inside else (mod > 1))
            if not np.any(m):
                continue
            x, co = (z[m], c) if inside else (LD(1) / z[m], c[::-1])
            num = np.abs(_horner(co.astype(CLD), x))
            den = _horner(np.abs(co), np.abs(x))
            out[m] = np.where(num == 0, LD(0), num / den)
    return out.astype(np.float64)


def backward_error_unscaled(c, z):
    """The same ratio by plain Horner at z whatever its modulus (overflows for large |z|^n): pins the scaled evaluation."""
    c = np.asarray(c, dtype=np.float64).astype(LD)
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128)).astype(CLD)
    with np.errstate(all="ignore"):
        return (np.abs(_horner(c.astype(CLD), z)) / _horner(np.abs(c), np.abs(z))).astype(np.float64)


def bound(n):
    return 4.0 * n * U


def completeness(c, z):
    c = np.asarray(c, dtype=np.float64).astype(LD)
    z = np.asarray(z, dtype=np.complex128).astype(CLD)
    with np.errstate(all="ignore"):
        return float(np.abs(np.sum(z) + c[1] / c[0]) / max(LD(1), np.sum(np.abs(z))))


def completeness_tolerance(c):
    c = np.asarray(c, dtype=np.float64)
    return max(100.0 * completeness(c, np.roots(c)), (c.size - 1) * U)


def worst_duplicate(c, z):
    """The smallest completeness() over all ways of replacing ONE root by a copy of its nearest neighbour."""
    c = np.asarray(c, dtype=np.float64).astype(LD)
    z = np.asarray(z, dtype=np.complex128)
    d = np.abs(z[:, None] - z[None, :])
    np.fill_diagonal(d, np.inf)
    nn = z[np.argmin(d, axis=1)].astype(CLD)
    zl = z.astype(CLD)
    s, a = np.sum(zl), np.sum(np.abs(zl))
    res = np.abs(s - zl + nn + c[1] / c[0]) / np.maximum(LD(1), a - np.abs(zl) + np.abs(nn))
    return float(np.min(res))


def match(got, ref):
    """Greedy one-to-one nearest matching (root order is unspecified): the largest distance of a pair."""
    got, ref = np.asarray(got, dtype=np.complex128), np.asarray(ref, dtype=np.complex128)
    assert got.size == ref.size
    free = np.ones(ref.size, dtype=bool)
    worst = 0.0
    for g in got:
        d = np.where(free, np.abs(ref - g), np.inf)
        j = int(np.argmin(d))
        worst = max(worst, float(d[j]))
        free[j] = False
    return worst


def multiple_root_distance(z, root, m):
    """Largest distance to `root` among the m returned roots closest to it."""
    return float(np.sort(np.abs(np.asarray(z, dtype=np.complex128) - root))[:m].max())


# ------------------------------------------------------------------------------------------------------- the generators
def ring_roots(n, seed, rlo=0.9, rhi=0.999, extra=()):
    """AR-like roots: K = (n - len(extra)) // 2 conjugate pairs at angles (k + 0.5) / K * pi with +-0.3 / K * pi jitter and radii
    uniform in [rlo, rhi], a real root 0.5 when an odd number is left, then the `extra` roots as given."""
    rng = np.random.default_rng(seed)
    m = n - len(extra)
    assert m >= 0
    k = m // 2
    ang = (np.arange(k) + 0.5 + rng.uniform(-0.3, 0.3, k)) / max(k, 1) * np.pi
    up = rng.uniform(rlo, rhi, k) * np.exp(1j * ang)
    parts = [up, np.conj(up)] + ([np.array([0.5 + 0j])] if m % 2 else []) + [np.asarray(extra, dtype=np.complex128)]
    return np.concatenate(parts)


def poly_from_roots(roots, seed=0):
    """Real float64 coefficients (descending, monic) of prod (z - r): the factors multiplied in complex long double in a seeded
    random order, the real part rounded to float64."""
    roots = np.asarray(roots, dtype=np.complex128)
    c = np.ones(1, dtype=CLD)
    for r in roots[np.random.default_rng(seed).permutation(roots.size)].astype(CLD):
        c = np.concatenate([c, np.zeros(1, dtype=CLD)])
        c[1:] -= r * c[:-1]
    return c.real.astype(np.float64)


SEED_CANDIDATES = 8


def _candidates(m, seed, rlo, rhi):
    """[(max |c|, seed)] of the candidate seeds of a ring of degree m."""
    seeds = [seed + 1000 * j for j in range(SEED_CANDIDATES)]
    return [(float(np.abs(poly_from_roots(ring_roots(m, s, rlo, rhi), s)).max()), s) for s in seeds]


@functools.lru_cache(maxsize=None)
def _ring_cached(n, seed, rlo, rhi, extra):
    # Jittered rings are well scaled (max |c| is O(1)) up to degree 257; near degree 1000 max |c| ranges from 1 to 1e16 over
    # the seeds, and with it the condition of the sum of the roots: a backward-stable root finder still meets the backward
    # bound on the badly scaled ones (badly_scaled_case holds one to it), but not the completeness tolerance.  Of eight
    # candidate seeds the one whose ring part has the smallest max |c| is taken: a property of the polynomial alone.
    m = n - len(extra)
    best = min(_candidates(m, seed, rlo, rhi))[1] if m > 257 else seed
    r = ring_roots(n, best, rlo, rhi, extra)
    c = poly_from_roots(r, best)
    c.setflags(write=False)
    r.setflags(write=False)
    return c, r


def ring(n, seed, rlo=0.9, rhi=0.999, extra=()):
    """(coefficients, generating roots), both read-only and cached."""
    return _ring_cached(int(n), int(seed), float(rlo), float(rhi), tuple(complex(e) for e in extra))


# ------------------------------------------------------------------------------------- the kernel's trimming, restated
def trim(c, trail_eps=TRAIL_EPS):
    """(core, tz): trailing |c| < trail_eps dropped (one coefficient always stays), leading exact zeros stripped, then tz exact
    trailing zeros taken off (roots at 0, reported after the others); core is what is left, degree core.size - 1.  (None, 0)
    when no root is left."""
    c = np.asarray(c, dtype=np.float64)
    hi = c.size
    while hi > 1 and abs(c[hi - 1]) < trail_eps:
        hi -= 1
    lo = 0
    while lo < hi and c[lo] == 0.0:
        lo += 1
    if hi - lo <= 1:
        return None, 0
    tz = 0
    while hi - 1 - tz > lo and c[hi - 1 - tz] == 0.0:
        tz += 1
    return c[lo : hi - tz], tz


# --------------------------------------------------------------------------------- the kernel's iteration, restated
def aberth(c, safe=True, info=None):
    """Roots (complex128, n) of the trimmed polynomial c (descending, c[0] != 0, c[-1] != 0) by the kernel's iteration: start
    circle of radius |c_n / c_0|^(1/n) clamped to [1e-3, 1e3] at angles 2 pi k / n + 0.4, Jacobi sweeps of the Aberth-Ehrlich
    correction, stop when no correction exceeds 2e-13 of its iterate (1-norms), at most 200 sweeps.  safe: for |z| > 1 the
    Newton ratio comes from the reversed polynomial at y = 1 / z, p / p' = 1 / (y (n - y q'(y) / q(y))), coincident
    iterates are left out of the pair sum, and an iterate whose |p| (1-norm) is within 2 u of sum_k |c_k| |z|^(n-k) stays where
    it is (plain: only when p is exactly 0), which ends the noise-driven sweeps at a multiple root."""
    c = np.asarray(c, dtype=np.float64)
    n = c.size - 1
    a = c / c[0]
    r0 = abs(a[n]) ** (1.0 / n)
    if not r0 > 1e-3:
        r0 = 1e-3
    r0 = min(r0, 1e3)
    z = r0 * np.exp(1j * (2.0 * np.pi * np.arange(n) / n + 0.4))
    rev = a[::-1]
    tau = 2.0 * U
    with np.errstate(all="ignore"):
        for sweep in range(MAX_SWEEPS):
            pv, dv = np.ones(n, complex), np.zeros(n, complex)
            for m in range(1, n + 1):
                dv = dv * z + pv
                pv = pv * z + a[m]
            ratio = pv / dv
            mod = np.abs(z)
            sv = np.ones(n)
            for m in range(1, n + 1):
                sv = sv * mod + abs(a[m])
            zero = (np.abs(pv.real) + np.abs(pv.imag) <= tau * sv) if safe else (pv == 0)
            if safe:
                out = (z.real * z.real + z.imag * z.imag) > 1.0
                if np.any(out):
                    y = 1.0 / z[out]
                    qv, dq = np.full(y.size, rev[0], complex), np.zeros(y.size, complex)
                    for m in range(1, n + 1):
                        dq = dq * y + qv
                        qv = qv * y + rev[m]
                    ratio[out] = 1.0 / (y * (n - y * (dq / qv)))
                    mod, sv = np.abs(y), np.full(y.size, abs(rev[0]))
                    for m in range(1, n + 1):
                        sv = sv * mod + abs(rev[m])
                    zero[out] = np.abs(qv.real) + np.abs(qv.imag) <= tau * sv
            d = z[:, None] - z[None, :]
            d2 = d.real * d.real + d.imag * d.imag
            np.fill_diagonal(d2, np.inf)
            if safe:
                d2[d2 == 0] = np.inf
            s = np.sum(np.conj(d) / d2, axis=1)
            w = np.where(zero, 0.0, ratio / (1.0 - ratio * s))
            changed = np.any(np.abs(w.real) + np.abs(w.imag) > 2e-13 * (np.abs(z.real) + np.abs(z.imag)))
            z = z - w
            if not changed:
                break
    if info is not None:
        info["sweeps"] = sweep + 1
    return z


# -------------------------------------------------------------------------------------------------- the FIR numerator
def fir_numerator(a, x, n_len, divisor, q):
    """(b, s) in long double: b[n] = sum_k a[k] h[n-k] over 0 <= n-k < n_len with h = x / divisor (x float32, exact quotient up
    to 2^-64), n = 0..q, and s[n] = sum_k |a[k] h[n-k]|, the sum the float64 bound (p + 3) u s[n] refers to: p + 1 products
    and sums plus the division of each sample."""
    a = np.asarray(a, dtype=np.float64).astype(LD)
    h = np.asarray(x, dtype=np.float32)[: max(0, min(int(n_len), q + 1))].astype(LD) / LD(float(divisor))
    b, s = np.zeros(q + 1, dtype=LD), np.zeros(q + 1, dtype=LD)
    if h.size:
        full, fabs = np.convolve(a, h), np.convolve(np.abs(a), np.abs(h))
        k = min(q + 1, full.size)
        b[:k], s[:k] = full[:k], fabs[:k]
    return b, s


# ---------------------------------------------------------------------------------------------------- the case lists
# Degrees on both sides of every launch boundary: four lanes per root in 256- (n <= 64), 512- (n <= 128) and 1024-thread
# (n <= 256) workgroups, one lane per root in 512- (n <= 512) and 1024-thread workgroups above.
DEGREES = (1, 2, 3, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024)
MATCH_MAX_DEGREE = 129
# (degree, roots outside the unit circle that replace as many ring roots)
OUTSIDE = ((256, (-20.0,)), (512, (-4.5,)), (128, (-300.0,)), (64, (-6e4,)), (257, (2 + 9j, 2 - 9j)), (1000, (-1.05, 1.02)),
           (1024, (-2.5,)))


def degree_case(n):
    return ring(n, 100 + n)


def outside_case(n, extra):
    return ring(n, 200 + n, extra=extra)


@functools.lru_cache(maxsize=None)
def badly_scaled_case(n=1024):
    """Coefficients of the WORST scaled of the candidate rings of degree n (max |c| around 1e14 at 1024): held to the backward
    bound only, the sum of its roots is too ill conditioned for the completeness tolerance."""
    worst = max(_candidates(n, 100 + n, 0.9, 0.999))[1]
    c = poly_from_roots(ring_roots(n, worst), worst)
    c.setflags(write=False)
    return c


def multiple_cases():
    """[(name, coefficients, multiple root, multiplicity)]"""
    c5 = np.real(np.poly([0.5, 0.5, -0.9, 0.9j, -0.9j]))
    c62, _ = ring(62, 362)
    c64 = np.convolve(c62, np.array([1.0, -1.9, 0.9025]))
    return [("double", np.array([1.0, -2.0, 1.0]), 1.0, 2), ("triple", np.array([1.0, -3.0, 3.0, -1.0]), 1.0, 3),
            ("double_in_5", c5, 0.5, 2), ("ring62_double", c64, 0.95, 2)]


def special_cases():
    """[(name, coefficients)]: z^n - 1 at n = 4 and 64; roots of modulus 1e-3 .. 2e-3 (the start radius is clamped at 1e-3)."""
    out = []
    for n in (4, 64):
        c = np.zeros(n + 1)
        c[0], c[n] = 1.0, -1.0
        out.append((f"unity{n}", c))
    out.append(("small_modulus", ring(32, 432, rlo=1e-3, rhi=2e-3)[0]))
    return out


def all_cases():
    """[(name, coefficients)] of every polynomial the GPU file holds to both bounds."""
    out = [(f"ring{n}", degree_case(n)[0]) for n in DEGREES]
    out += [(f"outside{n}", outside_case(n, e)[0]) for n, e in OUTSIDE]
    return out + special_cases()


# Every trimming rule in one launch: NPOLY rows of NCOEF coefficients that trim to different degrees.
NCOEF = 66
NPOLY = 37
KINDS = ("full65", "tiny_trailing_64", "tiny_trailing_40", "leading_zeros", "trailing_zeros", "all_zero", "constant")
KIND_COUNTS = {"full65": 65, "tiny_trailing_64": 64, "tiny_trailing_40": 40, "leading_zeros": 63, "trailing_zeros": 62,
               "all_zero": 0, "constant": 0}                # roots with the product's trail_eps


def trim_rows():
    rows = np.zeros((NPOLY, NCOEF))
    rng = np.random.default_rng(66)
    for i in range(NPOLY):
        kind = KINDS[i % len(KINDS)]
        if kind == "full65":
            rows[i] = ring(65, 500 + i)[0]
        elif kind == "tiny_trailing_64":
            rows[i, :65] = ring(64, 500 + i)[0]
            rows[i, 65] = 9e-15 * (-1.0) ** i
        elif kind == "tiny_trailing_40":
            rows[i, :41] = ring(40, 500 + i)[0]
            rows[i, 41:] = rng.uniform(-9e-15, 9e-15, NCOEF - 41) * (rng.random(NCOEF - 41) < 0.7)
        elif kind == "leading_zeros":
            rows[i, 2:] = 3.0 * ring(63, 500 + i)[0]
        elif kind == "trailing_zeros":
            rows[i, :63] = -0.5 * ring(62, 500 + i)[0]
        elif kind == "constant":
            rows[i, i % 2] = 3.0
            rows[i, i % 2 + 1] = 5e-15
    return rows
