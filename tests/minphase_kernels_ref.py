"""Reference for the five kernels of ira_minphase.hip, one entry point at a time: ira_minphase_logmag (the maximum, then
G and the floored count), ira_minphase_excess, ira_minphase_gather and ira_minphase_spectrum.

tests/minphase_ref.py restates the whole chain and holds it to bounds that the float32 cepstrum dominates (1e-7 rad); here
every kernel stands alone.  Its inputs are float64 arrays this module builds (no transform output), so the reference is a
function of exactly the bits the kernel reads, and the bounds are the kernel's own arithmetic: helper module, no tests.
tests/test_minphase_kernels_ref_cpu.py shows that the case tables, judged by the checkers below, reject the subtly wrong
kernels one could write; tests/test_gpu_minphase_kernels.py launches them.

u = 2^-53.  LIB_ULP (tests/spectrum_ref.py) is what the project assumes of the device library's float64 functions, in
ulp of the result; an ulp of v is numpy.spacing(|v|) <= 2 u |v|.

P, count   exact.  |X|^2 = re * re + im * im rounds one operation at a time (the file is compiled with -ffp-contract=off),
           like NumPy float64; the maximum and the comparison round nothing.  P == numpy.max of the powers to the bit, NaN
           when any power is NaN, +inf when one overflows; count == count_nonzero(power < P * floor_lin) with floor_lin =
           math.pow(10.0, floor_db / 10.0), the C library's pow the host code calls.  Powers are 0 or >= 1e-80 in every
           table, so that P * floor_lin is a normal number at floor_db = -300 and its rounding is the one IEEE product;
           this is all the chain can produce: a float32 segment that is not silence has sum x^2 >= (2^-149)^2 = 2^-298,
           and P >= mean_k |X_k|^2 >= sum x^2 by Parseval.
G          long-double 0.5 ln(max(p, P_floor)) of the float64 p and P_floor.  The maximum and the 0.5 are exact, so the
           error is the library's ln alone: |dG| <= LIB_ULP ulp(G).  Im G is +0.0 to the bit.  An element whose P is 0,
           NaN or inf: all-zero bits, count 0.
excess     the kernel's formula in long double: d = atan2(im, re) + TWO_PI ((k p mod N) / N) - 2 Im T, then
           d - TWO_PI rint(d / TWO_PI), TWO_PI the float64 constant, k p an exact integer.  One rounding per operation:
             atan2                 LIB_ULP ulp of a value <= pi:            2 LIB_ULP u pi
             (k p mod N) / N       exact (N a power of two, k p mod N < 2^21)
             TWO_PI * turn         turn < 1:                                 2 u pi
             atan2 + product       |sum| < 3 pi:                             3 u pi
             2 Im T                exact
             rel - 2 Im T          = d:                                      u |d|
             d / TWO_PI, rint      no error in the result unless the quotient crosses a tie: see below
             TWO_PI * n            |2 pi n| <= |d| + pi:                     u (|d| + pi)
             d - TWO_PI n          |result| <= pi:                           u pi
           bound(d) = u ((2 LIB_ULP + 7) pi + 2 |d|)   (a = 2 LIB_ULP + 7 = 11, b = 2)
           The quotient's own error, u |d| / (2 pi) in units of the quotient, moves the integer only if d lies within
           bound(d) of an odd multiple of PI = TWO_PI / 2: there, and only there, the comparison is modulo TWO_PI.
           Where the inputs make every step before the wrap exact (re > 0, Im X = +0.0, k p mod N == 0: atan2 = +0, turn
           0, d = -2 Im T to the bit) the wrap is four IEEE operations and the device must return numpy float64's bits;
           the planted d = +-pi, 3 pi are of this kind, so the tie (rint to even: wrap(pi) = +pi, wrap(-pi) = -pi) is held
           exactly and not excused.
           Im X is read as it stands, its sign bit included, at k = 0 and N/2 as well: (-1, +0.0) is +pi, (-1, -0.0) is
           -pi.  The chain relies on its transforms leaving +0.0 in Im X_0 (a -0.0 under a negative X_0 would turn the
           whole unwrapped curve by 360 degrees); tests/test_gpu_minphase.py::test_polarity_and_a_negative_sample_sum
           pins that on every path the first transform takes, and found +0.0 on all of them.
gather     bits: Re X, Im X, Im T[k-1], Im T[k], Im T[k+1], u[k-1], u[k], u[k+1] at k clamped to 1 .. N/2 - 1; an invalid
           element all NaN.
spectrum   long-double exp(G) (cos 2t, sin 2t), t = Im T (2 t exact), normwise per bin: exp is LIB_ULP ulp of the
           magnitude (2 LIB_ULP u relative), sincos LIB_ULP ulp of each component (2 LIB_ULP u of the unit vector,
           normwise), each product one rounding (u of its component, u normwise): |dM| <= (4 LIB_ULP + 1) u |M| (+ second
           order, allowed as 2^-40 of it).  Im M is +0.0 to the bit at k = 0 and N/2 and the real part is held alone
           there; an invalid element is all-zero bits.

The library's own figures: where the rest of a formula is exact the device's error IS the library function's, and the
checkers return it in ulp: ln from G (always), atan2 from the excess bins with Im T == 0 and k p mod N == 0 (d = atan2, the
wrap subtracts 0), exp from the spectrum bins with cos 2t == 1 (t == 0), sincos from the bins with G == 0 (e^G = 1).
"""
import functools
import math

import numpy as np

from deconv_ref import LD, LONGDOUBLE_OK, need_longdouble  # noqa: F401  (the GPU and CPU tests take them from here)
from spectrum_ref import LIB_ULP

U = 2.0 ** -53
TWO_PI = 6.283185307179586                # the kernels' MP_TWO_PI
PI = TWO_PI / 2.0
FIELDS = 8
MAX_N = 1 << 21
FLOORS_DB = (-120.0, -60.0, 0.0, -300.0)
NPTS = (1, 255, 256, 257, 479, 4096)
ABI_BINS = (0, -5, None, 1 << 30)          # None: N/2 of the element; refused by the engine wrapper, clamped by the kernel
SPEC_C = 4.0 * LIB_ULP + 1.0
EXCESS_A, EXCESS_B = 2.0 * LIB_ULP + 7.0, 2.0


def floor_lin(floor_db):
    return math.pow(10.0, float(floor_db) / 10.0)


def power(X):
    X = np.asarray(X, np.complex128)
    with np.errstate(all="ignore"):
        return X.real * X.real + X.imag * X.imag


def pmax(X):
    """P as the device forms it: the maximum of the float64 powers, NaN if any is NaN."""
    p = power(X)
    return float("nan") if np.isnan(p).any() else float(np.max(p))


def valid(P):
    return bool(P > 0.0 and P < math.inf)


def words(a):
    return np.ascontiguousarray(a).view(np.uint64)


def ulps(err, ref):
    """err in ulp of the float64 nearest ref."""
    return np.asarray(err, LD) / np.spacing(np.abs(np.asarray(ref, LD).astype(np.float64))).astype(LD)


# -------------------------------------------------------------------------------------------------------------- logmag
def logmag(X, floor_db):
    """(G long double, P, count) of one element."""
    p, P = power(X), pmax(X)
    if not valid(P):
        return np.zeros(p.size, LD), P, 0
    p_floor = P * floor_lin(floor_db)
    return LD(0.5) * np.log(np.maximum(p, p_floor).astype(LD)), P, int(np.count_nonzero(p < p_floor))


def check_logmag(g, p_got, count_got, X, floor_db, what=""):
    """g complex128 (nbins), p_got float64, count_got int64 of one element.  Returns (worst |dG| / bound, worst ln error in ulp)."""
    ref, P, count = logmag(X, floor_db)
    g = np.asarray(g)
    assert g.dtype == np.complex128 and g.shape == ref.shape, (what, g.dtype, g.shape)
    if math.isnan(P):
        assert math.isnan(float(p_got)), f"{what}: P = {p_got!r}, a bin's power is NaN"
    else:
        assert words(np.float64(p_got))[()] == words(np.float64(P))[()], f"{what}: P = {float(p_got)!r}, numpy.max gives {P!r}"
    assert int(count_got) == count, f"{what}: {int(count_got)} bins below the floor, {count} by the float64 comparison"
    assert not words(g.imag.copy()).any(), f"{what}: Im G is not +0.0 at every bin"
    if not valid(P):
        assert not words(g.real.copy()).any(), f"{what}: an element without values has a G that is not all-zero bits"
        return 0.0, 0.0
    assert np.isfinite(g.real).all(), f"{what}: G is not finite"
    err = np.abs(g.real.astype(LD) - ref)
    bound = LIB_ULP * np.spacing(np.abs(ref.astype(np.float64))).astype(LD)
    ratio = float(np.max(err / bound))
    k = int(np.argmax(err / bound))
    assert ratio <= 1.0, f"{what}: |dG| = {ratio:.3g} of {LIB_ULP} ulp at bin {k}: {g.real[k]!r} against {float(ref[k])!r}"
    return ratio, float(np.max(ulps(err, ref)))


# -------------------------------------------------------------------------------------------------------------- excess
def wrap64(d):
    d = np.asarray(d, np.float64)
    return d - TWO_PI * np.rint(d / TWO_PI)


def excess(X, T, p, n):
    """(wrapped excess long double, d long double) of one element with values."""
    X, T = np.asarray(X, np.complex128), np.asarray(T, np.complex128)
    k = np.arange(n // 2 + 1, dtype=np.int64)
    p = min(max(int(p), 0), 0x7fffffff)
    assert n <= MAX_N                                                    # k p < 2^51: the product is exact in int64
    turn = ((k * p) % n).astype(LD) / LD(n)
    d = np.arctan2(X.imag.astype(LD), X.real.astype(LD)) + LD(TWO_PI) * turn - LD(2.0) * T.imag.astype(LD)
    return d - LD(TWO_PI) * np.rint(d / LD(TWO_PI)), d


def exact_bins(X, p, n):
    """Bins whose d is -2 Im T to the bit: atan2 = +0 and no turn."""
    X = np.asarray(X, np.complex128)
    k = np.arange(n // 2 + 1, dtype=np.int64)
    return (X.real > 0) & (X.imag == 0) & ~np.signbit(X.imag) & ((k * (int(p) % n)) % n == 0)


def check_excess(got, X, T, p, n, is_valid, what=""):
    """got float64 (nbins).  Returns (worst error / bound, bins compared modulo 2 pi, worst atan2 error in ulp or 0)."""
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == (n // 2 + 1,), (what, got.dtype, got.shape)
    if not is_valid:
        assert not words(got).any(), f"{what}: an element without values has an excess phase that is not all-zero bits"
        return 0.0, 0, 0.0
    assert np.isfinite(got).all(), f"{what}: the excess phase is not finite"
    ref, d = excess(X, T, p, n)
    bound = LD(U) * (LD(EXCESS_A * np.pi) + LD(EXCESS_B) * np.abs(d)) * (LD(1.0) + LD(2.0) ** -40)
    near = LD(PI) - np.abs(ref) <= bound                                 # d within the bound of an odd multiple of PI
    err = got.astype(LD) - ref
    err = np.where(near, err - LD(TWO_PI) * np.rint(err / LD(TWO_PI)), err)
    ratio = np.abs(err) / bound
    j = int(np.argmax(ratio))
    assert ratio[j] <= 1.0, (f"{what}: excess phase off by {float(ratio[j]):.3g} of its bound at bin {j}: {got[j]!r} against "
                             f"{float(ref[j])!r} (d = {float(d[j])!r}, X = {X[j]!r}, Im T = {T[j].imag!r})")
    ex = exact_bins(X, p, n)
    want = wrap64(-2.0 * np.asarray(T).imag[ex])
    bad = words(got[ex]) != words(want)
    assert not bad.any(), (f"{what}: the wrap of an exact d differs from the IEEE arithmetic at bin "
                           f"{int(np.nonzero(ex)[0][np.argmax(bad)])}: {got[ex][bad][0]!r} against {want[bad][0]!r}")
    k = np.arange(n // 2 + 1, dtype=np.int64)
    pure = ((k * (int(p) % n)) % n == 0) & (np.asarray(T).imag == 0) & ~near & (ref != 0)
    lib = float(np.max(ulps(np.abs(err[pure]), ref[pure]))) if pure.any() else 0.0
    return float(ratio[j]), int(np.count_nonzero(near)), lib


# -------------------------------------------------------------------------------------------------------------- gather
def gather(X, T, u, bins, n, is_valid):
    """(J, FIELDS) float64 of one element."""
    k = np.clip(np.asarray(bins, np.int64), 1, n // 2 - 1)
    if not is_valid:
        return np.full((k.size, FIELDS), np.nan)
    X, T, u = np.asarray(X, np.complex128), np.asarray(T, np.complex128), np.asarray(u, np.float64)
    return np.stack([X.real[k], X.imag[k], T.imag[k - 1], T.imag[k], T.imag[k + 1], u[k - 1], u[k], u[k + 1]], axis=1)


def check_gather(got, X, T, u, bins, n, is_valid, what=""):
    got = np.asarray(got)
    ref = gather(X, T, u, bins, n, is_valid)
    assert got.dtype == np.float64 and got.shape == ref.shape, (what, got.dtype, got.shape)
    if not is_valid:
        assert np.isnan(got).all(), f"{what}: a record of an element without values holds a number"
        return
    bad = words(got) != words(ref)
    j, f = np.unravel_index(int(np.argmax(bad)), bad.shape)
    assert not bad.any(), (f"{what}: {int(bad.sum())} fields differ, first at point {j} (bin {int(np.asarray(bins)[j])}) "
                           f"field {f}: {got[j, f]!r} against {ref[j, f]!r}")


# ------------------------------------------------------------------------------------------------------------ spectrum
def spectrum(G, T):
    """(Re M, Im M) long double of one element with values; Im M = 0 at the two edge bins."""
    g, t2 = np.asarray(G, np.complex128).real.astype(LD), LD(2.0) * np.asarray(T, np.complex128).imag.astype(LD)
    mag = np.exp(g)
    re, im = mag * np.cos(t2), mag * np.sin(t2)
    im[0] = im[-1] = LD(0.0)
    return re, im, mag


def check_spectrum(got, G, T, is_valid, what=""):
    """got complex128 (nbins).  Returns (worst |dM| / bound, worst exp error in ulp, worst sin / cos error in ulp)."""
    got = np.asarray(got)
    assert got.dtype == np.complex128 and got.shape == np.asarray(G).shape, (what, got.dtype, got.shape)
    if not is_valid:
        assert not words(got).any(), f"{what}: an element without values has an M that is not all-zero bits"
        return 0.0, 0.0, 0.0
    re, im, mag = spectrum(G, T)
    gi = got.imag.copy()
    assert not words(gi[[0, -1]]).any(), f"{what}: Im M is not +0.0 at k = 0 and N/2: {gi[0]!r}, {gi[-1]!r}"
    assert np.isfinite(got.real).all() and np.isfinite(gi).all(), f"{what}: M is not finite"
    err = np.hypot(got.real.astype(LD) - re, gi.astype(LD) - im)
    bound = LD(SPEC_C * U) * mag * (LD(1.0) + LD(2.0) ** -40)
    ratio = err / bound
    j = int(np.argmax(ratio))
    assert ratio[j] <= 1.0, (f"{what}: |dM| = {float(ratio[j]) * SPEC_C:.3g} u |M| at bin {j} ({SPEC_C} allowed): {got[j]!r} "
                             f"against ({float(re[j])!r}, {float(im[j])!r}), G = {np.asarray(G)[j].real!r}, Im T = {np.asarray(T)[j].imag!r}")
    t, g = np.asarray(T).imag, np.asarray(G).real
    lib_exp = float(np.max(ulps(np.abs(got.real[t == 0].astype(LD) - re[t == 0]), re[t == 0]))) if (t == 0).any() else 0.0
    one = (g == 0) & (t != 0)
    one[0] = one[-1] = False
    lib_sc = 0.0
    if one.any():
        lib_sc = float(max(np.max(ulps(np.abs(got.real[one].astype(LD) - re[one]), re[one])),
                           np.max(ulps(np.abs(gi[one].astype(LD) - im[one]), im[one]))))
    return float(ratio[j]), lib_exp, lib_sc


# ----------------------------------------------------------------------------------------------------------- the tables
def plant(target):
    """(re, im) float64 with re * re + im * im == target to the bit."""
    target = float(target)
    re = math.sqrt(target)
    for _ in range(256):
        rem = target - re * re
        if rem >= 0.0:
            im = math.sqrt(rem)
            for cand in (0.0, im, np.nextafter(im, 0.0), np.nextafter(im, np.inf)):
                if re * re + cand * cand == target:
                    return re, float(cand)
        re = float(np.nextafter(re, 0.0))
    raise AssertionError(f"no float64 pair has the power {target!r}")


def steps(v, n):
    """v moved n float64 steps (up for n > 0)."""
    v = np.float64(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, np.inf if n > 0 else 0.0)
    return float(v)


P_PLANTED = 4.0
PLANT_STEPS = (-3, -1, 0, 1, 3)
#          name              N      centre p      what it holds
ELEMENTS = (("max_at_0", 32, 0, "largest power at bin 0; exact-d bins (d = +-pi, 3 pi ..), X_0 = (-9, -0.0)"),
            ("max_at_nyquist", 64, 1, "largest power at bin N/2 = 32, (-8, -0.0); (-1, +0), (+0, +0), (-0, -0) at 0, 3, 5"),
            ("equal_maxima", 512, 511, "bins 7 and 100 share the largest power; (-1, -0.0) at 0, (-1, +0.0) at N/2"),
            ("max_in_last_group", 4096, 4096, "largest power at bin 1500 (second workgroup); p = N; Im T = 0 on 1024 .. 2047"),
            ("nine_groups", 32768, (1 << 31) - 1, "largest power at bin 8965 (ninth workgroup); p = 2^31 - 1"),
            ("zeros", 64, 5, "X = 0"),
            ("nan_bin", 512, 3, "Re X = NaN at bin 200"),
            ("inf_bin", 4096, 9, "Im X = inf at bin 700 (second workgroup)"),
            ("overflow", 32, 2, "(1e160, 1e160) at bin 4: the power overflows from finite parts"),
            ("planted", 4096, 12345, "P = 4; bins a few float64 steps either side of P_floor at every floor, one step "
                                     "below P, zeros; G = 0 on 256 .. 511"))
MAIN_MAX_NFFT, SPARSE_MAX_NFFT = 32768, 131072
BIG = ("big", MAX_N, (1 << 31) - 1, "k p reaches 2^51; the excess kernel only")


def _element(name, n, p, rng):
    nb = n // 2 + 1
    X = (rng.standard_normal(nb) + 1j * rng.standard_normal(nb)) * rng.uniform(1e-3, 1.0, nb)
    T = rng.uniform(-50.0, 50.0, nb) * 1j + rng.standard_normal(nb)
    G = rng.uniform(-30.0, 10.0, nb) + 0j
    u = rng.uniform(-400.0, 400.0, nb)
    mz = complex(-0.0, -0.0)
    if name == "max_at_0":
        X[0] = complex(-9.0, -0.0)
        X[1:9] = 1.5 + 0j
        three_pi = 3.0 * PI
        T.imag[1:9] = [-PI / 2, PI / 2, -three_pi / 2, three_pi / 2, -5.0 * PI / 2, 0.0, -1e-300, 7.0 * PI / 2]
    elif name == "max_at_nyquist":
        X[0], X[3], X[5], X[32] = complex(-1.0, 0.0), 0j, mz, complex(-8.0, -0.0)
    elif name == "equal_maxima":
        X[7], X[100] = 6.0 - 2.5j, -2.5 + 6.0j
        X[0], X[256] = complex(-1.0, -0.0), complex(-1.0, 0.0)
    elif name == "max_in_last_group":
        X[1500] = -5.0 + 7.0j
        X[0], X[2048], X[9] = 0j, mz, complex(-1.0, -0.0)
        T.imag[1024:2048] = 0.0
        X[20:30] = 0.75 + 0j                                              # exact d at p = N: the wrap of several turns, to the bit
    elif name == "nine_groups":
        X[8 * 256 + 5 + 3 * 9 * 256] = 4.0 + 4.0j
        X[0], X[16384] = complex(-1.0, 0.0), complex(-1.0, -0.0)
    elif name == "zeros":
        X[:] = 0.0
    elif name == "nan_bin":
        X[200] = complex(np.nan, 1.0)
    elif name == "inf_bin":
        X[700] = complex(1.0, np.inf)
    elif name == "overflow":
        X[4] = complex(1e160, 1e160)
    elif name == "planted":
        X *= 0.5
        X[11] = 2.0 + 0j
        j = 40
        for db in FLOORS_DB:
            for s in PLANT_STEPS:
                if db == 0.0 and s > 0:
                    continue                                             # nothing lies above P
                X[j] = complex(*plant(steps(P_PLANTED * floor_lin(db), s)))
                j += 1
        X[j:j + 3] = 0.0
        X[2048] = complex(*plant(steps(P_PLANTED, -1)))
        G[256:512] = 0.0
    if name in ("planted", "max_in_last_group"):
        T.imag[600:700] = 0.0                                            # cos 2t = 1: M = e^G, the library's exp alone
    pw = power(X)
    assert np.all((pw == 0) | (pw >= 1e-80) | ~np.isfinite(pw)), name
    for a in (X, T, G, u):
        a.setflags(write=False)
    return dict(name=name, n=n, p=p, X=X, T=T, G=G, u=u, P=pmax(X), valid=valid(pmax(X)))


@functools.lru_cache(maxsize=None)
def elements():
    """The ragged launch at max_nfft = 32768: one dict(name, n, p, X, T, G, u, P, valid) per row of ELEMENTS."""
    rng = np.random.default_rng(2031)
    return tuple(_element(name, n, p, rng) for name, n, p, _ in ELEMENTS)


@functools.lru_cache(maxsize=None)
def sparse_elements():
    """The elements of at most 4096 points, launched at max_nfft = 131072: most workgroups own no bin."""
    return tuple(e for e in elements() if e["n"] <= 4096)


@functools.lru_cache(maxsize=None)
def big_element():
    """N = 2^21, p = 2^31 - 1: X and T only."""
    rng = np.random.default_rng(2032)
    name, n, p, _ = BIG
    nb = n // 2 + 1
    X = rng.standard_normal(nb) + 1j * rng.standard_normal(nb)
    T = rng.uniform(-50.0, 50.0, nb) * 1j
    X.setflags(write=False), T.setflags(write=False)
    return dict(name=name, n=n, p=p, X=X, T=T, P=pmax(X), valid=True)


@functools.lru_cache(maxsize=None)
def gather_bins(npts, abi=False):
    """(len(elements()), npts) int32: every element's bins 1 (first) and N/2 - 1 (last) around random ones; with abi the four of ABI_BINS
    that only the C-ABI takes (npts >= 6)."""
    rng = np.random.default_rng(2033 + npts)
    rows = []
    for i, e in enumerate(elements()):
        half = e["n"] // 2
        b = rng.integers(1, half, npts).astype(np.int64)
        b[0] = 1
        if npts > 1 or i % 2:                                            # a single point: bin 1 and bin N/2 - 1 in turn
            b[-1] = half - 1
        if abi:
            b[1:5] = [half if v is None else v for v in ABI_BINS]
        rows.append(b)
    out = np.stack(rows).astype(np.int32)
    out.setflags(write=False)
    return out
