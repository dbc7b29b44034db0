"""
A long-double NumPy restatement of the frequency-dependent-window sums (ira_fdw_response, include/ira.h) and the error
bounds the device and a float64 emulation are held to.  Helper module, like reflections_ref.py: it holds no tests.

reference(x, p, rho, H, window): the six fields and A1 = sum |k v| of ONE (channel, point), in long double:
  terms k = -H .. H with i = p + k inside [0, len(x)), ascending;  w(k) = 0.5 + 0.5 cos(pi k / (H + 1)) or 1, evaluated as
  the identical sin(pi (H + 1 - |k|) / (2 H + 2))^2: at the window's ends, where w is about (pi / (2 H + 2))^2, the literal
  form cancels and keeps an ABSOLUTE error of the format's rounding unit -- a relative error of (H + 1)^2 units, in long
  double as in float64 -- which a clipped window of a few end terms would show (literal_hann states that form);
  the turn count k * rho from the same float64 rho, formed exactly: rho = hi + lo with hi = float32(rho), so that k hi
  and k lo (|k| <= 2^20) are exact in a 64-bit significand, k hi is reduced by its nearest whole number exactly, and the
  two parts are added with one rounding of 2^-65 turns;  pi to long-double precision;  plain ascending sums (cumsum).

Bounds (u = 2^-53; derived, not tuned): a sum of N float64 terms in ANY order carries at most N u of the absolute sum
(first order), and a term -- weight, phasor and the two products -- carries under 8 u of its magnitude, doubled here:
  |S0 - ref| <= (N + 16) u A        |S1 - ref| <= (N + 16) u A1        |A - ref| <= (N + 4) u A        N exact
with A = sum |v| and A1 = sum |k v| of the reference.  A bound of 0 (nothing inside, or silence) asks for equality.

emulate64(x, p, rho, H, window): the same sums in float64 NumPy the way the kernel forms them (t_hi = k rho rounded, its
error by an exact product split, r = (t_hi - rint(t_hi)) + t_lo; hann as sin(pi (H + 1 - |k|) / (2 H + 2))^2), summed
pairwise by numpy.sum: it shows the bounds are float64 arithmetic's own, whatever the order of the sums.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the restatement needs an extended long double"
PI = LD("3.14159265358979323846264338327950288")
U = 2.0 ** -53
WINDOWS = ("hann", "rect")


def _span(n, p, half):
    lo, hi = max(int(p) - int(half), 0), min(int(p) + int(half), int(n) - 1)
    return (lo, hi) if hi >= lo else (0, -1)


def reference(x, p, rho, half, window):
    """dict(re0, im0, re1, im1, a, n, a1), long double (n an int), of one channel x (float32) centred at p."""
    assert window in WINDOWS
    x = np.asarray(x, dtype=np.float32)
    lo, hi = _span(x.size, p, half)
    zero = LD(0)
    if hi < lo:
        return dict(re0=zero, im0=zero, re1=zero, im1=zero, a=zero, n=0, a1=zero)
    i = np.arange(lo, hi + 1, dtype=np.int64)
    k = (i - int(p)).astype(LD)
    r_hi = LD(np.float32(rho))
    r_lo = LD(np.float64(rho)) - r_hi
    t = k * r_hi
    turn = (t - np.rint(t)) + k * r_lo
    ang = LD(2) * PI * turn
    if window == "hann":
        w = np.sin(PI * (LD(int(half) + 1) - np.abs(k)) / LD(2 * int(half) + 2)) ** 2
    else:
        w = np.ones(k.size, dtype=LD)
    v = w * x[i].astype(LD)
    c, s = np.cos(ang), np.sin(ang)

    def total(terms):
        return np.cumsum(terms)[-1]

    return dict(re0=total(v * c), im0=total(-(v * s)), re1=total(k * v * c), im1=total(-(k * v * s)),
                a=total(np.abs(v)), n=int(i.size), a1=total(np.abs(k * v)))


def literal_hann(k, half, dtype=LD):
    """0.5 + 0.5 cos(pi k / (H + 1)) as written, in dtype: what reference() does NOT use (see above)."""
    k = np.asarray(k).astype(dtype)
    return dtype(0.5) + dtype(0.5) * np.cos(PI.astype(dtype) * k / dtype(int(half) + 1))


def _two_product_error(k, rho, t_hi):
    """fma(k, rho, -t_hi) for whole k, |k| <= 2^26, in float64: rho is split into two 26-bit halves whose products with k
    are exact."""
    c = 134217729.0 * rho                                    # 2^27 + 1 (Veltkamp)
    r_hi = c - (c - rho)
    r_lo = rho - r_hi
    return (k * r_hi - t_hi) + k * r_lo


def emulate64(x, p, rho, half, window):
    """(6,) float64: the fields as float64 NumPy forms them, the kernel's arithmetic with numpy.sum's order."""
    assert window in WINDOWS
    x = np.asarray(x, dtype=np.float32)
    lo, hi = _span(x.size, p, half)
    if hi < lo:
        return np.zeros(6)
    i = np.arange(lo, hi + 1, dtype=np.int64)
    k = (i - int(p)).astype(np.float64)
    rho = np.float64(rho)
    t_hi = k * rho
    turn = (t_hi - np.rint(t_hi)) + _two_product_error(k, rho, t_hi)
    ang = 2.0 * np.pi * turn
    if window == "hann":
        w = np.sin(np.pi * ((int(half) + 1 - np.abs(k)) / (2.0 * int(half) + 2.0))) ** 2
    else:
        w = np.ones(k.size)
    v = w * x[i].astype(np.float64)
    c, s = np.cos(ang), np.sin(ang)
    return np.array([np.sum(v * c), np.sum(-(v * s)), np.sum(k * v * c), np.sum(-(k * v * s)), np.sum(np.abs(v)),
                     float(i.size)])


def bounds(ref):
    """(bound of |S0 - ref|, of |S1 - ref|, of |A - ref|) as long doubles."""
    n = ref["n"]
    return (LD(n + 16) * LD(U) * ref["a"], LD(n + 16) * LD(U) * ref["a1"], LD(n + 4) * LD(U) * ref["a"])


def errors(fields, ref):
    """(|S0 - ref|, |S1 - ref|, |A - ref|) of six float64 fields, long double."""
    f = np.asarray(fields, dtype=np.float64).astype(LD)
    return (np.hypot(f[0] - ref["re0"], f[1] - ref["im0"]), np.hypot(f[2] - ref["re1"], f[3] - ref["im1"]),
            np.abs(f[4] - ref["a"]))


def worst_ratio(fields, ref):
    """The largest error / bound of the three sums (0 where both are 0, inf where an error meets a bound of 0); N must be
    exact and the sums finite, or inf."""
    f = np.asarray(fields, dtype=np.float64)
    if not np.all(np.isfinite(f)) or f[5] != ref["n"]:
        return float("inf")
    worst = 0.0
    for e, b in zip(errors(f, ref), bounds(ref)):
        if b == 0:
            worst = max(worst, 0.0 if e == 0 else float("inf"))
        else:
            worst = max(worst, float(e / b))
    return worst
