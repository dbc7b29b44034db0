"""
Restatements for the burst-decay map (ira_burst_table, ira_burst_decay; include/ira.h) on top of tests/fdw_ref.py, and the
bounds the device and a float64 emulation are held to.  Helper module, like fdw_ref.py: it holds no tests.

A cell (channel x, centre p, step delta, point rho / H, window) IS fdw_ref.reference(x, p + delta, rho, H, window): its re0,
im0, a = sum |v| and n.  Bounds (u = 2^-53; fdw_ref.py derives them):
  |S - ref| <= (n + 16) u a                          (a bound of 0 asks for equality)
  |g(k) - long-double g(k)| <= 16 u w(k)             the per-term allowance of that bound, for a table entry
wavelet_reference(rho, H, window): (re, im, w) of g(k), k = -H .. H, long double, formed as fdw_ref.reference forms a term.
wavelet_emulate64(rho, H, window): the same in float64 NumPy the way the kernel forms it (fdw_ref.emulate64's arithmetic).
cell_emulate64(g, x, c, H, order): the table form (w * phasor) * x summed in float64, order "pairwise" (numpy.sum) or
"lanes" (the device's: lane l adds the terms l, l + 64, .. ascending, the 64 lane sums are then added ascending).
"""
import numpy as np

import fdw_ref as R

LD = np.longdouble
U = R.U
LANES = 64                                                     # IRA_BURST_LANES


def wavelet_reference(rho, half, window):
    assert window in R.WINDOWS
    k = np.arange(-int(half), int(half) + 1).astype(LD)
    r_hi = LD(np.float32(rho))
    r_lo = LD(np.float64(rho)) - r_hi
    t = k * r_hi
    ang = LD(2) * R.PI * ((t - np.rint(t)) + k * r_lo)
    if window == "hann":
        w = np.sin(R.PI * (LD(int(half) + 1) - np.abs(k)) / LD(2 * int(half) + 2)) ** 2
    else:
        w = np.ones(k.size, dtype=LD)
    return w * np.cos(ang), -(w * np.sin(ang)), w


def wavelet_emulate64(rho, half, window):
    """(2 H + 1, 2) float64."""
    assert window in R.WINDOWS
    k = np.arange(-int(half), int(half) + 1).astype(np.float64)
    rho = np.float64(rho)
    t_hi = k * rho
    ang = 2.0 * np.pi * ((t_hi - np.rint(t_hi)) + R._two_product_error(k, rho, t_hi))
    if window == "hann":
        w = np.sin(np.pi * ((int(half) + 1 - np.abs(k)) / (2.0 * int(half) + 2.0))) ** 2
    else:
        w = np.ones(k.size)
    return np.stack([w * np.cos(ang), -(w * np.sin(ang))], axis=1)


def table_ratio(table, rho, half, window):
    """The worst |entry - long-double entry| / (16 u w(k)) of one point's (2 H + 1, 2) float64 table."""
    re, im, w = wavelet_reference(rho, half, window)
    g = np.asarray(table, dtype=np.float64).reshape(-1, 2).astype(LD)
    assert g.shape[0] == 2 * int(half) + 1
    return float(np.max(np.hypot(g[:, 0] - re, g[:, 1] - im) / (LD(16) * LD(U) * w)))


def cell_emulate64(g, x, c, half, order):
    """(re, im) float64 of one cell from a float64 table g (2 H + 1, 2) of its point."""
    x = np.asarray(x, dtype=np.float32)
    lo, hi = R._span(x.size, c, half)
    if hi < lo:
        return 0.0, 0.0
    i = np.arange(lo, hi + 1)
    terms = g[i - int(c) + int(half)] * x[i].astype(np.float64)[:, None]
    if order == "pairwise":
        return float(np.sum(terms[:, 0])), float(np.sum(terms[:, 1]))
    assert order == "lanes"
    full = np.zeros((-(-(2 * int(half) + 1) // LANES) * LANES, 2))
    full[i - int(c) + int(half)] = terms
    lanes = np.add.reduce(full.reshape(-1, LANES, 2), axis=0)      # row after row: ascending rounds
    total = np.cumsum(lanes, axis=0)[-1]                            # ascending lanes
    return float(total[0]), float(total[1])


class Cells:
    """fdw_ref.reference per cell, remembered: tests that share channels and deltas compute a cell once."""

    def __init__(self):
        self._seen = {}

    def ref(self, key, x, c, rho, half, window):
        k = (key, int(c), float(rho), int(half), window)
        if k not in self._seen:
            self._seen[k] = R.reference(x, int(c), rho, int(half), window)
        return self._seen[k]


def cell_ratio(re, im, ref):
    """|S - ref| / ((n + 16) u a): 0 where both are 0, inf where an error meets a bound of 0 or S is not finite."""
    if not (np.isfinite(re) and np.isfinite(im)):
        return float("inf")
    err = np.hypot(LD(re) - ref["re0"], LD(im) - ref["im0"])
    bound = LD(ref["n"] + 16) * LD(U) * ref["a"]
    if bound == 0:
        return 0.0 if err == 0 else float("inf")
    return float(err / bound)
