"""Reference for the kernels of ira_modal.hip: ira_waterfall_rel and both layouts of ira_logbin_aggregate.

Plain NumPy restatements of the two formulas (reference analyse/waterfall.py:308-341 and analyse/modalcloud.py:176-207),
written from the formulas and sharing no code with the kernels or the engine; the case tables the GPU tests launch; and
the comparison functions those tests use.  tests/test_modal_ref_cpu.py ties the restatements to the oracle and shows, on a
machine without a GPU, that every case table rejects the subtly wrong kernels one could write (wrong row, wrong
maximum, wrong divisor, lost NaN).

waterfall_rel is EXACT: a maximum (comparisons), one float32 subtraction and two float32 comparisons per value, so the
device must return its bits.  logbin is a long-double chain (10^(dB/20), ascending sum, division, clamp, 20 log10); the
device does the same chain in float64 and rounds once to float32, so it may differ from the long-double value by half a
float32 ulp plus logbin_bound_db(count).
"""
import functools
import math

import numpy as np

LD = np.longdouble
LONGDOUBLE_OK = np.finfo(LD).nmant >= 63


def need_longdouble():
    import pytest
    if not LONGDOUBLE_OK:
        pytest.skip("np.longdouble has no 64-bit mantissa on this machine: no reference more precise than float64")


# ----------------------------------------------------------------------------------------------------------- waterfall
def waterfall_rel(mag, k_lo, nsel, slice_max, dyn):
    """mag: float32 (F, S).  Rows k_lo .. k_lo+nsel-1, minus their maximum (np.max keeps a NaN) over the whole selection or
    per slice, float32 subtraction, clipped to [-float32(dyn), 0] with NaN kept.  (S, nsel) float32."""
    m = np.asarray(mag)
    assert m.dtype == np.float32 and m.ndim == 2 and 0 <= k_lo and k_lo + nsel <= m.shape[0] and nsel >= 1
    sel = m[k_lo:k_lo + nsel, :]
    with np.errstate(invalid="ignore"):
        ref = np.max(sel, axis=0, keepdims=True) if slice_max else np.max(sel)
        rel = sel - ref
        assert rel.dtype == np.float32
        out = np.minimum(np.maximum(rel, np.float32(-np.float32(dyn))), np.float32(0.0))       # both keep a NaN
    return np.ascontiguousarray(out.T)


def check_waterfall(got, ref, what=""):
    """Exact: the same NaN cells and the same values everywhere else."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float32, (what, got.shape, ref.shape, got.dtype)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: NaN cells differ ({int(gn.sum())} against {int(rn.sum())} of the reference)"
    bad = ~rn & (got != ref)
    assert not bad.any(), (f"{what}: {int(bad.sum())} values differ, first at {tuple(np.argwhere(bad)[0])}: "
                           f"{got[bad][0]!r} against {ref[bad][0]!r}")


WF_SLICES = (1, 2, 3, 40, 63, 64, 65, 130, 257)       # below, at and above the 64-slice tile; counts that do not divide 256
WF_SELECTIONS = ((0, 1), (3, 5), (0, 257), (3, 1000))      # (k_lo, nsel)
WF_DYN = (60.0, 10.0, 0.5, 60.1)
WF_SPARE = 3                                          # rows above the selection (k_lo rows lie below it)


@functools.lru_cache(maxsize=None)
def waterfall_case(k_lo, nsel, slice_max, dyn):
    """One ragged launch: a float32 (k_lo + nsel + WF_SPARE, S) matrix per S of WF_SLICES, random dB in [-120, -6] with

    * the maximum of the selection (-3 dB) in its first row and slice (elements 0, 3, 6), in its last row and slice
      (1, 4, 7) or in both, tied (2, 5, 8); per slice a maximum of -4 .. -8 dB in the first row (even slices) or the last
      (odd slices), in both for every third slice;
    * in up to three slices of an element whose reference level is finite, the values exactly float32(dyn) below that
      level and one float32 step either side of it (selections of at least five rows);
    * a slice that is all -inf (elements 2, 7, 8), a NaN in one slice (3, 7), a +inf (4);
    * in the rows outside the selection values of +10 .. +50 dB and NaNs, which must change nothing.
    """
    rng = np.random.default_rng([11, k_lo, nsel, int(bool(slice_max)), int(round(dyn * 10))])
    d32 = np.float32(dyn)
    mats = []
    for e, S in enumerate(WF_SLICES):
        F = k_lo + nsel + WF_SPARE
        m = rng.uniform(-120.0, -6.0, (F, S)).astype(np.float32)
        sel = m[k_lo:k_lo + nsel]                     # a view
        for s in range(S):
            top = np.float32(-4.0 - (s % 5))
            if s % 3 == 0:
                sel[0, s] = sel[-1, s] = top
            else:
                sel[0 if s % 2 == 0 else -1, s] = top
        if e % 3 in (0, 2):
            sel[0, 0] = np.float32(-3.0)
        if e % 3 in (1, 2):
            sel[-1, -1] = np.float32(-3.0)
        if e in (2, 7, 8):
            sel[:, {2: 1, 7: 64, 8: 256}[e]] = -np.inf
        if e in (3, 7):
            sel[nsel // 2 if e == 3 else 0, 7 if e == 3 else 129] = np.nan
        if e == 4:
            sel[-1, 5] = np.inf
        if nsel >= 5:
            for s in sorted({0, S // 2, S - 1}):
                with np.errstate(invalid="ignore"):
                    level = np.max(sel[:, s]) if slice_max else np.max(sel)
                if not np.isfinite(level) or not np.all(np.isfinite(sel[1:4, s])):
                    continue
                t = np.float32(level - d32)
                sel[1, s], sel[2, s], sel[3, s] = t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))
        out = np.ones(F, bool)
        out[k_lo:k_lo + nsel] = False
        m[out] = rng.uniform(10.0, 50.0, (int(out.sum()), S)).astype(np.float32)
        m[k_lo + nsel, S - 1] = np.nan
        if k_lo > 0:
            m[k_lo - 1, 0] = np.nan
        m.setflags(write=False)
        mats.append(m)
    return tuple(mats)


def waterfall_cases():
    return [(k_lo, nsel, sm, dyn) for (k_lo, nsel) in WF_SELECTIONS for sm in (False, True) for dyn in WF_DYN]


# ------------------------------------------------------------------------------------------------------------- log bins
def logbin(mag, k_base, first, count, frame_major=False):
    """mag: float32 (F, T), or (T, F) when frame_major.  Bin b: rows k_base + first[b] .. + count[b] - 1 as linear magnitude
    10 ** (dB / 20), summed in ascending row order, divided by count[b], max(., 1e-30) with NaN kept (np.maximum),
    20 log10; everything in np.longdouble.  An empty bin is NaN.  Returns (long-double values, their float32 rounding),
    both (nbins, T)."""
    m = np.asarray(mag)
    assert m.dtype == np.float32 and m.ndim == 2
    if frame_major:
        m = m.T
    first, count = np.asarray(first, np.int64), np.asarray(count, np.int64)
    out = np.full((first.size, m.shape[1]), np.nan, dtype=LD)
    with np.errstate(all="ignore"):
        for b in range(first.size):
            c = int(count[b])
            if c <= 0:
                continue
            r0 = k_base + int(first[b])
            assert 0 <= r0 and r0 + c <= m.shape[0]
            lin = LD(10.0) ** (m[r0:r0 + c].astype(LD) / LD(20.0))
            acc = lin[0].copy()
            for k in range(1, c):
                acc = acc + lin[k]
            out[b] = LD(20.0) * np.log10(np.maximum(acc / LD(c), LD(1e-30)))
        return out, out.astype(np.float32)


def logbin_bound_db(count):
    """What the device's float64 chain may be off by, in dB, before its one rounding to float32:
    20 / ln 10 * (count + A) * 2^-53 -- count - 1 additions and one division at half an ulp each (rounded up to one), and
    A = 9 for exp10 and log10.  A is an ALLOWANCE, not a measurement: the ROCm device library's table of ulp figures for
    the double-precision exp10 and log10 is not among the documents this project can read, so each is allowed 4 ulp,
    plus one for the division.  The relative error of the mean turns into dB through d(20 log10 m) = 20 / ln 10 * dm / m."""
    return 20.0 / math.log(10.0) * (np.asarray(count, np.float64) + 9.0) * 2.0 ** -53


def ulp32(x):
    """The float32 spacing of the binade that holds |x| (x long double or float64); the smallest subnormal for 0."""
    _, e = np.frexp(np.abs(np.asarray(x, LD)))
    return np.ldexp(LD(1.0), np.maximum(e.astype(np.int64) - 24, -149).astype(np.int32))


def check_logbin(got, ref_ld, count, what=""):
    """|got - ref| <= ulp32(ref) / 2 + logbin_bound_db(count) on every finite value, the same NaN cells, the same
    infinities.  Returns the largest error / bound."""
    got, ref_ld = np.asarray(got), np.asarray(ref_ld)
    assert got.shape == ref_ld.shape and got.dtype == np.float32, (what, got.shape, ref_ld.shape, got.dtype)
    gn, rn = np.isnan(got), np.isnan(ref_ld)
    assert np.array_equal(gn, rn), (f"{what}: NaN cells differ: got only {np.argwhere(gn & ~rn)[:4].tolist()}, "
                                    f"reference only {np.argwhere(rn & ~gn)[:4].tolist()} (bin, frame)")
    inf = np.isinf(ref_ld)
    assert np.array_equal(got[inf].astype(LD), ref_ld[inf]) and not np.isinf(got[~inf & ~rn]).any(), f"{what}: infinities differ"
    ok = ~rn & ~inf
    bound = ulp32(ref_ld) / LD(2.0) + np.broadcast_to(np.asarray(logbin_bound_db(count), LD)[:, None], ref_ld.shape)
    ratio = np.zeros(ref_ld.shape, LD)
    ratio[ok] = np.abs(got[ok].astype(LD) - ref_ld[ok]) / bound[ok]
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, (f"{what}: error / bound {worst:.3f} at (bin, frame) {np.unravel_index(int(np.argmax(ratio)), ratio.shape)}: "
                          f"{got.flat[int(np.argmax(ratio))]!r} against {ref_ld.flat[int(np.argmax(ratio))]!r}")
    return worst


LB_FRAMES = (1, 63, 64, 65, 200)                      # below, at and above the (F, T) kernel's 64-frame workgroup
LB_FRAMES_WIDE = (1, 65, 3)                           # at 8193 rows
LB_COUNTS = (9, 0, 1, 17, 2, 8, 16, 10, 18, 300)      # the frame-major kernel adds rows in groups of 8 after the first
LB_LEAD = 2                                           # rows between k_base and the first bin
LB_GEOMETRIES = ((383, 0), (420, 37), (8193, 0), (8193, 37))      # (rows of the matrix, k_base)


def logbin_bins(nrows, k_base):
    """first[b] (relative to k_base) and count[b] for the counts of LB_COUNTS: the small bins packed from row
    k_base + LB_LEAD on, the 300-row bin ending on the matrix's last row."""
    count = np.array(LB_COUNTS, np.int32)
    first = np.zeros(count.size, np.int32)
    pos = LB_LEAD
    for b, c in enumerate(LB_COUNTS):
        if c == 300:
            first[b] = nrows - k_base - 300
        elif c > 0:
            first[b] = pos
            pos += c
    assert pos <= nrows - k_base - 300
    return first, count


@functools.lru_cache(maxsize=None)
def logbin_case(nrows, k_base):
    """One ragged launch: (first, count, matrices (nrows, T) float32 for the frame counts T, their long-double reference).
    Random dB in [-120, 20]; planted, in the rows of the bin with the count named:
    8: every row at -700 dB (the mean is below 1e-30: exactly -600 dB);  9: a -inf dB row in frame 0;  10: +inf in the last
    row, last frame;  2: 0 dB beside -300 dB;  18: a NaN in the last row of frame T // 2;  300: a NaN in the middle row of
    frame 0 of the second element;  and a NaN and +90 dB in the rows between k_base and the first bin, which no bin reads."""
    first, count = logbin_bins(nrows, k_base)
    row0 = {int(c): k_base + int(f) for f, c in zip(first, count)}
    rng = np.random.default_rng([12, nrows, k_base])
    mats = []
    for e, T in enumerate(LB_FRAMES if nrows < 8193 else LB_FRAMES_WIDE):
        m = rng.uniform(-120.0, 20.0, (nrows, T)).astype(np.float32)
        m[row0[8]:row0[8] + 8, :] = -700.0
        m[row0[9] + 4, 0] = -np.inf
        m[row0[10] + 9, T - 1] = np.inf
        m[row0[2], :], m[row0[2] + 1, :] = 0.0, -300.0
        m[row0[18] + 17, T // 2] = np.nan
        if e == 1:
            m[row0[300] + 150, 0] = np.nan
        m[k_base:k_base + LB_LEAD, :] = 90.0
        m[k_base + LB_LEAD - 1, 0] = np.nan
        m.setflags(write=False)
        mats.append(m)
    refs = tuple(logbin(m, k_base, first, count)[0] for m in mats)
    return first, count, tuple(mats), refs
