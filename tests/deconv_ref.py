"""Reference for the kernels of ira_deconv.hip: ira_deconv_divide and ira_deconv_finish.

Plain NumPy restatements of the two steps of the reference's analyse/deconvolve.py (:150-169 the regularised spectral
division, :180-191 with :101-107 the DC removal and the one peak normalisation per file), written from those lines and
sharing no code with the kernels or the engine; the case tables the GPU tests launch, the small ragged end-to-end batch
of tests/test_gpu_deconvolve.py, and the comparison functions.  tests/test_deconv_ref_cpu.py ties the restatements to
the oracle and shows that the case tables reject the subtly wrong kernels one could write.

divide works in np.longdouble; the device works in float64 and may be off by 8 * 2^-53 |H| per bin, normwise: the
complex product (2u), the power (3u), + eps (1u), the division (1u).  finish is float32 arithmetic: apart from the mean
(a float64 sum on the device, long double here) every step is one correctly rounded float32 operation, so given the
device's own mean the device must return the restatement's bits.
"""
import functools

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
LONGDOUBLE_OK = np.finfo(LD).nmant >= 63
U = 2.0 ** -53


def need_longdouble():
    import pytest
    if not LONGDOUBLE_OK:
        pytest.skip("np.longdouble has no 64-bit mantissa on this machine: no reference more precise than float64")


# -------------------------------------------------------------------------------------------------------------- divide
def divide(Y, X, n_fft, reg):
    """H = Y conj(X) / (p + eps) over the n_fft // 2 + 1 bins, p = hypot(re X, im X)^2, eps = reg * max(1e-30, max p), in
    np.longdouble.  Returns (H as np.clongdouble, max p).

    p is held the way the reference and the device hold it, as a float64: the long-double power is rounded once to
    float64, so a magnitude of 1e160 overflows the power to inf and one of 1e-160 leaves a subnormal power, as in NumPy
    (long double has the range for both and would otherwise describe a computation neither side performs).  In the
    normal range that rounding is half an ulp, inside the 3u the bound allows for the power.  max(1e-30, .) is Python's
    max, as in the reference: it returns 1e-30 unless the second argument is greater."""
    nb = int(n_fft) // 2 + 1
    Y, X = np.asarray(Y)[:nb], np.asarray(X)[:nb]
    yr, yi = Y.real.astype(LD), Y.imag.astype(LD)
    xr, xi = X.real.astype(LD), X.imag.astype(LD)
    with np.errstate(all="ignore"):
        p = (np.hypot(xr, xi) ** 2).astype(np.float64).astype(LD)
        pmax = np.max(p)
        eps = LD(reg) * (pmax if pmax > LD(1e-30) else LD(1e-30))
        den = p + eps
        H = np.empty(nb, CLD)
        H.real = (yr * xr + yi * xi) / den
        H.imag = (yi * xr - yr * xi) / den
    return H, pmax


def check_pmax(got, ref, what=""):
    """The device's max |X|^2 within 2 float64 ulp of the long-double maximum; inf is inf."""
    got, ref = float(got), LD(ref)
    if not np.isfinite(ref):
        assert got == float(ref), (what, got, ref)
        return
    assert abs(LD(got) - ref) <= 2.0 * np.spacing(np.float64(ref)), (what, got, ref)


def check_divide(got, ref, what=""):
    """got complex128, ref np.clongdouble: the same NaN and inf components, and |got - ref| <= 8 * 2^-53 |ref| on the
    complex value of every finite bin.  Returns the largest error in units of 2^-53 |ref|."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.complex128, (what, got.shape, ref.shape, got.dtype)
    for part in ("real", "imag"):
        g, r = getattr(got, part), getattr(ref, part)
        assert np.array_equal(np.isnan(g), np.isnan(r)), f"{what}: NaN pattern of the {part} parts differs"
        inf = np.isinf(r)
        assert np.array_equal(np.isinf(g), inf) and np.array_equal(g[inf], r[inf].astype(np.float64)), \
            f"{what}: inf pattern of the {part} parts differs"
    ok = np.isfinite(ref.real) & np.isfinite(ref.imag)
    with np.errstate(all="ignore"):
        err = np.hypot(got.real[ok].astype(LD) - ref.real[ok], got.imag[ok].astype(LD) - ref.imag[ok])
        mag = np.hypot(ref.real[ok], ref.imag[ok])
    assert np.all(err[mag == 0] == 0), f"{what}: a bin that is exactly zero came back non-zero"
    units = err[mag > 0] / (mag[mag > 0] * LD(U))
    worst = float(units.max()) if units.size else 0.0
    assert worst <= 8.0, f"{what}: |dH| = {worst:.2f} * 2^-53 |H| at its worst bin (8 allowed)"
    return worst


DIV_REG = (0.0, 1e-10, 1e-6, 1.0)
#               n_fft  what X holds                                       X shared with entry
DIV_ENTRIES = ((2,    "noise", None), (8, "peak_first", None), (512, "peak_last", None), (4096, "peak_last", None),
               (4096, "shared", 3), (4096, "peak_tail", None), (512, "zero", None), (8, "1e-160", None),
               (512, "1e150", None), (8, "1e160", None))


@functools.lru_cache(maxsize=None)
def divide_case():
    """One launch for every reg of DIV_REG: entries of 2, 5, 257 and 2049 bins (a block that is partly filled, entries far
    smaller than max_nfft, more than one grid stride).  The largest |X|^2 sits at bin 0 (entry 1), at the last bin (2, 3: bin
    2048 is the only bin of the last, partly filled grid stride) and at bin 2047, the last bin of the last full stride (5); entry 4 divides another Y by entry 3's X; entry 6 has
    X = 0 (H = 0 with reg > 0, NaN with reg = 0); entries 7-9 have |X| of 1e-160, 1e150 and 1e160 (the last overflows the
    power).  Returns (Y list, X list, share list) with complex128 spectra; X[e] is X[share[e]] where share[e] is set."""
    rng = np.random.default_rng(13)
    Ys, Xs, share = [], [], []
    for n_fft, kind, sh in DIV_ENTRIES:
        nb = n_fft // 2 + 1
        Y = rng.standard_normal(nb) + 1j * rng.standard_normal(nb)
        X = (rng.standard_normal(nb) + 1j * rng.standard_normal(nb)) * rng.uniform(0.01, 1.0, nb)
        if kind == "peak_first":
            X[0] = 7.0 - 3.0j
        elif kind == "peak_last":
            X[-1] = -6.0 + 5.0j
        elif kind == "peak_tail":
            X[2047] = 5.0 + 8.0j
        elif kind == "zero":
            X[:] = 0.0
        elif kind in ("1e-160", "1e150", "1e160"):
            X = X / np.abs(X) * float(kind)
        elif kind == "shared":
            X = Xs[sh]
        Y.setflags(write=False)
        X.setflags(write=False)
        Ys.append(Y), Xs.append(X), share.append(sh)
    return tuple(Ys), tuple(Xs), tuple(share)


# -------------------------------------------------------------------------------------------------------------- finish
def mean32(h, n):
    """float32 of the long-double mean of the first n samples."""
    with np.errstate(all="ignore"):
        return np.float32(np.sum(np.asarray(h, np.float32)[:n].astype(LD)) / LD(n)) if n > 0 else np.float32(0.0)


def finish(h_list, n_out, group, remove_dc, normalise_peak, target, mean=None):
    """Each h float32, of any length >= n_out[e]; only its first n_out[e] samples are touched.  remove_dc: h - mean as a
    float32 subtraction, the mean taken in long double and rounded to float32, or mean[e] when given.  normalise_peak: per
    group, peak = np.max(np.abs(.)) over all its channels (a NaN sample makes it NaN); only peak <= 0 leaves the group as
    it is, a NaN peak scales by NaN like the reference; scale = float32(target / float64(peak)), a float32 multiplication.
    Returns (the list of new arrays, the float32 means or None)."""
    out = [np.array(h, dtype=np.float32, copy=True) for h in h_list]
    n_out, group = [int(n) for n in n_out], [int(g) for g in group]
    means = None
    with np.errstate(all="ignore"):
        if remove_dc:
            means = np.array([mean32(h, n) if mean is None else np.float32(mean[e])
                              for e, (h, n) in enumerate(zip(out, n_out))], np.float32)
            for h, n, mu in zip(out, n_out, means):
                h[:n] = h[:n] - mu
        if normalise_peak:
            for g in sorted(set(group)):
                members = [e for e in range(len(out)) if group[e] == g and n_out[e] > 0]
                if not members:
                    continue
                peak = np.max(np.array([np.max(np.abs(out[e][:n_out[e]])) for e in members], np.float32))
                if peak <= 0.0:
                    continue
                scale = np.float32(float(target) / float(np.float64(peak)))
                for e in members:
                    out[e][:n_out[e]] = out[e][:n_out[e]] * scale
    return out, means


def check_mean(got, h, n, what=""):
    """The device's float32 mean within ulp32 / 2 + n * 2^-53 * mean|h| of the long-double mean."""
    x = np.asarray(h, np.float32)[:n].astype(LD)
    ref = np.sum(x) / LD(n)
    _, e = np.frexp(np.abs(ref))
    half_ulp = np.ldexp(LD(1.0), int(max(int(e) - 24, -149))) / LD(2.0)
    tol = half_ulp + LD(n) * LD(U) * (np.sum(np.abs(x)) / LD(n))
    assert abs(LD(np.float32(got)) - ref) <= tol, (what, float(got), float(ref), float(tol))


def check_finish(got, ref, n, what=""):
    """One channel's slot: the first n samples have the same NaN cells and the same bits everywhere else; every sample of
    the tail has the same bits."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float32, (what, got.shape, ref.shape, got.dtype)
    gb, rb = got.view(np.uint32), ref.view(np.uint32)
    assert np.array_equal(gb[n:], rb[n:]), f"{what}: the tail past n_out was written"
    gn, rn = np.isnan(got[:n]), np.isnan(ref[:n])
    assert np.array_equal(gn, rn), f"{what}: NaN cells differ ({int(gn.sum())} against {int(rn.sum())} of the reference)"
    bad = ~rn & (gb[:n] != rb[:n])
    assert not bad.any(), (f"{what}: {int(bad.sum())} samples differ, first at {int(np.argmax(bad))}: "
                           f"{got[:n][bad][0]!r} against {ref[:n][bad][0]!r}")


FIN_N_OUT = (1, 63, 1023, 1024, 1025, 2048, 2049, 5000)        # around the 1024-thread mean pass and the 2048-sample blocks
FIN_GROUP = (2, 0, 1, 2, 0, 2, 3, 3)                           # unsorted files of 3, 2, 1 and 2 channels
FIN_TARGET = (0.95, 0.5, 1e-3)
FIN_TAIL = 0xA5A50000                                          # tail sample j holds the bits FIN_TAIL + j


def tail_bits(k):
    return (np.uint32(FIN_TAIL) + np.arange(k, dtype=np.uint32)).view(np.float32)


@functools.lru_cache(maxsize=None)
def finish_case():
    """(slots, n_out, group): channel e is a slot of n_out[e] samples and a tail of 5 + e samples of fixed bits.  Decaying
    noise on a DC offset, each channel at its own level; the peak of file 2 lies in its second channel (entry 3); file 1
    (entry 2) is all zero."""
    rng = np.random.default_rng(14)
    slots = []
    for e, n in enumerate(FIN_N_OUT):
        level = (0.02, 0.3, 0.0, 4.0, 0.7, 0.5, 1e-3, 2e-3)[e]
        x = level * (rng.standard_normal(n) * np.exp(-np.arange(n) / (0.3 * n + 1.0)) + 0.11 * (1 + e % 3))
        s = np.concatenate([np.abs(x.astype(np.float32)) if level == 0.0 else x.astype(np.float32), tail_bits(5 + e)])
        s.setflags(write=False)
        slots.append(s)
    return tuple(slots), FIN_N_OUT, FIN_GROUP


@functools.lru_cache(maxsize=None)
def finish_nonfinite_case(bad):
    """Five channels in files (0, 0, 1, 1, 2): file 0's second channel and file 1's first hold one `bad` sample (NaN or inf),
    file 2 is finite."""
    rng = np.random.default_rng(15)
    n_out, group = (700, 700, 2049, 2049, 300), (0, 0, 1, 1, 2)
    slots = []
    for e, n in enumerate(n_out):
        x = (0.2 + 0.1 * e) * rng.standard_normal(n) + 0.05
        if e == 1:
            x[n - 1] = bad
        if e == 2:
            x[1030] = bad
        s = np.concatenate([x.astype(np.float32), tail_bits(4)])
        s.setflags(write=False)
        slots.append(s)
    return tuple(slots), n_out, group


# ---------------------------------------------------------------------------------------------- end to end, small sizes
E2E_FILES = ((8, 2, 8), (9, 1, 64), (100, 2, 700), (1000, 1, 64), (5000, 1, 4096))      # (samples, channels, sweep samples)
E2E_SETTINGS = tuple((mode, reg) for mode in ("recorded", "full_fft") for reg in (1e-10, 1e-6))


@functools.lru_cache(maxsize=None)
def e2e_files():
    """[(recording (N, C) float32, sweep float32)]: two stereo and three mono files whose channels need transforms of 8, 64,
    1024, 1024 and 8192 points in one batch; sweeps longer and shorter than their recordings.  A recording is its sweep (a
    noise burst, so no bin of its spectrum is empty) convolved with a short known response, cut to the recording's length."""
    rng = np.random.default_rng(16)
    files = []
    for n_rec, chans, n_sw in E2E_FILES:
        sweep = (0.1 * rng.standard_normal(n_sw)).astype(np.float32)        # recordings stay inside [-1, 1]: nothing clips
        rec = np.zeros((n_rec, chans), np.float32)
        for c in range(chans):
            g = np.array([0.0, 0.9 - 0.5 * c, 0.0, -0.35, 0.2 * (c + 1), 0.05])
            rec[:, c] = np.convolve(sweep.astype(np.float64), g)[:n_rec].astype(np.float32) if n_rec <= n_sw + 5 else \
                np.pad(np.convolve(sweep.astype(np.float64), g), (0, n_rec - n_sw - 5)).astype(np.float32)
        rec.setflags(write=False)
        sweep.setflags(write=False)
        files.append((rec, sweep))
    return tuple(files)


def next_power_of_two(n):
    return 1 if n <= 1 else 1 << (int(n - 1).bit_length())


def deconvolve_f64(rec, sweep, reg, normalise_peak=True, target=0.95, remove_dc=True, mode="recorded"):
    """The restatements composed with numpy.fft in float64: rfft, divide (rounded to complex128), irfft -> float32,
    finish.  Returns ((N_out, C) float32, the float64 responses before the float32 rounding)."""
    n_rec, chans = rec.shape
    n_fft = next_power_of_two(max(n_rec, sweep.size))
    X = np.fft.rfft(sweep.astype(np.float64), n=n_fft)
    raw = []
    for c in range(chans):
        H, _ = divide(np.fft.rfft(rec[:, c].astype(np.float64), n=n_fft), X, n_fft, reg)
        raw.append(np.fft.irfft(H.astype(np.complex128), n=n_fft))
    n_out = n_rec if mode == "recorded" else n_fft
    hs, _ = finish([h.astype(np.float32) for h in raw], [n_out] * chans, [0] * chans, remove_dc, normalise_peak, target)
    return np.stack([h[:n_out] for h in hs], axis=1), raw
