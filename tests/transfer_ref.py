"""
Float64 NumPy restatement of the dual-channel spectral sums (ira_xspec.hip, audio_analysis_amd/analyse/transfer.py) and
the bound its device results are held to.  Helper module, like echo_ref.py / decay_ref.py: it holds no tests.

A pair is (reference x, measurement y, delay d):  x'[n] = x[n + max(0, -d)],  y'[n] = y[n + max(0, d)],
N = min(len x - max(0, -d), len y - max(0, d)),  K = 1 + (N - n_fft) // hop frames (0 when N < n_fft), frame f at f hop,
X_f = rfft(w x'_f), Y_f = rfft(w y'_f) in float64 (each channel its OWN real transform here: the device packs both into
one complex transform), Sxx = sum_f |X_f|^2, Syy = sum_f |Y_f|^2, Sxy = sum_f conj(X_f) Y_f, frames added in ascending
order.  The window is what Engine.window holds: numpy.hanning(n_fft) or ones, float64.
"""
import math

import numpy as np

FRAMES_PER_CHUNK = 16          # IRA_XSPEC_FRAMES
ROWS = ("sxx", "syy", "sxy_re", "sxy_im", "h1_re", "h1_im", "h2_re", "h2_im", "coherence", "mag_db", "phase_rad")
U = 2.0 ** -53


def window(n_fft, name):
    """The table of Engine.window(n_fft, name == "hann", 64), restated."""
    if name == "hann":
        return np.hanning(n_fft).astype(np.float64)
    if name == "rect":
        return np.ones(n_fft, dtype=np.float64)
    raise ValueError(name)


def hop_of(n_fft, overlap):
    return max(1, n_fft - int(math.floor(overlap * n_fft + 0.5)))


def geometry(lx, ly, d):
    """(x skip, y skip, N)."""
    xs, ys = max(0, -d), max(0, d)
    return xs, ys, max(0, min(lx - xs, ly - ys))


def frames(n, n_fft, hop):
    return 1 + (n - n_fft) // hop if n >= n_fft else 0


def frame_spectra(x, y, d, n_fft, hop, win):
    """(X (K, nbins) complex128, Y (K, nbins), nf (K,)): the frames' spectra and joint norms
    nf = sqrt(||w x'_f||^2 + ||w y'_f||^2)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    xs, ys, n = geometry(x.size, y.size, d)
    k = frames(n, n_fft, hop)
    nb = n_fft // 2 + 1
    X, Y, nf = np.zeros((k, nb), complex), np.zeros((k, nb), complex), np.zeros(k)
    for f in range(k):
        a = win * x[xs + f * hop : xs + f * hop + n_fft]
        b = win * y[ys + f * hop : ys + f * hop + n_fft]
        X[f], Y[f] = np.fft.rfft(a), np.fft.rfft(b)
        nf[f] = math.sqrt(float(np.dot(a, a)) + float(np.dot(b, b)))
    return X, Y, nf


def sums(X, Y):
    """(Sxx, Syy, Sxy) of frame_spectra's X and Y, frames added in ascending order."""
    nb = X.shape[1]
    sxx, syy, sxy = np.zeros(nb), np.zeros(nb), np.zeros(nb, complex)
    for f in range(X.shape[0]):
        sxx += X[f].real ** 2 + X[f].imag ** 2
        syy += Y[f].real ** 2 + Y[f].imag ** 2
        sxy += np.conj(X[f]) * Y[f]
    return sxx, syy, sxy


def tolerance(X, Y, nf, n_fft):
    """Bounds (on |dSxx|, |dSyy|, |dSxy|, per bin) for sums formed from float64 transforms -- derived, not fitted.

    One packed transform z = w x'_f + i w y'_f has normwise error at most g nf: every output bin is off by at most
    g nf in magnitude, with
        g  = 16 log2(n_fft) 2^-53    a float64 radix FFT with table twiddles (a few roundings per butterfly level, log2(n_fft)
                                     levels; 16 per level leaves room for the twiddle table's own rounding, the window multiply
                                     and the unpacking of the two channels), on the device and in NumPy alike;
        nf = sqrt(||w x'_f||^2 + ||w y'_f||^2)    the JOINT norm: both channels ride one transform, so a quiet channel
                                     carries the loud channel's rounding error.
    So |dX_f[k]|, |dY_f[k]| <= g nf.  With |X + dX|^2 - |X|^2 = 2 Re(conj(X) dX) + |dX|^2 -- the second-order term is
    left out: it matters only in bins with |X_f[k]| below g nf, fifteen decimal orders under the frame's norm, which
    broadband test signals do not have (a channel that is all zeros is exact by construction on the device) -- and
    K - 1 additions plus the 3 roundings of each product-sum and one of the chunk fold, each at most 2^-53 of a partial
    sum of non-negative terms <= the whole sum:
        |dSxx[k]| <= 2 g sum_f nf |X_f[k]| + (K + 4) 2^-53 Sxx[k]                        (the same for Syy)
        |dSxy[k]| <= g sum_f nf (|X_f[k]| + |Y_f[k]|) + (K + 4) 2^-53 sum_f |X_f[k]| |Y_f[k]|
    (conj(X) Y picks up conj(dX) Y + conj(X) dY; its partial sums are bounded by the sum of the magnitudes).
    """
    k = X.shape[0]
    g = 16.0 * math.log2(n_fft) * U
    ax, ay = np.abs(X), np.abs(Y)
    w = nf[:, None]
    bxx = 2.0 * g * np.sum(w * ax, axis=0) + (k + 4) * U * np.sum(ax * ax, axis=0)
    byy = 2.0 * g * np.sum(w * ay, axis=0) + (k + 4) * U * np.sum(ay * ay, axis=0)
    bxy = g * np.sum(w * (ax + ay), axis=0) + (k + 4) * U * np.sum(ax * ay, axis=0)
    return bxx, byy, bxy


def h1_bound(sxx, sxy, bxx, bxy):
    """|dH1| for H1 = Sxy / Sxx with |dSxx| <= bxx, |dSxy| <= bxy: first order, (|dSxy| + |H1| |dSxx|) / Sxx, plus the
    quotient's own rounding (2 ulp on each part); second-order terms are (bxx / Sxx) times the first and get 1 %."""
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.abs(sxy) / sxx
        return 1.01 * (bxy + h * bxx) / sxx + 4.0 * U * h


def coherence_bound(sxx, syy, sxy, bxx, byy, bxy):
    """|d coherence| for c = |Sxy|^2 / (Sxx Syy) before the clamp: c (2 |dSxy| / |Sxy| + |dSxx| / Sxx + |dSyy| / Syy)
    to first order (1 % for the rest), plus 4 roundings of the products and the quotient."""
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.abs(sxy)
        c = a * a / (sxx * syy)
        return 1.01 * c * (2.0 * bxy / a + bxx / sxx + byy / syy) + 8.0 * U * c


def derived(sxx, syy, sre, sim):
    """The eleven rows (ROWS order) from the four sums, operation by operation as ira_xspec_finish forms them (float64,
    one rounding per operation): a quotient whose denominator is 0 is NaN."""
    sxx, syy, sre, sim = (np.asarray(v, dtype=np.float64) for v in (sxx, syy, sre, sim))
    nan = np.full(sxx.shape, np.nan)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        h1r = np.where(sxx == 0.0, nan, sre / sxx)
        h1i = np.where(sxx == 0.0, nan, sim / sxx)
        m2 = sre * sre + sim * sim
        h2r = np.where(m2 == 0.0, nan, syy * sre / m2)
        h2i = np.where(m2 == 0.0, nan, syy * sim / m2)
        den = sxx * syy
        q = np.where(den == 0.0, nan, m2 / den)
        coh = np.where(q > 1.0, 1.0, q)
        mag = 10.0 * np.log10(h1r * h1r + h1i * h1i)
        ph = np.arctan2(sim, sre)
    return np.stack([sxx, syy, sre, sim, h1r, h1i, h2r, h2i, coh, mag, ph])


def status(k, sxx, syy, sxy):
    """1 silent reference (Sxx 0 in every bin, frames present), 2 too short (K < 1), 4 non-finite sums."""
    s = 0
    if k < 1:
        s |= 2
    elif not np.any(sxx != 0.0):
        s |= 1
    if not (np.all(np.isfinite(sxx)) and np.all(np.isfinite(syy)) and np.all(np.isfinite(sxy))):
        s |= 4
    return s


def pair_reference(x, y, d, n_fft, hop, window_name):
    """Everything a test wants of one pair: dict(K, sxx, syy, sxy, rows (11, nbins), bounds (bxx, byy, bxy), status)."""
    X, Y, nf = frame_spectra(x, y, d, n_fft, hop, window(n_fft, window_name))
    with np.errstate(invalid="ignore", over="ignore"):
        sxx, syy, sxy = sums(X, Y)
        return dict(K=X.shape[0], sxx=sxx, syy=syy, sxy=sxy, rows=derived(sxx, syy, sxy.real, sxy.imag),
                    bounds=tolerance(X, Y, nf, n_fft), status=status(X.shape[0], sxx, syy, sxy))


def ulps(got, want):
    """|got - want| in units of the spacing of want, elementwise; 0 where both are NaN or the same infinity, inf where
    only one is NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(got - want) / np.spacing(np.abs(want))
    same = (np.isnan(got) & np.isnan(want)) | (got == want)
    d = np.where(same, 0.0, d)
    return np.where(np.isnan(d), np.inf, d)
