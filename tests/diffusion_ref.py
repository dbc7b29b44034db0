"""
Restatement of the diffusion metrics (ira_diffusion.hip: max |autocorrelation|, echo density, corr0, IACC per window) in
NumPy alone, for the tests: no torch, no oracle, no np.mean.

Two kinds of quantity:
  * echo density is a COUNT over float32 values, so every float32 step of the reference is restated in its order -- the
    mean and the rms through np_pairwise_sum_f32, NumPy's float32 pairwise summation spelled out addition by addition, so
    that the expectation does not depend on how the installed NumPy was built;
  * the three correlation quantities take the same float32 mean-removed window and sum in np.longdouble: the value the
    kernel's float64 sums approximate, not the reference's float32-BLAS one.
"""
import math

import numpy as np

LD = np.longdouble
F32 = np.float32
SILENCE = 1e-20                   # energies and rms at or below this give NaN
MIN_EXCEEDANCE = 1e-12            # Gaussian exceedances at or below this give NaN
NAN32 = F32(np.nan)


# ---------------------------------------------------------------------------------------------------- float32 pairwise sum
def pairwise_leaves(n):
    """[(start, length)] of the <= 128-value blocks NumPy's pairwise sum cuts n values into, left to right."""
    if n <= 128:
        return [(0, n)]
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_leaves(n2) + [(n2 + s, l) for s, l in pairwise_leaves(n - n2)]


def np_pairwise_sum_f32(a):
    """np.add.reduce of a contiguous float32 array, every addition rounded to float32."""
    a = np.ascontiguousarray(a, dtype=F32)
    n = a.size
    if n < 8:
        res = F32(0.0)
        for v in a:
            res = F32(res + v)
        return res
    if n <= 128:
        r = a[:8].copy()
        i = 8
        while i < n - (n % 8):
            r = r + a[i : i + 8]                                # eight float32 additions
            i += 8
        res = F32(F32(F32(r[0] + r[1]) + F32(r[2] + r[3])) + F32(F32(r[4] + r[5]) + F32(r[6] + r[7])))
        for v in a[i:]:
            res = F32(res + v)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return F32(np_pairwise_sum_f32(a[:n2]) + np_pairwise_sum_f32(a[n2:]))


def mean_f32(a):
    """np.mean of a float32 array: the pairwise sum divided by float32(n), in float32."""
    return F32(np_pairwise_sum_f32(a) / F32(a.size))


def remove_mean(w):
    w = np.ascontiguousarray(w, dtype=F32)
    w0 = w - mean_f32(w)
    assert w0.dtype == F32
    return w0


# ---------------------------------------------------------------------------------------------------- one window
def lag_sums(cur, src, lag_lo, lag_hi):
    """[sum_k cur[k] src[k - lag] for lag = lag_lo..lag_hi] in long double."""
    c, s = cur.astype(LD), src.astype(LD)
    n = c.size
    return np.array([np.dot(c[lag:], s[: n - lag]) for lag in range(lag_lo, lag_hi + 1)], dtype=LD)


def _peak_of(values, lags):
    """(peak, lag of the peak, runner-up) of |values|."""
    mag = np.abs(values)
    k = int(np.argmax(mag))
    rest = np.delete(mag, k)
    return mag[k], int(lags[k]), (rest.max() if rest.size else LD(0.0))


def window_autocorr(w, max_lag):
    """(peak, lag_of_peak, runner_up) of |r(lag)|, r = sum w0[k] w0[k + lag] / sum w0^2, lag = 1..min(max_lag, n - 2)."""
    n = int(np.size(w))
    nan = (LD(np.nan), 0, LD(np.nan))
    if n < 4:
        return nan
    w0 = remove_mean(w)
    den = np.dot(w0.astype(LD), w0.astype(LD))
    if den <= SILENCE:
        return nan
    lmax = min(int(max_lag), n - 2)
    return _peak_of(lag_sums(w0, w0, 1, lmax) / den, np.arange(1, lmax + 1))


def gaussian_exceedance(k):
    """P(|x| > k sigma) of a Gaussian."""
    phi = 0.5 * (1.0 + math.erf(float(k) / np.sqrt(2.0)))
    return 2.0 * (1.0 - phi)


def echo_density_parts(w):
    """(w0, rms) as the reference forms them: float32 products, pairwise mean, float32 sqrt."""
    w0 = remove_mean(w)
    sq = w0 * w0
    assert sq.dtype == F32
    return w0, F32(np.sqrt(mean_f32(sq)))


def window_echo_density(w, thr_rms, normalise):
    """fraction(|w0| > thr_rms rms), over the Gaussian exceedance if asked; float32."""
    n = int(np.size(w))
    if n < 4:
        return NAN32
    w0, rms = echo_density_parts(w)
    if float(rms) <= SILENCE:
        return NAN32
    thr = F32(float(thr_rms) * float(rms))
    frac = float(np.count_nonzero(np.abs(w0) > thr)) / float(n)
    if not normalise:
        return F32(frac)
    ex = gaussian_exceedance(thr_rms)
    return NAN32 if ex <= MIN_EXCEEDANCE else F32(frac / ex)


def _energies(a, b):
    a0, b0 = remove_mean(a), remove_mean(b)
    al, bl = a0.astype(LD), b0.astype(LD)
    return a0, b0, np.dot(al, al), np.dot(bl, bl), np.dot(al, bl)


def window_corr0(a, b):
    n = int(np.size(a))
    if n != int(np.size(b)) or n < 4:
        return LD(np.nan)
    _, _, aa, bb, ab = _energies(a, b)
    if aa <= SILENCE or bb <= SILENCE:
        return LD(np.nan)
    return ab / np.sqrt(aa * bb)


def window_iacc(a, b, max_lag, detail=False):
    """max |sum a0[k] b0[k + lag]| / sqrt(aa bb) over lag = -L..L, L = min(max_lag, n - 2); lag 0 once.
    detail=True: (peak, signed lag of the peak, runner-up)."""
    n = int(np.size(a))
    nan = LD(np.nan)
    if n != int(np.size(b)) or n < 4:
        return (nan, 0, nan) if detail else nan
    a0, b0, aa, bb, _ = _energies(a, b)
    den = np.sqrt(aa * bb)
    if den <= SILENCE:
        return (nan, 0, nan) if detail else nan
    lmax = min(int(max_lag), n - 2)
    pos = lag_sums(b0, a0, 0, lmax)                             # sum_k a0[k] b0[k + lag], lag >= 0
    neg = lag_sums(a0, b0, 1, lmax)                             # sum_k a0[k + lag] b0[k], lag >= 1
    out = _peak_of(np.concatenate([pos, neg]) / den, np.concatenate([np.arange(0, lmax + 1), -np.arange(1, lmax + 1)]))
    return out if detail else out[0]


# ---------------------------------------------------------------------------------------------------- series
def series_mono(x, start, frames, win, hop, max_lag, thr_rms=1.0, normalise=True, exact=False):
    """(max_abs_autocorr, echo_density) of `frames` windows of x from `start`: float32 arrays.  exact=True leaves the
    autocorrelation peaks in long double (the kernel's bar allows ONE float32 rounding, its own)."""
    ac = np.zeros(frames, dtype=LD)
    ed = np.zeros(frames, dtype=F32)
    for f in range(frames):
        w = x[start + f * hop : start + f * hop + win]
        assert w.size == win
        ac[f] = window_autocorr(w, max_lag)[0]
        ed[f] = window_echo_density(w, thr_rms, normalise)
    return (ac if exact else ac.astype(F32)), ed


def series_stereo(left, right, start, frames, win, hop, max_lag, exact=False):
    """(corr0, iacc_max) of `frames` window pairs from `start`: float32 arrays (long double with exact=True)."""
    c0 = np.zeros(frames, dtype=LD)
    ia = np.zeros(frames, dtype=LD)
    for f in range(frames):
        a = left[start + f * hop : start + f * hop + win]
        b = right[start + f * hop : start + f * hop + win]
        assert a.size == win and b.size == win
        c0[f] = window_corr0(a, b)
        ia[f] = window_iacc(a, b, max_lag)
    return (c0, ia) if exact else (c0.astype(F32), ia.astype(F32))


def bound(ref, win):
    """|got - ref| allowed for a correlation quantity: one float32 rounding of the output, plus float64 accumulation --
    sum |a_k b_k| <= den (Cauchy-Schwarz), so a sum of win products is within win 2^-53 den of exact; numerator,
    denominator and quotient make at most four such terms."""
    return 2.0 ** -24 * np.abs(np.asarray(ref, dtype=np.float64)) + 4.0 * win * 2.0 ** -53


# ---------------------------------------------------------------------------------------------------- windows
NOISE_LEVEL = 0.01


def two_spike(n, d, i, rng):
    """0.01-level Gaussian noise with +1 at i and i + d: the autocorrelation peak (about 0.45) sits at lag d."""
    assert 0 <= i and d >= 1 and i + d < n
    w = NOISE_LEVEL * rng.standard_normal(n)
    w[i] += 1.0
    w[i + d] += 1.0
    return w.astype(F32)


def two_spike_stereo(n, d, i, rng):
    """(left, right): noise with +1 at i on the left and at i + d on the right (d may be negative or 0): the cross
    correlation sum a[k] b[k + lag] peaks at lag d."""
    assert 0 <= i < n and 0 <= i + d < n
    a = NOISE_LEVEL * rng.standard_normal(n)
    b = NOISE_LEVEL * rng.standard_normal(n)
    a[i] += 1.0
    b[i + d] += 1.0
    return a.astype(F32), b.astype(F32)


def spike_row(n, d):
    """Where the tests put the first spike of two_spike(n, d, ...): spread over the window, always in range."""
    return (7 * d) % (n - d)


def alternating(n):
    """+1, -1, ...: mean exactly 0 and rms exactly 1 (n even)."""
    w = np.ones(n, dtype=F32)
    w[1::2] = -1.0
    return w


def decaying_noise(n, seed, dc=0.3):
    """Gaussian noise under an exponential envelope (30 dB down over the n samples) on a DC offset."""
    rng = np.random.default_rng(seed)
    env = 10.0 ** (-1.5 * np.arange(n) / max(n, 1))
    return (dc + rng.standard_normal(n) * env).astype(F32)


# ---------------------------------------------------------------------------------------------------- inputs the tests share
# (built once here: the CPU file proves that each input tests what it claims, the GPU file runs the kernels on the same ones)
PLAN_WINS = [4, 7, 8, 9, 15, 16, 17, 127, 128, 129, 136, 143, 255, 256, 257, 1000, 2401, 4099, 8191, 8192]
EVERY_LAG_N = 64
BOUNDARY_N, BOUNDARY_LAGS = 2402, [1, 9, 10, 2295, 2296, 2297, 2304, 2399, 2400]
BOUNDARY_MAX_LAGS = [2400, 2295, 1148]                          # nsub == 1 (>= 256 groups), 255 groups, 128 groups
CLIP_D = 40
SUBRANGE_N, SUBRANGE_ROWS = 2400, [9, 10, 18, 19, 2389]
DIRECTION_LAGS = [0, 1, -1, 9, -9, 10, -10, 61, -61, 62, -62]
LONG_STEREO_LAGS = [2295, -2295, 2296, -2296, 2400, -2400]


def every_lag_windows():
    """[(d, window)]: n = 64, every lag d = 1..62 planted once."""
    n = EVERY_LAG_N
    return [(d, two_spike(n, d, spike_row(n, d), np.random.default_rng(1000 + d))) for d in range(1, n - 1)]


def boundary_windows():
    """[(d, window)]: n = 2402, peaks planted at the lag-group and row-split boundaries."""
    n = BOUNDARY_N
    return [(d, two_spike(n, d, spike_row(n, d), np.random.default_rng(2000 + d))) for d in BOUNDARY_LAGS]


def clip_window():
    n = EVERY_LAG_N
    return two_spike(n, CLIP_D, spike_row(n, CLIP_D), np.random.default_rng(3000))


def subrange_windows(d):
    """[(row, window)]: n = 2400, lag d planted with its first spike at the rows around the row sub-range edges."""
    return [(i, two_spike(SUBRANGE_N, d, i, np.random.default_rng(4000 + 10 * d + k))) for k, i in enumerate(SUBRANGE_ROWS)]


def _stereo_row(n, d):
    return spike_row(n, abs(d)) + (abs(d) if d < 0 else 0) if d else 23


def direction_pairs(lags=DIRECTION_LAGS, n=EVERY_LAG_N, seed=5000):
    """[(d, left, right)]: the cross-correlation peak planted at signed lag d."""
    return [(d,) + two_spike_stereo(n, d, _stereo_row(n, d), np.random.default_rng(seed + 100 + d)) for d in lags]


def long_stereo_pairs():
    return direction_pairs(LONG_STEREO_LAGS, BOUNDARY_N, 6000 + 3000)


NAN_RULE_N = 64


def nan_rule_windows():
    """{name: (window, autocorrelation finite?, echo density finite?)} for the silence rules, n = 64."""
    n = NAN_RULE_N
    rng = np.random.default_rng(7000)
    return {
        "zeros": (np.zeros(n, dtype=F32), False, False),
        "const_0.5": (np.full(n, 0.5, dtype=F32), False, False),                 # float32 mean exact: w0 == 0
        "const_0.1": (np.full(n, 0.1, dtype=F32), True, True),                   # float32 mean inexact: |w0| == 2^-27
        "noise_1e-12": ((1e-12 * rng.standard_normal(n)).astype(F32), False, True),
        "noise": (rng.standard_normal(n).astype(F32), True, True),
    }


def degenerate_pairs():
    """{name: (left, right, corr0 finite?, iacc finite?)}, n = 64."""
    n = NAN_RULE_N
    rng = np.random.default_rng(8000)
    a = rng.standard_normal(n).astype(F32)
    b = rng.standard_normal(n).astype(F32)
    return {
        "identical": (a, a.copy(), True, True),
        "negated": (a, -a, True, True),
        "right_zeros": (a, np.zeros(n, dtype=F32), False, False),
        "left_1e-12": ((1e-12 * b).astype(F32), a, False, True),
    }
