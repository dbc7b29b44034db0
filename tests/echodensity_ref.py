"""
Normalized echo density restated in NumPy from the docstring of audio_analysis_amd.analyse.echodensity, in long double
(or any float type): helper module, it holds no tests and shares no code with the module.

For a channel x (float32) of L samples, onset o, half window delta (W = 2 delta + 1), step S, at most Kmax positions:
  w[k] = 0.5 - 0.5 cos(2 pi (k + 1) / (W + 1)) (hann) | 1 (rect), float64;  K = 0 if L <= o else min((L - 1 - o) // S + 1, Kmax)
  c_j = o + j S;  window i = c_j - delta .. c_j + delta clipped to [0, L), k = i - (c_j - delta);  h2[i] = x[i]^2
  A = sum w[k],  B = sum w[k] h2[i],  in[i] = h2[i] A > B G (G = 1 + 2^-32),  C = sum of w[k] where in[i]
  eta = (C / A) / E,  E = 0.31731050786291415;  NaN where B == 0 (kind 1) or B is not finite (kind 2).

The bound of every comparison with the device is derived, not fitted.  A, B and C are sums of at most W non-negative
terms; the device adds them one rounding at a time in float64, so each is within (W - 1) 2^-53 of its exact value
relatively, the products w h2 add one rounding each, C / A / E three more: (2 W + 16) 2^-53 eta covers the arithmetic
when both sides take the SAME samples as "outside sigma".  The two sides can disagree only on a sample whose h2 A lies
within the rounding of both sides' B G and A of it, |h2 A - B G| <= (W + 8) 2^-52 B G: the weight of such samples is the
position's AMBIGUOUS WEIGHT, and it enters the bound as ambiguous_weight / (A E).  On the seeded inputs of the tests it
is 0 at every position, so the second term vanishes.  The float32 profile gets one float32 ulp on top.
"""
import math

import numpy as np

E = 0.31731050786291415
LD = np.longdouble


def half_window(window_ms, fs):
    return max(1, int(math.floor(window_ms * fs / 2000.0 + 0.5)))


def step_of(step_ms, fs):
    return max(1, int(math.floor(step_ms * fs / 1000.0 + 0.5)))


def kmax_of(max_time_ms, fs, step):
    return (1 << 31) if max_time_ms is None else 1 + int(math.ceil(max_time_ms * fs / 1000.0)) // step


def count(length, onset, step, kmax):
    return 0 if length <= onset else min((length - 1 - onset) // step + 1, kmax)


def weights(delta, window):
    w = 2 * delta + 1
    if window == "rect":
        return np.ones(w, dtype=np.float64)
    assert window == "hann"
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * (k + 1.0) / (w + 1.0)) for k in range(w)], dtype=np.float64)


def onset_index(x, onset_db=-20.0):
    """First n <= peak with x[n]^2 >= x[peak]^2 * 10^(onset_db / 10) (float64), 0 for an empty channel."""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return 0
    e = x * x
    p = int(np.argmax(np.abs(x)))
    return int(np.argmax(e[: p + 1] >= e[p] * 10.0 ** (onset_db / 10.0)))


def profile(x, onset, delta, window, step, kmax=1 << 31, dtype=LD, chunk=256):
    """(eta (K,) dtype with NaN where undefined, kind (K,) int: 0 value / 1 B == 0 / 2 B not finite, ambiguous weight (K,),
    A (K,)) of one channel."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n, w_len = x.size, 2 * delta + 1
    k_pos = count(n, onset, step, kmax)
    w = weights(delta, window).astype(dtype)
    h2 = np.zeros(n + 2 * delta, dtype=dtype)
    h2[delta : delta + n] = x.astype(dtype) ** 2
    valid = np.zeros(n + 2 * delta, dtype=bool)
    valid[delta : delta + n] = True
    eta, kind = np.full(k_pos, np.nan, dtype=dtype), np.zeros(k_pos, dtype=np.int64)
    amb, a_all = np.zeros(k_pos, dtype=dtype), np.zeros(k_pos, dtype=dtype)
    guard = dtype(1.0) + dtype(2.0) ** -32
    eps = dtype(w_len + 8) * dtype(2.0) ** -52
    with np.errstate(invalid="ignore", over="ignore"):
        for j0 in range(0, k_pos, chunk):
            c = onset + step * np.arange(j0, min(j0 + chunk, k_pos))       # padded index of k = 0 is c itself
            idx = c[:, None] + np.arange(w_len)[None, :]
            h, v = h2[idx], valid[idx]
            wv = np.where(v, w[None, :], dtype(0.0))
            a = wv.sum(axis=1)
            b = np.where(v, w[None, :] * h, dtype(0.0)).sum(axis=1)
            lhs, rhs = h * a[:, None], (b * guard)[:, None]
            inn = v & (lhs > rhs)
            cc = np.where(inn, wv, dtype(0.0)).sum(axis=1)
            near = v & (np.abs(lhs - rhs) <= eps * rhs)
            fin = np.isfinite(b)
            ok = fin & (b != 0)
            sl = slice(j0, j0 + c.size)
            eta[sl] = np.where(ok, (cc / a) / dtype(E), np.nan)
            kind[sl] = np.where(ok, 0, np.where(fin, 1, 2))
            amb[sl] = np.where(ok, np.where(near, wv, dtype(0.0)).sum(axis=1), 0)
            a_all[sl] = a
    return eta, kind, amb, a_all


def bound(eta, amb, a, delta):
    """|eta_dev - eta_ref| <= (2 W + 16) 2^-53 eta_ref + ambiguous_weight / (A E), plus one float32 ulp of eta_ref for the
    float32 profile (float64, NaN where eta is)."""
    w_len = 2 * delta + 1
    eta64 = np.asarray(eta, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ulp = np.spacing(np.abs(eta64.astype(np.float32))).astype(np.float64)
        return (2.0 * w_len + 16.0) * 2.0 ** -53 * eta64 + np.asarray(amb / (a * LD(E)), dtype=np.float64) + ulp


def record(prof32, thresholds, nan_silent=0x7fc00000, nan_nonfinite=0x7fc00001):
    """The 8-double record from a float32 profile as stored: K, the count of each NaN kind (told apart by the payload),
    the maximum of the other values and its first index, the first index at or above each threshold."""
    p = np.asarray(prof32, dtype=np.float32)
    bits = p.view(np.uint32)
    isn = np.isnan(p)
    rec = np.full(8, -1.0)
    rec[0] = p.size
    rec[2] = int(np.sum(isn & (bits == nan_nonfinite)))
    rec[1] = int(np.sum(isn)) - rec[2]
    val = np.where(isn, -np.inf, p.astype(np.float64))
    if np.any(~isn):
        rec[3], rec[4] = val.max(), int(np.argmax(val))
    else:
        rec[3] = np.nan
    for t, thr in enumerate(thresholds):
        hit = ~isn & (p.astype(np.float64) >= thr)
        if np.any(hit):
            rec[5 + t] = int(np.argmax(hit))
    return rec


# ------------------------------------------------------------------------------------------------ seeded inputs
def decaying_gaussian(n, seed=11, rt_samples=6000.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.exp(-np.arange(n) / rt_samples)).astype(np.float32)


def thickening_poisson(n, seed=12, start=0.02, growth=3.9):
    """A unit pulse at sample 0, then pulses of random sign and size whose rate grows from `start` per sample by a factor
    e^growth over the signal: sparse reflections that thicken into a dense tail."""
    rng = np.random.default_rng(seed)
    rate = np.minimum(1.0, start * np.exp(growth * np.arange(n) / n))
    x = np.where(rng.random(n) < rate, rng.standard_normal(n) * 0.3, 0.0)
    x[0] = 1.0
    return x.astype(np.float32)


def dc_offset(n, seed=13):
    rng = np.random.default_rng(seed)
    return (0.25 + 0.05 * rng.standard_normal(n)).astype(np.float32)


def tiny_values(n, seed=14):
    """Magnitudes from 1 down to float32 denormals, a -0.0 among them."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-44.0, 0.0, n)).astype(np.float32)
    x[0] = 1.0
    x[n // 2] = -0.0
    x[n // 2 + 1] = np.float32(1e-45)
    return x
