"""Reference for the echo-criterion kernels (ira_echo.hip): a float64 NumPy restatement (np.power, np.cumsum) of the
definition the docstring of audio_analysis_amd/analyse/echo.py pins, written from that text and sharing no code with the
module or the kernels (imported by name, like lundeby_ref.py; tests/test_echo_ref_cpu.py holds it to closed forms on a
machine without a GPU).  Besides the values it gives the tolerance the GPU tests compare with and an interval version
of the same arithmetic for inputs known only to within +-delta per sample."""
import math

import numpy as np


def onset(x, onset_db=-20.0):
    x = np.asarray(x, dtype=np.float32)
    e = x.astype(np.float64) ** 2
    p = int(np.argmax(np.abs(x)))
    return int(np.flatnonzero(e[: p + 1] >= e[p] * 10.0 ** (onset_db / 10.0))[0])


def lag(window_ms, fs):
    return max(1, int(math.floor(window_ms * fs / 1000.0 + 0.5)))


def guard(end_guard_ms, fs):
    return int(math.ceil(end_guard_ms * fs / 1000.0))


def mmax(max_tau_ms, fs):
    return None if max_tau_ms is None else 1 + int(math.ceil(max_tau_ms * fs / 1000.0))


def eval_len(n_samples, o, fs, end_guard_ms=50.0, max_tau_ms=1000.0):
    """M = min(L - G, Mmax)."""
    m = (n_samples - o) - guard(end_guard_ms, fs)
    cap = mmax(max_tau_ms, fs)
    return m if cap is None else min(m, cap)


def power(y, n):
    a = np.abs(np.asarray(y, dtype=np.float32).astype(np.float64))
    s = np.power(a, n)
    s[a == 0.0] = 0.0
    return s


def centre_time(s, fs):
    """ts[m] = V[m] / (fs W[m]), 0 where W[m] == 0; also W and V."""
    w = np.cumsum(s)
    v = np.cumsum(np.arange(s.size, dtype=np.float64) * s)
    with np.errstate(divide="ignore", invalid="ignore"):
        ts = np.where(w == 0.0, 0.0, v / (fs * w))
    return ts, w, v


def lagged(ts, d, fs, m):
    prev = np.concatenate([np.zeros(min(d, m)), ts[: max(m - d, 0)]])
    return (ts[:m] - prev) / (d / fs)


def ek_curve(y, o, n, d, fs, m):
    """(EK[0 .. m), ts[0 .. m), W, V) of the signal y from its onset o on.  Only y[o : o + m] enters: the sums are causal."""
    s = power(np.asarray(y)[o : o + m], n)
    ts, w, v = centre_time(s, fs)
    return lagged(ts, d, fs, m), ts, w, v


def tolerance(m, ts, d, fs):
    """tol = (8 M + 100) 2^-53 max(ts) / (D / fs): worst-case rounding of two sums of M non-negative terms on each side,
    through the ratio and the lagged difference, plus 16 ulp for pow."""
    return (8.0 * m + 100.0) * 2.0 ** -53 * float(np.max(ts)) / (d / fs)


def first_at_or_above(ek, thr):
    hit = np.flatnonzero(ek >= thr)
    return int(hit[0]) if hit.size else -1


def step_max(ek, step):
    """float32 of max EK[k S .. min((k + 1) S, M) - 1] per step k."""
    m = ek.size
    k = -(-m // step)
    pad = np.full(k * step, -np.inf)
    pad[:m] = ek
    return pad.reshape(k, step).max(axis=1).astype(np.float32)


def rating(ek_max, thr10, thr50):
    return "audible" if ek_max >= thr50 else ("marginal" if ek_max >= thr10 else "inaudible")


def ek_interval(y, delta, o, n, d, fs, m):
    """(lower, upper) bounds of EK[0 .. m) when every sample of y may be off by delta: s between max(|y| - delta, 0)^n and
    (|y| + delta)^n, ts between V_lo / W_hi and V_hi / W_lo, EK between the crossed differences."""
    a = np.abs(np.asarray(y, dtype=np.float64)[o : o + m])
    s_lo, s_hi = np.power(np.maximum(a - delta, 0.0), n), np.power(a + delta, n)
    idx = np.arange(m, dtype=np.float64)
    w_lo, w_hi = np.cumsum(s_lo), np.cumsum(s_hi)
    v_lo, v_hi = np.cumsum(idx * s_lo), np.cumsum(idx * s_hi)
    with np.errstate(divide="ignore", invalid="ignore"):
        ts_lo = np.where(w_hi == 0.0, 0.0, v_lo / (fs * w_hi))
        ts_hi = np.where(w_lo == 0.0, np.inf, v_hi / (fs * w_lo))
    return ((ts_lo - np.concatenate([np.zeros(min(d, m)), ts_hi[: max(m - d, 0)]])) / (d / fs),
            (ts_hi - np.concatenate([np.zeros(min(d, m)), ts_lo[: max(m - d, 0)]])) / (d / fs))
