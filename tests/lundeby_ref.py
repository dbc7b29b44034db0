"""Reference for the Lundeby kernels (ira_lundeby.hip): a long-double NumPy restatement of the algorithm the docstring of
audio_analysis_amd/analyse/lundeby.py pins, written from that text and sharing no code with the module or the kernels
(imported by name, like decay_ref.py; tests/test_lundeby_cpu.py pins it on a machine without a GPU).

Besides the results, estimate() returns its DECISION MARGIN: the smallest distance, in dB, of any D[k] from a threshold it
was compared with (and of the runner-up from the maximum), and, in units of one interval m1 * B, the distance of every
rounded, floored or compared time from its boundary.  Integer outputs of a float64 implementation are only comparable
on inputs whose margins are large against float64 rounding (1e-6 dB, 1e-6 of an interval): a condition on the input.
"""
import math

import numpy as np

LD = np.longdouble
LONGDOUBLE_OK = bool(np.finfo(LD).eps < 2e-19)
TINY = 1e-300
MAX_BLOCKS = 4096
MIN_BLOCKS = 32
S_SILENT, S_SHORT, S_NO_RANGE, S_SLOPE, S_NON_FINITE, S_NO_FLOOR = 1, 2, 4, 8, 16, 32
MARGIN_DB = 1e-6
MARGIN_INTERVAL = 1e-6


def need_longdouble():
    import pytest
    if not LONGDOUBLE_OK:
        pytest.skip("np.longdouble has no 64-bit mantissa on this machine: no reference more precise than float64")


def block_size(fs, length):
    return max(-(-int(fs) // 1000), -(-int(length) // MAX_BLOCKS))


def first_interval(fs, b):
    return max(1, int(math.floor(0.030 * float(fs) / b + 0.5)))


def block_energies(y, b, dtype=LD):
    """(E[0 .. nb), energy of the partial tail block) of a row y (from its start index on)."""
    e = np.asarray(y, np.float32).astype(dtype) ** 2
    nb = e.size // b
    return e[: nb * b].reshape(nb, b).sum(axis=1), e[nb * b:].sum()


class _Margin:
    def __init__(self):
        self.db = math.inf
        self.interval = math.inf

    def level(self, d):
        d = np.abs(np.asarray(d, dtype=np.float64))
        if d.size:
            self.db = min(self.db, float(d.min()))

    def time(self, v):
        self.interval = min(self.interval, abs(float(v)))

    def ok(self):
        return self.db >= MARGIN_DB and self.interval >= MARGIN_INTERVAL


def _means(E, m, b):
    k = E.size // m
    M = E[: k * m].reshape(k, m).sum(axis=1) / LD(m * b)
    kmax = int(np.argmax(M))
    with np.errstate(all="ignore"):
        D = LD(10) * np.log10(np.maximum(M, LD(TINY)) / M[kmax])
    return M, D, kmax


def _level(mean, mmax):
    return LD(10) * np.log10(max(mean, LD(TINY)) / mmax)


def _first_below(D, start, thr, mg):
    """first k >= start with D[k] < thr (None if there is none); every compared level counts towards the margin"""
    hit = np.flatnonzero(D[start:] < thr)
    end = start + int(hit[0]) + 1 if hit.size else D.size
    mg.level(D[start:end] - thr)
    return start + int(hit[0]) if hit.size else None


def _line(D, k0, k1, mb):
    k = np.arange(k0, k1).astype(LD)
    t = (k + LD(0.5)) * LD(mb)
    d = D[k0:k1]
    n = LD(k1 - k0)
    tm, dm = t.sum() / n, d.sum() / n
    slope = ((t - tm) * (d - dm)).sum() / ((t - tm) ** 2).sum()
    return slope, dm - slope * tm


def estimate(y, fs, compensate=True, b=None):
    """The algorithm, steps 1 to 6, on a row y (float32, from its start index on).  Returns a dict: status, Ln, t1, slope (dB
    per sample), intercept, C, rounds, m1, kmax, k0, k1, widened (the last round lowered k0), clamped (m1 hit nb // 16), tx0, tx, mmax, B, nb, length (samples the curve covers), margin
    (_Margin).  On an error status (bits 1 to 16) only status, B, nb and margin are meaningful."""
    y = np.asarray(y, np.float32)
    L = int(y.size)
    b = int(b) if b else block_size(fs, L)
    nb = L // b
    mg = _Margin()
    out = dict(status=0, B=b, nb=nb, margin=mg, length=0)
    if nb < MIN_BLOCKS:
        out["status"] = S_SHORT
        return out
    E, tail = block_energies(y, b)
    if not (np.all(np.isfinite(E.astype(np.float64))) and np.isfinite(float(tail))):
        out["status"] = S_NON_FINITE
        return out
    if float(E.max()) == 0.0:
        out["status"] = S_SILENT
        return out
    # preliminary pass
    m0 = first_interval(fs, b)
    M, D, kmax = _means(E, m0, b)
    K = M.size
    mg.level(np.delete(D, kmax))
    Ln = _level(M[K - max(1, K // 10):].sum() / LD(max(1, K // 10)), M[kmax])
    kend = _first_below(D, kmax + 1, Ln + 10, mg)
    if kend is None or kend - kmax < 3:
        out["status"] = S_NO_RANGE
        return out
    slope, c = _line(D, kmax, kend, m0 * b)
    if not slope < 0:
        out["status"] = S_SLOPE
        return out
    tx0 = tx = (Ln - c) / slope
    # re-averaging
    want = (LD(-10) / slope) / LD(5) / LD(b)
    hi = max(1, nb // 16)
    w = min(float(want), 1e15)
    raw = math.floor(w + 0.5)
    m1 = int(min(max(raw, 1), hi))
    if raw < 1:
        mg.time((0.5 - w) / m1)
    elif raw > hi:
        mg.time((w - (hi + 0.5)) / m1)
    else:
        f = (w + 0.5) - raw
        mg.time(min(f, 1.0 - f) / m1)
    M, D, kmax = _means(E, m1, b)
    K = M.size
    mb = m1 * b
    mg.level(np.delete(D, kmax))
    rounds = 0
    k0 = k1 = 0
    widened = False
    for _ in range(5):
        rounds += 1
        start = min(tx + LD(-10) / slope, LD(0.9) * LD(nb * b))
        centres = (np.arange(K).astype(LD) + LD(0.5)) * LD(mb)
        mg.time(np.abs((centres - start).astype(np.float64)).min() / mb)
        kn = min(int(np.sum(centres < start)), K - 1)
        Ln = _level(M[kn:].sum() / LD(K - kn), M[kmax])
        k1 = _first_below(D, kmax + 1, Ln + 10, mg)
        if k1 is None:
            out["status"] = S_NO_RANGE
            return out
        hit = np.flatnonzero(D[kmax:k1] <= Ln + 30)
        mg.level(D[kmax:(kmax + int(hit[0]) + 1) if hit.size else k1] - (Ln + 30))
        k0 = kmax + int(hit[0]) if hit.size else k1
        widened = k0 > k1 - 3
        k0 = min(k0, k1 - 3)
        if k0 < kmax:
            out["status"] = S_NO_RANGE
            return out
        slope, c = _line(D, k0, k1, mb)
        if not slope < 0:
            out["status"] = S_SLOPE
            return out
        new = (Ln - c) / slope
        moved = abs(new - tx)
        tx = new
        mg.time((float(moved) - mb) / mb)
        if moved < mb:
            break
    status = 0
    mg.time(float(tx - nb * b) / mb)
    if tx >= nb * b:
        status |= S_NO_FLOOR
        t1, C, length = nb * b, LD(0), L
    else:
        q = math.floor(float(tx / b))
        mg.time(float(tx / b - q) * b / mb)
        mg.time(float(q + 1 - tx / b) * b / mb)
        t1 = min(max(q * b, b), nb * b)
        lev = M[kmax] * LD(10) ** ((c + slope * t1) / LD(10))
        C = lev * LD(10) / (-slope * LD(np.log(LD(10)))) if compensate else LD(0)
        length = t1
    if not all(np.isfinite(float(v)) for v in (Ln, slope, c, C, tx)):
        out["status"] = S_NON_FINITE
        return out
    out.update(status=status, Ln=Ln, t1=int(t1), slope=slope, intercept=c, C=C, rounds=rounds, m1=m1, kmax=kmax, k0=int(k0),
               k1=int(k1), widened=bool(widened), clamped=bool(raw > hi), tx0=tx0, tx=tx, mmax=M[kmax], length=int(length))
    return out


def curve(y, length, C, eps, floor_db, dtype=LD):
    """Step 6's curve over y[:length] with compensation energy C: (float64 dB before the floor, float32 dB).  dtype =
    np.float64 restates it in plain float64 (to measure how often the two precisions give the same float32)."""
    e = np.asarray(y, np.float32)[:length].astype(dtype) ** 2
    with np.errstate(all="ignore"):
        v = np.maximum(np.cumsum(e[::-1])[::-1] + dtype(C), dtype(eps))
        db = (dtype(10) * np.log10(v / v[0])).astype(np.float64)
        return db, np.maximum(db, float(floor_db)).astype(np.float32)


def curve_bound_db(y, length, C, eps):
    """The allowance decay_ref.py states for ira_edc_db's curve (comparison A), for this curve: a float64 sum of at most
    `length` + 2 non-negative terms (the samples, the block suffix, C) in numerator and denominator, and 4 ulps of
    max(1, |log2|) for each of the kernel's two table logarithms."""
    e = np.asarray(y, np.float32)[:length].astype(LD) ** 2
    v = np.maximum(np.cumsum(e[::-1])[::-1] + LD(C), LD(eps))
    with np.errstate(all="ignore"):
        l2 = np.abs(np.log2(v)).astype(np.float64)
    u52 = 2.0 ** -52
    return (10.0 / np.log(10.0)) * (length + 2) * u52 + 3.0102999566398120 * 4.0 * u52 * (np.maximum(1.0, l2) + max(1.0, float(l2[0])))


def decaying_noise(fs, seconds, rt, noise_db, seed, fade=0.0):
    """Gaussian noise with an exponential envelope of reverberation time rt (60 dB in rt seconds) plus stationary Gaussian
    noise noise_db below the start of the decay (None: no floor); fade > 0: a linear fade to zero over that last fraction."""
    rng = np.random.default_rng(seed)
    n = int(round(fs * seconds))
    t = np.arange(n) / float(fs)
    x = rng.standard_normal(n) * 10.0 ** (-3.0 * t / rt)
    if noise_db is not None:
        x = x + rng.standard_normal(n) * 10.0 ** (noise_db / 20.0)
    if fade > 0.0:
        k = int(round(n * fade))
        x[n - k:] *= np.linspace(1.0, 0.0, k)
    return (0.5 * x).astype(np.float32)


def two_slope_noise(fs, seconds, rt_early, t_break, rt_late, noise_db, seed):
    """Gaussian noise whose envelope decays with rt_early up to t_break seconds and with rt_late after it, plus a stationary
    floor: a late decay much steeper than the preliminary line (whose slope sizes the intervals) is what leaves fewer than
    three intervals between Ln + 30 and Ln + 10."""
    rng = np.random.default_rng(seed)
    n = int(round(fs * seconds))
    t = np.arange(n) / float(fs)
    env_db = np.where(t < t_break, -60.0 * t / rt_early, -60.0 * t_break / rt_early - 60.0 * (t - t_break) / rt_late)
    x = rng.standard_normal(n) * 10.0 ** (env_db / 20.0) + rng.standard_normal(n) * 10.0 ** (noise_db / 20.0)
    return (0.5 * x).astype(np.float32)


def after_peak(x, length):
    """x cut so that exactly `length` samples remain from its first maximum of |x| on."""
    x = np.asarray(x, np.float32)
    p = int(np.argmax(np.abs(x)))
    assert p + length <= x.size
    return x[: p + length]
