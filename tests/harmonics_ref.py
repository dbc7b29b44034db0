"""
Float64 NumPy restatement of the harmonic distortion measure (audio_analysis_amd.analyse.harmonics), a float64
deconvolution with numpy.fft, and the builder of the test signals.  Helper module, like sti_ref.py / decay_ref.py: it holds
no tests.  Everything here is written from the definitions, one formula per function, and shares no code with the package.

The measure, for a circular float32 response h of n_fft samples at sample rate fs (steps as the module docstring numbers them):
  lags      L = T / ln(f2 / f1), d_k = floor(L fs ln k + 0.5), k = 1 .. K
  peak      p = first maximum of |h| over [0, n_search), n_search = n_fft - ceil(L fs ln(K + 1)) - guard
  window    W = min(floor(window_ms fs / 1000), floor(L fs ln(K / (K - 1))) - guard), seg = guard + W, n_h = 2^ceil(log2 seg)
  segments  s_k[i] = float32(float64(h[(p - d_k - guard + i) mod n_fft]) * w[i])
  spectra   rfft of s_k zero-padded to n_h
  powers    E_k(j) = mean |S_k|^2 over the bins of [k f_j 2^(-1/(2P)), k f_j 2^(1/(2P))], f_j = f1 2^(j / P)
  results   HD_k = sqrt(E_k / E_1), THD = sqrt(sum_k>=2 E_k / E_1), fundamental 10 log10 E_1
"""
import math

import numpy as np

STATUS_SILENT, STATUS_TOO_SHORT, STATUS_NON_FINITE = 1, 2, 4
MIN_WINDOW = 64


def sweep_rate(T, f1, f2):
    return T / math.log(f2 / f1)


def lags(T, f1, f2, fs, K):
    L = sweep_rate(T, f1, f2)
    return np.array([math.floor(L * fs * math.log(k) + 0.5) for k in range(1, K + 1)], dtype=np.int64)


def search_length(n_fft, T, f1, f2, fs, K, guard):
    return int(n_fft) - math.ceil(sweep_rate(T, f1, f2) * fs * math.log(K + 1)) - int(guard)


def window_length(T, f1, f2, fs, K, guard, window_ms):
    return min(math.floor(window_ms * fs / 1000.0), math.floor(sweep_rate(T, f1, f2) * fs * math.log(K / (K - 1))) - guard)


def fft_size(seg):
    n = 1
    while n < seg:
        n *= 2
    return n


def window(guard, W, fade_fraction):
    seg = guard + W
    nfade = math.floor(fade_fraction * W)
    w = np.ones(seg, dtype=np.float64)
    for i in range(guard):
        w[i] = 0.5 - 0.5 * math.cos(math.pi * (i + 0.5) / guard)
    for m in range(nfade):
        w[seg - nfade + m] = 0.5 + 0.5 * math.cos(math.pi * (m + 0.5) / nfade)
    return w


def linear_peak(h, n_search):
    return int(np.argmax(np.abs(np.asarray(h)[:n_search])))          # argmax returns the first maximum


def segments(h, p, d, guard, w):
    """(K, seg) float32: one float64 multiply, then one rounding."""
    h = np.asarray(h, dtype=np.float32)
    n = h.size
    i = np.arange(w.size, dtype=np.int64)
    rows = []
    for dk in d:
        idx = (int(p) - int(dk) - int(guard) + i) % n
        rows.append((h[idx].astype(np.float64) * w).astype(np.float32))
    return np.stack(rows)


def spectra(rows, n_h):
    return np.fft.rfft(np.asarray(rows, dtype=np.float32).astype(np.float64), n=n_h, axis=-1)


def grid(f1, f2, P):
    J = math.floor(P * math.log2(f2 / f1))
    return np.array([f1 * 2.0 ** (j / P) for j in range(J + 1)], dtype=np.float64)


def tables(f1, f2, fs, K, P, n_h):
    """(f (J,), lo (K, J), cnt (K, J)): the bins lo .. lo + cnt - 1 of harmonic k at grid point j; cnt = 0 where invalid."""
    f = grid(f1, f2, P)
    df = fs / n_h
    up, dn = 2.0 ** (1.0 / (2 * P)), 2.0 ** (-1.0 / (2 * P))
    top = min(f2, fs / 2.0)
    lo = np.zeros((K, f.size), dtype=np.int32)
    cnt = np.zeros((K, f.size), dtype=np.int32)
    for k in range(1, K + 1):
        for j, fj in enumerate(f):
            c = k * fj
            if c * up > top:
                continue
            a, b = math.ceil(c * dn / df), math.floor(c * up / df)
            if b < a:
                a = b = math.floor(c / df + 0.5)
            a, b = min(a, n_h // 2), min(b, n_h // 2)
            lo[k - 1, j], cnt[k - 1, j] = a, b - a + 1
    return f, lo, cnt


def band_powers(spec, lo, cnt):
    """(K, J) float64 mean of re^2 + im^2 over each band of the (K, bins) spectra; 0 where cnt = 0.  The squares and the sum
    are formed in long double (64-bit significand on x86), so that this side's own rounding (one to float64 at the end)
    is far below the (cnt + 4) 2^-53 the tests allow the device's float64 sums."""
    spec = np.asarray(spec)
    re, im = spec.real.astype(np.longdouble), spec.imag.astype(np.longdouble)
    pw = re * re + im * im
    out = np.zeros(lo.shape, dtype=np.float64)
    for k in range(lo.shape[0]):
        for j in range(lo.shape[1]):
            if cnt[k, j]:
                out[k, j] = float(np.sum(pw[k, lo[k, j] : lo[k, j] + cnt[k, j]]) / np.longdouble(int(cnt[k, j])))
    return out


def results(E, cnt):
    """(hd (K - 1, J), thd (J,), counted (J,), fundamental_db (J,)) from the mean powers and the validity table."""
    K, J = E.shape
    nan = float("nan")
    hd = np.full((K - 1, J), nan)
    thd = np.full(J, nan)
    counted = np.zeros(J, dtype=np.int64)
    fund = np.full(J, nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(J):
            if cnt[0, j]:
                fund[j] = 10.0 * np.log10(E[0, j])
            tot = 0.0
            for k in range(2, K + 1):
                if cnt[k - 1, j]:
                    hd[k - 2, j] = np.sqrt(E[k - 1, j] / E[0, j])
                    tot += E[k - 1, j]
                    counted[j] += 1
            if cnt[1, j]:
                thd[j] = np.sqrt(tot / E[0, j])
    return hd, thd, counted, fund


def analyse(h, fs, T=10.0, f1=20.0, f2=20000.0, K=5, P=3, window_ms=200.0, guard=64, fade_fraction=0.25):
    """The whole measure on one float32 response.  dict: status, p, W, seg, n_h, d, w, f, lo, cnt, rows, spec, E, hd, thd,
    counted, fund (what does not exist for the status is absent)."""
    h = np.asarray(h, dtype=np.float32)
    n_fft = h.size
    n_search = search_length(n_fft, T, f1, f2, fs, K, guard)
    W = window_length(T, f1, f2, fs, K, guard, window_ms)
    out = dict(status=0, n_search=n_search, W=W)
    if n_search < 1 or W < MIN_WINDOW:
        out["status"] = STATUS_TOO_SHORT
        return out
    d = lags(T, f1, f2, fs, K)
    p = linear_peak(h, n_search)
    seg = guard + W
    n_h = fft_size(seg)
    w = window(guard, W, fade_fraction)
    f, lo, cnt = tables(f1, f2, fs, K, P, n_h)
    out.update(p=p, seg=seg, n_h=n_h, d=d, w=w, f=f, lo=lo, cnt=cnt)
    if h[p] == 0.0:
        out["status"] = STATUS_SILENT
        return out
    rows = segments(h, p, d, guard, w)
    spec = spectra(rows, n_h)
    E = band_powers(spec, lo, cnt)
    out.update(rows=rows, spec=spec, E=E)
    if not math.isfinite(float(np.sum(E[0]))):
        out["status"] = STATUS_NON_FINITE
        return out
    hd, thd, counted, fund = results(E, cnt)
    out.update(hd=hd, thd=thd, counted=counted, fund=fund)
    return out


def deconvolve(y, x, regularization_relative=1e-10):
    """float64 circular response of n_fft = next power of two >= max(len) samples: H = Y conj(X) / (|X|^2 + eps),
    eps = regularization_relative * max |X|^2."""
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    n_fft = fft_size(max(y.size, x.size))
    X = np.fft.rfft(x, n=n_fft)
    Y = np.fft.rfft(y, n=n_fft)
    p = X.real ** 2 + X.imag ** 2
    return np.fft.irfft(Y * np.conj(X) / (p + regularization_relative * p.max()), n=n_fft)


def test_signal(fs, T, f1, f2, A, tail_seconds, c2, c3, mute=True):
    """(sweep, recording), float32.  Phase theta(t) = 2 pi f1 L (exp(t / L) - 1); envelope e: half-cosine fades of 10 ms at
    both ends; sweep x = A e sin(theta), silence appended; recording y = x - c2 A e m_2 cos(2 theta) - c3 A e m_3 sin(3 theta),
    m_k = 0.5 + 0.5 cos(pi clip((k f_inst - 0.8 f2) / (0.2 f2), 0, 1)), f_inst = f1 exp(t / L) (m_k = 1 without mute: the
    harmonics then run past f2, where the regularised inverse filter amplifies them)."""
    n = int(round(T * fs))
    t = np.arange(n, dtype=np.float64) / fs
    L = sweep_rate(T, f1, f2)
    theta = 2.0 * math.pi * f1 * L * (np.exp(t / L) - 1.0)
    e = np.ones(n)
    nf = int(round(0.010 * fs))
    ramp = 0.5 - 0.5 * np.cos(math.pi * (np.arange(nf) + 0.5) / nf)
    e[:nf] = ramp
    e[n - nf:] = ramp[::-1]
    f_inst = f1 * np.exp(t / L)

    def m(k):
        if not mute:
            return 1.0
        return 0.5 + 0.5 * np.cos(math.pi * np.clip((k * f_inst - 0.8 * f2) / (0.2 * f2), 0.0, 1.0))

    x = A * e * np.sin(theta)
    y = x - c2 * A * e * m(2) * np.cos(2.0 * theta) - c3 * A * e * m(3) * np.sin(3.0 * theta)
    tail = np.zeros(int(round(tail_seconds * fs)))
    return np.concatenate([x, tail]).astype(np.float32), np.concatenate([y, tail]).astype(np.float32)


test_signal.__test__ = False          # a builder, not a test (pytest collects by name)


def flat_range(f, k, f2, P, low_hz=800.0):
    """Grid points from low_hz up to 0.8 f2 / (k 2^(1/(2P))): where HD_k of the test signal equals c_k."""
    f = np.asarray(f)
    return (f >= low_hz) & (f <= 0.8 * f2 / (k * 2.0 ** (1.0 / (2 * P))))
