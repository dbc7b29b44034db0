"""
A long-double restatement of the modulation transfer sums and of the STI arithmetic pinned in the docstring of
audio_analysis_amd/analyse/sti.py, written from the definitions and sharing no code with the module.  Helper module, like
decay_ref.py / lundeby_ref.py: it holds no tests.

The phase is reduced in long double: w is the float64 the host formed, w * n is exact to 2^-64 relative in long double
(64-bit significand), the whole turns are removed before cos / sin are taken.
"""
import math

import numpy as np

LD = np.longdouble
PI_LD = LD(4) * np.arctan(LD(1))

FREQS = (0.63, 0.8, 1.0, 1.25, 1.6, 2.0, 2.5, 3.15, 4.0, 5.0, 6.3, 8.0, 10.0, 12.5)
ALPHA = (0.085, 0.127, 0.230, 0.233, 0.309, 0.224, 0.173)
BETA = (0.085, 0.078, 0.065, 0.011, 0.047, 0.095)
A_RT = (46.0, 27.0, 12.0, 6.5, 7.5, 8.0, 12.0)


def turns(freqs, fs):
    return [float(f) / float(fs) for f in freqs]


def cis(w, n):
    """(cos, sin) of 2 pi frac(w n) in long double for the float64 w and the integers n."""
    ph = LD(float(w)) * np.asarray(n, dtype=LD)
    ang = (LD(2) * PI_LD) * (ph - np.rint(ph))
    return np.cos(ang), np.sin(ang)


def sums(x, w, block=2048):
    """E, A_0, B_0, ... (long double) of one float32 row for the float64 turns-per-sample w.  Sample n = block a + b takes the
    phasor cis(w block a) cis(w b), both factors evaluated directly from a reduced phase (their product is exact to a few
    2^-64): a row of 2^21 samples costs 3072 evaluations per frequency instead of 2^21."""
    x = np.asarray(x, dtype=np.float32)
    nb = max(1, -(-x.size // block))
    e = np.zeros(nb * block, dtype=LD)
    e[: x.size] = x.astype(LD) ** 2
    e = e.reshape(nb, block)
    out = [np.sum(e)]
    for wi in w:
        ca, sa = cis(wi, block * np.arange(nb))
        cb, sb = cis(wi, np.arange(block))
        ec, es = e @ cb, e @ sb
        out += [np.sum(ca * ec - sa * es), np.sum(sa * ec + ca * es)]
    return np.array(out, dtype=LD)


def m_of(s):
    s = np.asarray(s, dtype=LD)
    return (np.hypot(s[1::2], s[2::2]) / s[0]).astype(np.float64)


def mtf(x, w):
    return m_of(sums(x, w))


def masking_db(level):
    if level < 63.0:
        return 0.5 * level - 65.0
    if level < 67.0:
        return 1.8 * level - 146.9
    if level < 100.0:
        return 0.5 * level - 59.8
    return -10.0


def adjust(m, snr_db=None, levels_db=None):
    """m (7, nf): noise factor first, level factor second."""
    m = np.array(m, dtype=np.float64)
    for k in range(7):
        if snr_db is not None:
            s = snr_db[k] if np.ndim(snr_db) else snr_db
            m[k] = m[k] / (1.0 + 10.0 ** (-float(s) / 10.0))
        if levels_db is not None:
            i_k = 10.0 ** (levels_db[k] / 10.0)
            i_am = 0.0 if k == 0 else 10.0 ** (levels_db[k - 1] / 10.0) * 10.0 ** (masking_db(levels_db[k - 1]) / 10.0)
            i_rt = 10.0 ** (A_RT[k] / 10.0)
            m[k] = m[k] * i_k / (i_k + i_am + i_rt)
    return m


def ti(m):
    if m >= 1.0:
        snr = 15.0
    elif m <= 0.0:
        snr = -15.0
    else:
        snr = min(15.0, max(-15.0, 10.0 * math.log10(m / (1.0 - m))))
    return (snr + 15.0) / 30.0


def sti(m):
    """(STI, [MTI_k]) of m (7, nf)."""
    mti = [sum(ti(float(v)) for v in row) / len(row) for row in m]
    s = sum(a * v for a, v in zip(ALPHA, mti)) - sum(b * math.sqrt(mti[k] * mti[k + 1]) for k, b in enumerate(BETA))
    return s, mti


def schroeder_m(f_hz, t_seconds):
    """m(F) of an ideal exponential decay with reverberation time T."""
    return 1.0 / math.sqrt(1.0 + (2.0 * math.pi * f_hz * t_seconds / 13.8155) ** 2)


def schroeder_sti(t_seconds, freqs=FREQS):
    return sti([[schroeder_m(f, t_seconds) for f in freqs]] * 7)[0]


def decaying_noise(seed, t_seconds, seconds, fs):
    """Gaussian noise whose ENERGY decays by 60 dB in t_seconds (amplitude exp(-6.90776 t / T)), float32."""
    n = int(round(seconds * fs))
    g = np.random.default_rng(seed).standard_normal(n)
    return (g * np.exp(-(13.8155 / 2.0) * np.arange(n) / (fs * t_seconds))).astype(np.float32)


def geometric_row(stride, count, a=0.25):
    """x[stride j] = sqrt(a^j), j < count, zero elsewhere, and a.  With a = 0.25 every sample is a power of two, so the float32
    row's squares are a^j exactly and the closed form below holds to rounding (stride 1 is the plain row x[n] = sqrt(a^n))."""
    x = np.zeros(stride * (count - 1) + 1, np.float32)
    x[::stride] = np.sqrt(np.float64(a) ** np.arange(count))
    return x, a


def geometric_m(a, stride, count, w):
    """|(1 - z^J) / (1 - z)| / sum_j a^j with z = a e^(-j 2 pi w stride): m of geometric_row."""
    out = []
    for wi in w:
        ph = float(LD(float(wi)) * LD(stride) % LD(1))
        z = a * np.exp(-2j * np.pi * ph)
        out.append(abs((1.0 - z ** count) / (1.0 - z)) / ((1.0 - a ** count) / (1.0 - a)))
    return np.array(out)


def oracle_band_signals(x, sr):
    """[(name, float32 band signal)]: the oracle's float64 filter bank for the STI bands, rounded to float32."""
    from oracle import ira_oracle as O
    x = np.asarray(x, dtype=np.float32)
    n = x.size
    f = np.fft.rfftfreq(n, d=1.0 / float(sr)).astype(np.float32)
    spec = np.fft.rfft(x.astype(np.float64))
    out = []
    for b in O.band_definitions(sr, band_mode="octave", f_min_hz=125.0, f_max_hz=8000.0):
        m = O.band_mask(f, b, 1.0 / 6.0, 0.5 * float(sr))
        out.append((b["name"], np.fft.irfft(spec * m.astype(np.float64), n=n).astype(np.float32)))
    return out
