"""
Restatement of the equalisation chain (audio_analysis_amd/analyse/equalise.py, include/ira_equalise.h) in NumPy float64, for
the tests: nothing of the package is used.  Helper module, like minphase_ref.py: it holds no tests.

What is here
  * every line of the module's docstring: pyramid / query (the window sum W), windows, power, smooth, grid_bins,
    reference_level, tables (t, beta), correction, taper, arithmetic (the curves); design() runs them in order from spectra.
    The device kernels are held to these BIT FOR BIT: every operation is one float64 operation in the same order.
  * filter_chain(c, n): the float64 restatement of the filter, minphase_ref.chain's steps on the complex (c, 0);
  * the bounds, derived here.

Bounds (u = 2^-53).
  window sum   W(lo, hi) adds at most 2 log2 N non-negative pyramid entries, each itself a pairwise sum of depth <= log2 N
       of non-negative terms.  Non-negative terms: every addition moves the running value by at most u relative, and the
       relative errors compound without cancellation: an entry of level j is off by at most j u, the two chains left and
       right add at most log2 N more each, the last addition one: (2 log2 N + 1) u relative, to first order.  math.fsum (the
       exact sum rounded once) adds u: WINDOW_ULPS(N) = 2 log2 N + 2.
  filter       FilterBounds: minphase_ref.Bounds with E_X = 0 (the chain's input c is the very array both sides are given,
       so neither the transform's error nor the floor's enters; floor_db = -300 never engages for c within 10^-15 of
       its maximum).  Per sample of g, Bounds.response; the taper multiplies by v[n] in float64 (u relative) and rounds to
       float32 once more:  v[n] resp[n] + 2^-24 (|f[n]| + v[n] resp[n]) + 2^-149.
  c against NumPy's own X   ln c is a function of ln s with slope in (-1, 0.5) (c = (sqrt(s) t + beta) / (s + beta):
       d ln c / d ln s = 0.5 a t / (a t + beta) - s / (s + beta)), so |d ln c_k| <= |d ln s_k| <= |d ln S_k| + |d ln ref|.
       A bin of a member's spectrum moves by at most E_X (longfft_ref.forward_bound, rigorous), its power by 2 |X| E_X +
       E_X^2.  Over a window of W bins (and the members of a row, whose mean is one more such average):
           |dS_k| <= (2 E_X / W) sum |X_j| + E_X^2 <= 2 E_X sqrt(S_k) + E_X^2     (Cauchy-Schwarz: sum |X_j| <= sqrt(W sum |X_j|^2))
       so |d ln S_k| <= 2 E_X / |X|_window,k with |X|_window,k = sqrt(S_k) the rms magnitude over the window -- the windowed
       form; b = 0 is its one-bin case, 2 E_X / |X_k|.  ln ref is the mean of ln S over the in-band grid points:
       |d ln ref| <= 2 E_X / min_grid |X|_window.  Together
           |d ln c_k| <= 2 E_X (1 / |X|_window,k + 1 / min_grid |X|_window)
       and the second order (E_X^2 / S, below 2^-40 of the first at the shapes tested) and the float64 rounding of the
       chain from X to c (a few hundred u) are allowed as a factor 1 + 2^-16 and 2^-40: log_c_bound.
  f against a c that moved   input_term, derived in its docstring: used where the device's filter is held to a closed form
       or to the restatement fed with NumPy's own X.
  closed forms  x = 0.5^n truncated at D = 64: X_k = (1 - 2^-64 z^-64) / (1 - 0.5 z^-1), the truncation moves |X| and so c
       by 2^-64 relative; beta = 10^-30 moves c by less than 10^-29.  f / sqrt(ref) = delta[n] - 0.5 delta[n - 1] up to the
       float64 rounding of four N-point transforms: each output is a sum of N products of magnitude <= 2 (|G| <= ln 2 + |ln
       ref| / 2, |M| <= 2 sqrt(ref) / ... all of order one here), off by at most N u times that in the worst case:
           CLOSED_BOUND(N) = 8 N u + 2^-60          (2.3e-13 at N = 256; the float64 chain gives 1e-16)
       The cepstral aliasing of a zero at radius 0.5 is 2 * 0.5^(N/2) / (N/2): 2^-134 at N = 256.
"""
import math

import numpy as np

import longfft_ref as L
import minphase_ref as MR

U = 2.0 ** -53


def window_ulps(n_fft):
    return 2.0 * math.log2(n_fft) + 2.0


def closed_bound(n_fft):
    return 8.0 * n_fft * U + 2.0 ** -60


# ================================================================================================ the smoothing
def layout(n_fft):
    """(offsets, lengths) of a row's levels: n_0 = N/2 + 1, n_(j+1) = ceil(n_j / 2) until 1."""
    lens = [n_fft // 2 + 1]
    while lens[-1] > 1:
        lens.append((lens[-1] + 1) // 2)
    off = [0]
    for n in lens[:-1]:
        off.append(off[-1] + n)
    return np.array(off, dtype=np.int64), np.array(lens, dtype=np.int64)


def pyramid(p):
    """The levels of P: pairwise sums, an entry without a partner copied."""
    lv = [np.asarray(p, dtype=np.float64)]
    while lv[-1].size > 1:
        a = lv[-1]
        b = a[0::2].copy()
        odd = a[1::2]
        b[: odd.size] = b[: odd.size] + odd
        lv.append(b)
    return lv


def flat_pyramid(p):
    return np.concatenate(pyramid(p))


def query(lv, lo, hi):
    """W(lo, hi) for arrays of window edges."""
    l = np.asarray(lo, dtype=np.int64).copy()
    r = np.asarray(hi, dtype=np.int64) + 1
    left, right = np.zeros(l.size), np.zeros(l.size)
    for a in lv:
        live = l < r
        if not live.any():
            break
        m = live & ((l & 1) == 1)
        left[m] = left[m] + a[l[m]]
        l[m] += 1
        m = live & ((r & 1) == 1)
        r[m] -= 1
        right[m] = right[m] + a[r[m]]
        l >>= 1
        r >>= 1
    return left + right


def windows(n_fft, b):
    k = np.arange(n_fft // 2 + 1, dtype=np.float64)
    if b == 0:
        return k.astype(np.int32), k.astype(np.int32)
    lo = np.ceil(k * 2.0 ** (-1.0 / (2.0 * b)))
    hi = np.minimum(np.floor(k * 2.0 ** (1.0 / (2.0 * b))), float(n_fft // 2))
    return lo.astype(np.int32), hi.astype(np.int32)


def power(specs, second=None):
    """P of one row from its members' spectra (complex128 arrays), ascending from 0.0; times |F|^2 with `second`."""
    p = np.zeros(specs[0].size)
    for x in specs:
        p = p + (x.real * x.real + x.imag * x.imag)
    p = p / float(len(specs))
    if second is not None:
        p = p * (second.real * second.real + second.imag * second.imag)
    return p


def smooth(p, lo, hi):
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    with np.errstate(all="ignore"):
        return query(pyramid(p), lo, hi) / (hi - lo + 1).astype(np.float64)


# ================================================================================================ the inversion
def grid(fs, points_per_octave=48, f_min=20.0, f_max=20000.0):
    top = min(f_max, fs / 2.0)
    count = int(np.floor(np.log2(top / f_min) * points_per_octave)) + 2
    f = f_min * 2.0 ** (np.arange(count, dtype=np.float64) / float(points_per_octave))
    return f[f <= top]


def grid_bins(f, n_fft, fs):
    return np.clip(np.rint(f * float(n_fft) / fs), 1, n_fft // 2 - 1).astype(np.int64)


def reference_level(s_grid, in_band):
    s = np.asarray(s_grid, dtype=np.float64)[in_band]
    if s.size == 0:
        return float("nan")
    with np.errstate(all="ignore"):
        return float(np.exp(np.mean(np.log(s))))


def valid(ref):
    return bool(ref > 0.0 and np.isfinite(ref))


def tables(n_fft, fs, f_low=40.0, f_high=16000.0, transition=0.5, reg_in=-20.0, reg_out=20.0, tilt=0.0):
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * fs / float(n_fft)
    f[0] = f[1]
    t = 10.0 ** (tilt * np.log2(f / 1000.0) / 20.0)
    u = np.where(f < f_low, np.clip(np.log2(f_low / f) / transition, 0.0, 1.0), np.clip(np.log2(f / f_high) / transition, 0.0, 1.0))
    w = 0.5 * (1.0 - np.cos(np.pi * u))
    w[0] = 1.0
    return t, 10.0 ** ((reg_in + w * (reg_out - reg_in)) / 10.0)


def correction(s_k, ref, t, beta, max_gain):
    """(c, clamped count); a row without values: c = 1, count 0."""
    if not valid(ref):
        return np.ones(np.size(s_k)), 0
    with np.errstate(all="ignore"):
        s = np.asarray(s_k, dtype=np.float64) / ref
        a = np.sqrt(s)
        c = (a * t + beta) / (s + beta)
    over = c > max_gain
    return np.where(over, max_gain, c), int(np.count_nonzero(over))


def taper(taps, fade=0.25):
    n0 = taps - int(np.rint(fade * taps))
    v = np.ones(taps)
    n = np.arange(n0, taps, dtype=np.float64)
    v[n0:] = 0.5 * (1.0 + np.cos(np.pi * (n - n0 + 1.0) / float(taps - n0 + 1)))
    return v


def apply_taper(g32, v):
    """f = float32((double)g v) from the float32 g."""
    return (np.asarray(g32, dtype=np.float32)[: v.size].astype(np.float64) * v).astype(np.float32)


def arithmetic(s_grid, c_grid, a_grid, t_grid, bins, in_band, n_fft, ref, clamped, fs):
    """The curves and row values of the module's docstring."""
    k = np.asarray(bins, dtype=np.int64)
    out = dict(frequencies_hz=k.astype(np.float64) * fs / float(n_fft), bin=k, target_db=20.0 * np.log10(t_grid))
    nan = np.full(k.size, np.nan)
    if not valid(ref):
        out.update(before_db=nan, correction_db=nan, after_db=nan, reference_level_db=math.nan, clamped_share=math.nan,
                   deviation_before_db=math.nan, deviation_after_db=math.nan)
        return out
    with np.errstate(all="ignore"):
        before = 10.0 * np.log10(s_grid / ref)
        after = 10.0 * np.log10(a_grid / ref)
        out.update(before_db=before, after_db=after, correction_db=20.0 * np.log10(c_grid),
                   reference_level_db=10.0 * math.log10(ref), clamped_share=float(clamped) / float(n_fft // 2 + 1),
                   deviation_before_db=float(np.sqrt(np.mean((before[in_band] - out["target_db"][in_band]) ** 2))),
                   deviation_after_db=float(np.sqrt(np.mean((after[in_band] - out["target_db"][in_band]) ** 2))))
    return out


def design(specs, n_fft, fs, b=6, f_low=40.0, f_high=16000.0, transition=0.5, reg_in=-20.0, reg_out=20.0, tilt=0.0,
           max_boost_db=12.0, points_per_octave=48, f_min=20.0, f_max=20000.0):
    """From the members' spectra of one row to c: dict of P, lo, hi, S, f, bins, in_band, ref, t, beta, c, clamped."""
    lo, hi = windows(n_fft, b)
    p = power(specs)
    s = smooth(p, lo, hi)
    f = grid(fs, points_per_octave, f_min, f_max)
    bins = grid_bins(f, n_fft, fs)
    in_band = (f >= f_low) & (f <= f_high)
    ref = reference_level(s[bins], in_band)
    t, beta = tables(n_fft, fs, f_low, f_high, transition, reg_in, reg_out, tilt)
    c, clamped = correction(s, ref, t, beta, 10.0 ** (max_boost_db / 20.0))
    return dict(P=p, lo=lo, hi=hi, S=s, f=f, bins=bins, in_band=in_band, ref=ref, t=t, beta=beta, c=c, clamped=clamped, n=n_fft)


def predict(specs, f32, n_fft, lo, hi):
    """(F, A, A_s) of the prediction with NumPy's own transform of the float32 filter."""
    F = np.fft.rfft(np.asarray(f32, dtype=np.float32).astype(np.float64), n=n_fft)
    a = power(specs, F)
    return F, a, smooth(a, lo, hi)


# ================================================================================================ the filter
def filter_chain(c, n_fft):
    """minphase_ref.chain's steps on the complex (c, 0), float64: a dict in the shape minphase_ref.Bounds reads (G, c =
    the cepstrum, power, P, P_floor, seg, n, d, sum_abs_c, phi_min) with g = the minimum-phase response, N samples."""
    c = np.asarray(c, dtype=np.float64)
    n = int(n_fft)
    pw = c * c + 0.0 * 0.0
    P = float(np.max(pw))
    p_floor = P * 10.0 ** (-300.0 / 10.0)
    G = 0.5 * np.log(np.maximum(pw, p_floor))
    cep = np.fft.irfft(G.astype(np.complex128), n=n)
    T = np.fft.rfft(cep[: n // 2], n=n)
    phi = 2.0 * T.imag
    M = np.exp(G) * (np.cos(phi) + 1j * np.sin(phi))
    M[0], M[-1] = M[0].real, M[-1].real
    g = np.fft.irfft(M, n=n)
    return dict(G=G, c=cep, power=pw, P=P, P_floor=p_floor, n=n, d=n, seg=np.zeros(1), phi_min=phi, T=T,
                sum_abs_c=float(np.sum(np.abs(cep[1 : n // 2]))), g=g, valid=True)


class FilterBounds(MR.Bounds):
    """minphase_ref.Bounds with E_X = 0: the chain's input is exact (module docstring)."""

    def __init__(self, ref):
        n = ref["n"]
        nbins = n // 2 + 1
        self.e_x = 0.0
        gn = float(np.sqrt(np.sum(ref["G"] ** 2)))
        self.mag = np.sqrt(ref["power"])
        d_g = U * (3.0 * gn + 2.0 * np.sqrt(nbins))
        self.inverse_path = L.predict_inverse_path(n, False)
        t_inv = L.inverse_const(n, *self.inverse_path) * U * np.sqrt(2.0) * gn / n
        cn = float(np.sqrt(np.sum(ref["c"][: n // 2] ** 2)))
        _, e_t, _ = L.forward_bound(n, cn, cn, False, d=n // 2, w=n, padded=True)
        self.first = 2.0 ** -23 * (ref["sum_abs_c"] + (n // 2) * t_inv) + n * 2.0 ** -150
        self.second = 2.0 * d_g + n * t_inv + 2.0 * e_t
        self.n = n

    def filter(self, ref, v):
        """Per sample of f = float32(g v), g = ref["g"]."""
        taps = v.size
        resp = self.response(ref, ref["g"])[:taps]
        f = ref["g"][:taps] * v
        return v * resp + 2.0 ** -24 * (np.abs(f) + v * resp) + 2.0 ** -149


def forward_error(x, n_fft):
    """E_X of a channel's transform at N (longfft_ref.forward_bound, rigorous)."""
    seg = np.asarray(x, dtype=np.float32).astype(np.float64)
    xn = float(np.sqrt(np.sum(seg ** 2)))
    return L.forward_bound(n_fft, xn, xn, False, d=seg.size, w=n_fft, padded=True)[1]


def log_c_bound(s_k, s_grid_in_band, e_x):
    """|d ln c_k| per bin (module docstring): 2 E_X (1 / |X|_window,k + 1 / min_grid |X|_window) (1 + 2^-16) + 2^-40."""
    with np.errstate(divide="ignore"):
        return 2.0 * e_x * (1.0 / np.sqrt(s_k) + 1.0 / np.sqrt(float(np.min(s_grid_in_band)))) * (1.0 + 2.0 ** -16) + 2.0 ** -40


def input_term(c, dlnc, n_fft, v):
    """How far f moves when ln c moves by at most dlnc per bin (a scalar: the largest of log_c_bound).  G = ln c moves by
    dlnc, phi_min by at most 2 sum_n |dcep[n]| <= 2 sqrt(N/2) ||dcep||_2 <= 2 ||dG||_2 <= 2 sqrt(N/2 + 1) dlnc (the T line of
    minphase_ref's docstring), M_k by |M_k| (|dG_k| + |dphi_k|) and g[n] by (2/N) sum_k |dM_k|:
        v[n] (2 / N) sum_k c_k (1 + 2 sqrt(N/2 + 1)) dlnc (1 + 2^-16)"""
    nbins = n_fft // 2 + 1
    return v * (2.0 / n_fft) * float(np.sum(np.abs(c))) * (1.0 + 2.0 * np.sqrt(nbins)) * dlnc * (1.0 + 2.0 ** -16)


# ================================================================================================ closed forms
def one_pole(d=64, r=0.5):
    """x[n] = r^n, n < D, float32 (exact for r = 0.5, D <= 127)."""
    return (r ** np.arange(d, dtype=np.float64)).astype(np.float32)
