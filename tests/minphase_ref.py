"""
Restatement of the minimum-phase chain (audio_analysis_amd/analyse/minphase.py) in NumPy float64, for the tests: the
cepstrum stays in float64 (no float32 step), numpy.fft does the transforms, nothing of the package's engine is used.
Helper module, like fdw_ref.py / burstdecay_ref.py: it holds no tests.

What is here
  * chain(x, p, D, N, floor_db): every line of the module's docstring, with sum |c[n]| over 1 <= n < N/2 beside it;
    records(ref, bins) cuts the per-point records ira_minphase_gather leaves out of it; minimum_phase_ir the response.
  * the bounds the device is held to (Bounds), derived below;
  * the analytic cases: a minimum-phase FIR from its zeros and its phase in closed form, a first-order all-pass.

Bounds (u = 2^-53).  E_X is the rigorous bound tests/longfft_ref.py states on ||X_dev - X||_2 over the bins of the path the
planner takes for (N, data_len D) (forward_bound, rigorous form); it bounds every single bin as well.
  G    |dG_k| <= |dX_k| |X_k| / max(|X_k|^2, P_floor) <= |dX_k| / max(|X_k|, sqrt(P_floor)): the transform's error divided
       by the magnitude, and by the floor (in amplitude) where the floor enters through ln; over all bins the divisor is
       m = max(min_k |X_k|, sqrt(P_floor)).  A floored bin moves with the floor instead: |dP| / (2 P) <= E_X / sqrt(P).
       re^2 + im^2 (2 u relative), the library's ln (2 ulp of G) and the 0.5 (exact) add u (3 |G_k| + 2).  In the 2-norm:
           dG = E_X / m + sqrt(N/2 + 1) E_X / sqrt(P) + u (3 ||G||_2 + 2 sqrt(N/2 + 1))
  c    the inverse transform of the exact G is off by t_inv = c_inv u sqrt(2) ||G||_2 / N per sample (longfft_ref
       docstring 6, inverse_const of the path taken), and carries dG as ||dc||_2 <= sqrt(2 / N) dG (Parseval).
  f32  rounding c to float32 moves c[n] by at most 2^-24 |c[n]| (+ 2^-150 below the normal range), and phi_min = 2 Im T =
       -2 sum_n c[n] sin(2 pi k n / N) by at most 2 sum_n |dc[n]|:
           first = 2^-23 (sum_{1 <= n < N/2} |c[n]| + (N/2) t_inv) + N 2^-150
       the term the issue names; c[0] meets sin 0 and does not enter.
  T    phi_min carries the float64 errors of c as 2 sum_n |dc[n]| <= 2 sqrt(N/2) ||dc||_2 = 2 dG + N t_inv, and the second
       forward transform's own error E_T (forward_bound at data_len N/2 on ||c[:N/2]||_2) twice:
           second = 2 dG + N t_inv + 2 E_T
  phi_rel  the angle of X_k moves by at most |dX_k| / |X_k| <= E_X / |X_k|; atan2 (2 ulp of pi), the turn's product and the
       sum add 8 u pi.
The device against this restatement: |phi_min| <= first + 2 second (NumPy's own transforms obey the same analysis with
smaller constants, so the restatement is allowed the device's share once more), the wrapped excess phase the same plus
2 E_X / |X_k| + 16 u pi, compared modulo 2 pi (numpy.unwrap is discontinuous where a step lies within the bound of pi; a
whole turn is no error of the chain).  A group delay is the difference of two such phases over 4 pi / N.
Against the analytic cases the restatement is allowed `second` (+ the phi_rel term), the device first + second.
The minimum-phase response is held per sample to Bounds.response, derived in its docstring from the same terms.
"""
import functools

import numpy as np

import longfft_ref as L

U = 2.0 ** -53
TWO_PI = 2.0 * np.pi
FIELDS = 8


def wrap(d):
    d = np.asarray(d, dtype=np.float64)
    return d - TWO_PI * np.rint(d / TWO_PI)


def sizes(length, p, fs, oversample=4, post_ms=None):
    """(D, N) of the module's docstring."""
    d = int(length) if post_ms is None else min(int(length), int(p) + 1 + int(np.rint(post_ms * fs / 1000.0)))
    n = 32
    while n < oversample * d:
        n *= 2
    return d, n


def grid_bins(n_fft, fs, points_per_octave=48, f_min=20.0, f_max=20000.0):
    top = min(f_max, fs / 2.0)
    count = int(np.floor(np.log2(top / f_min) * points_per_octave)) + 2
    f = f_min * 2.0 ** (np.arange(count, dtype=np.float64) / float(points_per_octave))
    f = f[f <= top]
    return np.clip(np.rint(f * float(n_fft) / fs), 1, n_fft // 2 - 1).astype(np.int64)


def chain(x, p, d, n, floor_db=-120.0):
    """The chain of one channel in float64: dict of X, P, P_floor, power, floored, G, c, sum_abs_c, T, phi_min, phi_rel,
    wrapped, excess, tau_e, tau_min (the delays in samples, NaN at k = 0 and N/2), valid."""
    seg = np.asarray(x, dtype=np.float32)[:d].astype(np.float64)
    k = np.arange(n // 2 + 1, dtype=np.int64)
    with np.errstate(all="ignore"):
        X = np.fft.rfft(seg, n=n)
        power = X.real * X.real + X.imag * X.imag
        P = float(np.max(power)) if not np.isnan(power).any() else float("nan")
    valid = bool(P > 0.0 and np.isfinite(P))
    out = dict(X=X, P=P, power=power, valid=valid, n=n, d=d, p=int(p), seg=seg)
    if not valid:
        return out
    p_floor = P * 10.0 ** (floor_db / 10.0)
    G = 0.5 * np.log(np.maximum(power, p_floor))
    c = np.fft.irfft(G.astype(np.complex128), n=n)
    T = np.fft.rfft(c[: n // 2], n=n)
    phi_min = 2.0 * T.imag
    turn = ((k * int(p)) % n).astype(np.float64) / float(n)
    phi_rel = np.arctan2(X.imag, X.real) + TWO_PI * turn
    wrapped = wrap(phi_rel - phi_min)
    excess = np.unwrap(wrapped)
    step = 4.0 * np.pi / n
    tau_e, tau_min = np.full(k.size, np.nan), np.full(k.size, np.nan)
    tau_e[1:-1] = -(excess[2:] - excess[:-2]) / step
    tau_min[1:-1] = -(phi_min[2:] - phi_min[:-2]) / step
    out.update(P_floor=p_floor, floored=power < p_floor, G=G, c=c, sum_abs_c=float(np.sum(np.abs(c[1 : n // 2]))), T=T,
               phi_min=phi_min, phi_rel=phi_rel, wrapped=wrapped, excess=excess, tau_e=tau_e, tau_min=tau_min)
    return out


def records(ref, bins):
    """The (J, FIELDS) records of the grid bins: Re X, Im X, Im T at k - 1, k, k + 1, excess at k - 1, k, k + 1."""
    k = np.asarray(bins, dtype=np.int64)
    if not ref["valid"]:
        return np.full((k.size, FIELDS), np.nan)
    X, T, e = ref["X"], ref["T"], ref["excess"]
    return np.stack([X.real[k], X.imag[k], T.imag[k - 1], T.imag[k], T.imag[k + 1], e[k - 1], e[k], e[k + 1]], axis=1)


def minimum_phase_ir(ref):
    """h_min in float64: irfft(e^G (cos phi_min, sin phi_min)) with the edge bins real, the first D samples."""
    M = np.exp(ref["G"]) * (np.cos(ref["phi_min"]) + 1j * np.sin(ref["phi_min"]))
    M[0], M[-1] = M[0].real, M[-1].real
    return np.fft.irfft(M, n=ref["n"])[: ref["d"]]


# ================================================================================================ bounds
class Bounds:
    """The bounds of the module docstring for one channel (ref = chain(..)): first, second, and e_x; phi_min(device),
    phi_rel(k), excess(k, device), in radians."""

    def __init__(self, ref):
        n, d = ref["n"], ref["d"]
        nbins = n // 2 + 1
        xn = float(np.sqrt(np.sum(ref["seg"] ** 2)))
        _, self.e_x, self.path = L.forward_bound(n, xn, xn, False, d=d, w=n, padded=True)
        gn = float(np.sqrt(np.sum(ref["G"] ** 2)))
        self.mag = np.sqrt(ref["power"])
        d_g = (self.e_x / max(float(np.min(self.mag)), np.sqrt(ref["P_floor"])) + np.sqrt(nbins) * self.e_x / np.sqrt(ref["P"])
               + U * (3.0 * gn + 2.0 * np.sqrt(nbins)))
        self.inverse_path = L.predict_inverse_path(n, False)
        t_inv = L.inverse_const(n, *self.inverse_path) * U * np.sqrt(2.0) * gn / n
        cn = float(np.sqrt(np.sum(ref["c"][: n // 2] ** 2)))
        _, e_t, _ = L.forward_bound(n, cn, cn, False, d=n // 2, w=n, padded=True)
        self.first = 2.0 ** -23 * (ref["sum_abs_c"] + (n // 2) * t_inv) + n * 2.0 ** -150
        self.second = 2.0 * d_g + n * t_inv + 2.0 * e_t
        self.n = n

    def phi_min(self, against_device=True, analytic=False):
        if analytic:
            return (self.first if against_device else 0.0) + self.second
        return self.first + 2.0 * self.second

    def phi_rel(self, k, shares=2):
        with np.errstate(divide="ignore"):
            return shares * (self.e_x / self.mag[k] + 8.0 * U * np.pi)

    def excess(self, k, against_device=True, analytic=False):
        return self.phi_min(against_device, analytic) + self.phi_rel(k, 1 if analytic else 2)

    def delay(self, phase_bound_lo, phase_bound_hi):
        """samples: two phase errors over 4 pi / N"""
        return (phase_bound_lo + phase_bound_hi) / (4.0 * np.pi / self.n)

    def response(self, ref, h):
        """Per sample of h = minimum_phase_ir(ref): how far the device's float32 h_min may lie from it.

        h[n] = (1/N) sum_k w_k Re(M_k e^{2 pi i k n / N}), w_k = 2 but 1 at the edges, so |dh[n]| <= (2/N) sum_k |dM_k|.
          M    M_k = e^{G_k} e^{i phi_min_k} moves by |M_k| (|dG_k| + |dphi_min_k|) to first order (both are below 1e-5;
               the second order is allowed as a factor 1 + 2^-16).  dG_k per bin is the G line of the module docstring,
               the device's and the restatement's share each: 2 (E_X / max(|X_k|, sqrt(P_floor)) + E_X / sqrt(P)) +
               2 u (3 |G_k| + 2); dphi_min_k <= phi_min(), which already holds both shares.  exp, sincos and the two
               products of ira_minphase_spectrum, and NumPy's, add 2 * 9 u |M_k| (tests/minphase_kernels_ref.py).
                   spec = (2/N) sum_k |M_k| (dG_k + phi_min() + 18 u) (1 + 2^-16)
          inv  the inverse transform of the exact M is off by c_inv u sqrt(2) ||M||_2 / N per sample (longfft_ref
               docstring 6, inverse_const of the path taken, as for t_inv above), once for the device and once more for
               numpy.fft: inv = 2 c_inv u sqrt(2) ||M||_2 / N
          f32  the output is rounded to float32 once: 2^-24 (|h[n]| + spec + inv) + 2^-149
        """
        n = self.n
        m = np.exp(ref["G"])
        d_g = (2.0 * (self.e_x / np.maximum(self.mag, np.sqrt(ref["P_floor"])) + self.e_x / np.sqrt(ref["P"]))
               + 2.0 * U * (3.0 * np.abs(ref["G"]) + 2.0))
        spec = (2.0 / n) * float(np.sum(m * (d_g + self.phi_min() + 18.0 * U))) * (1.0 + 2.0 ** -16)
        inv = 2.0 * L.inverse_const(n, *self.inverse_path) * U * np.sqrt(2.0) * float(np.sqrt(np.sum(m * m))) / n
        return 2.0 ** -24 * (np.abs(np.asarray(h, dtype=np.float64)) + spec + inv) + 2.0 ** -149 + spec + inv


def mod_turns(err):
    """err with the whole turns taken out."""
    return wrap(err)


def ambiguous_steps(ref, bound):
    """How many steps of the wrapped excess phase lie within `bound` of pi: where numpy.unwrap may turn the other way."""
    step = np.abs(wrap(np.diff(ref["wrapped"])))
    return int(np.count_nonzero(np.pi - step <= bound))


# ================================================================================================ analytic cases
# zeros of the minimum-phase FIR: two conjugate pairs and a real one, designed at r = 0.88 and held inside r = 0.9 after the
# taps are rounded; its first tap is the largest
ZEROS = np.array([0.88 * np.exp(1j * 1.9), 0.88 * np.exp(-1j * 1.9), 0.6 * np.exp(1j * 0.7), 0.6 * np.exp(-1j * 0.7), -0.3])
RADIUS = 0.9
TAP_BITS = 10


@functools.lru_cache(maxsize=None)
def min_phase_fir():
    """(a): prod (1 - z_i z^-1) with the taps rounded to multiples of 2^-10, float32.  So few bits keep every sample of
    the cases built from it -- delayed, reversed, through the dyadic all-pass below -- exact in float32: the closed forms
    (which use the zeros of the ROUNDED taps) then describe the very samples the chain is given."""
    h = np.array([1.0])
    for z in ZEROS:
        h = np.convolve(h, [1.0, -z])
    return (np.rint(h.real * 2.0 ** TAP_BITS) / 2.0 ** TAP_BITS).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fir_zeros():
    z = np.roots(min_phase_fir().astype(np.float64))
    assert z.size == ZEROS.size and np.max(np.abs(z)) <= RADIUS
    return z


def fir_phase(n):
    """phi_min of (a) at the bins of an N-point transform, closed form: sum_i angle(1 - z_i e^{-i w}), each term continuous
    in (-pi/2, pi/2)."""
    w = TWO_PI * np.arange(n // 2 + 1) / n
    return np.sum(np.angle(1.0 - fir_zeros()[:, None] * np.exp(-1j * w)[None, :]), axis=0)


def aliasing(n, zeros=ZEROS.size, r=RADIUS):
    """cepstral aliasing of an N-point cepstrum of Z zeros within radius r, in phi_min: 2 Z r^(N/2) / ((N/2) (1 - r))."""
    return 2.0 * zeros * r ** (n / 2) / ((n / 2) * (1.0 - r))


ALLPASS_A = 0.5


def allpass_ir(length):
    """(-a + z^-1) / (1 - a z^-1) truncated to `length` samples: -a, (1 - a^2) a^(m - 1), m >= 1."""
    a = ALLPASS_A
    h = (1.0 - a * a) * a ** (np.arange(length, dtype=np.float64) - 1.0)
    h[0] = -a
    return h


def allpass_phase(n):
    w = TWO_PI * np.arange(n // 2 + 1) / n
    e = np.exp(-1j * w)
    return np.angle((-ALLPASS_A + e) / (1.0 - ALLPASS_A * e))


def fir_through_allpass(length=64):
    """(c): (a) convolved with the all-pass, `length` samples, float32; the truncation is a^length."""
    return np.convolve(min_phase_fir().astype(np.float64), allpass_ir(length))[:length].astype(np.float32)
