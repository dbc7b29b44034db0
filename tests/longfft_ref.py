"""
Restatement of the long-FFT kernels (ira_fftsmooth.hip: the direct 2^a 3^b 5^c transform; ira_fftlong.hip: Bluestein) in
NumPy long double alone (64-bit mantissa), for the tests: no numpy.fft, no scipy, nothing of the package's engine.

What is here
  * rfft_ref / irfft_masked_ref: numpy.fft.rfft(x[:d] * hanning(w)[:d], n=L) and numpy.fft.irfft(X * mask, n) restated.
    The DFT is a recursive mixed-radix Cooley-Tukey over the prime factors of L (one call per factor, every sub-transform of
    a level in one batch), a direct O(p^2) DFT at prime leaves (a long-double chirp convolution above PRIME_DIRECT_MAX, where the direct
    sum would take minutes; held to the direct sum by the CPU tests), the direct O(L^2) sum below DIRECT_BELOW.  Every twiddle is
    unit_root(idx, L): the integer index is reduced mod L and to one octant BEFORE it meets pi = 4 atan(1).
  * the planner's choices restated (smooth_split_py, factor_radices_py, conv_size_py, bluestein_geometry, predict_path), so
    that the CPU tests can show which path every tested length takes without a device;
  * the bounds (direct_bound, bluestein_bound, band_bound);
  * planted errors (planted_spectrum, planted_band_signal): a float64 restatement that does one thing wrong.

Window.  hanning(w)[i] = 0.5 + 0.5 cos(pi (2 i + 1 - w) / (w - 1)), hanning(1) = 1, evaluated for every sample i < d that is
read.  NumPy defines x[:d] * hanning(w)[:d] for d <= w only (and for w = 1); for w < d the kernels evaluate the same cosine
past the end of the window, and that continuation is what the reference states (DESIGN.md, section "long-FFT edges").

Bounds.  u = 2^-53.  All are first order in u and normwise; v is the windowed, truncated, zero-padded input (exactly
representable products are not assumed: the window's own error is a term), x the samples that are read.

 (1) Elementary constants.  A complex product costs sqrt(5) u relative (CMUL); a sum u.  A table entry
     exp(-2 pi i k / P) is built on the host as cos / sin of fl(fl(-2 fl(pi) k) / P): the angle carries 2.35 u relative
     (pi's own rounding 0.35 u, one product, one quotient), so the entry is off by mu(theta) = (2.35 |theta| + 1.5) u,
     theta <= 2 pi.  Device sincospi / cospi: LIB_ULP = 2 ulp.

 (2) One in-LDS radix-r pass of the direct transform (dif_pass): the butterfly B_r (roundings on the longest path through
     bfly<r>: 2 -> 1, 4 -> 2, 3 -> 4, 5 -> 6, 8 -> 3 + CMUL, 6 -> B_3 + 1 + CMUL, 10 -> B_5 + 1 + CMUL), then, unless it is
     the last pass of the sub-transform (len == r: p == 0 everywhere), the twiddle W^(k p), k < r, formed as
     coarse * fine (mu(2 pi / r) + 1.5 u + CMUL) and raised to the power k by repeated products:
     T_r = mu(2 pi) ... precisely  2.35 * 2 pi (r - 1) / r + (r - 1) (3 + CMUL) + CMUL   (units of u).
     passes(N) = sum over the radices factor_radices(N) gives.

 (3) Direct transform of n = n1 n2 (two passes over the data):
        c_direct = passes(n1) + passes(n2) + INTER + 1,   INTER = mu(2 pi) + mu(2 pi / n1) + 2 CMUL
     (the product th * tl of two table entries and its application; + 1 for the zeroing / store conversions), so that
        || X_dev - X ||_2  <=  c_direct u sqrt(n) ||v||_2  +  sqrt(n) ||dv||_2 ,   ||dv||_2 <= c_win u ||x||_2,
        c_win = pi A + LIB_ULP + 2      (A = max(1, max_i |2 i + 1 - w| / (w - 1)): the argument carries at most 2 u
     relative -- one quotient here, a rounded reciprocal and a product in the Bluestein pass -- which cos turns into
     pi A 2 u / 2 on 0.5 + 0.5 cos; cospi is within 2 ulp; 0.5 + 0.5 c and the product with the sample round once each).
     A half-length job transforms z = x[2m] + i x[2m+1] (||z|| = ||v||, length n/2) and untangles
     X[k] = E[k] + W_2n^k O[k]: every returned bin takes two bins of Z, so the transform's error enters twice
     (sqrt(n/2) * 2 = sqrt(2) sqrt(n)), and the untangling adds UNT = 3 + CMUL + LIB_ULP + ROT * steps, where the fused
     job rotates W along a thread's run of steps = ceil(2 n2 / 256) - 1 elements (ROT = CMUL + 2.35 pi / 2 + 2 per step) and
     the split job calls sincospi per bin (steps = 0).

 (4) Bluestein, X[k] = w_k IFFT_M(FFT_M(v w) * Bhat)[k], M = N1 N2 from conv_size / ira_fft_split, radix-16 passes then
     radix 4 / 2 (lds_fft_dif), a radix-3 stage when M = 3 2^k.  Stage constants: radix 16: 4 + 2 CMUL butterfly, twiddle
     powers k <= 15 by a tree of depth 4: 2.35 * 2 pi + 15 (3 + CMUL) + 5 CMUL; radix 4: 2 + mu(2 pi) + 1.5 + 2 CMUL;
     radix 2 (last, no twiddle): 1; radix 3 stage: 4 + mu(2 pi) + 1.5 + 2 CMUL; the step between the passes INTER as above.
     c_M = stages(N1) + stages(N2) + INTER.  The chirps w_n run along a thread's elements by the recurrence
     w_{j+1} = w_j d_j, d_{j+1} = d_j e2 from exactly reduced starts: after j steps d is off by (LIB_ULP + 1) +
     j (CMUL + LIB_ULP + 1) and w by the sum of those, c_chirp(steps); steps = ceil(N1 C / 256) - 1 (0 for the small M
     the edge tests use most).  The Hann window is a rotation over the same run: c_win as above with A taken at the start
     of the run, plus steps * (CMUL + 2.35 pi a + LIB_ULP + 1), a = the rotation step in half-turns.
     With beta = max_k |Bhat_k| (evaluated in long double from the filter the kernel builds; the convolution's gain):
        rigorous:  || X_dev - X ||_2 <= u beta ||v|| (c_chirp + c_M + CMUL + c_M + c_chirp + 2)          [e1, e2, e4, e5]
                                         + u c_M sqrt(M) sqrt(2 L) ||v||                                   [e3: the filter]
                                         + beta ||dv||
     e3 bounds the precomputed filter spectrum's error by its 2-norm, c_M u sqrt(M) ||b||_2 (||b||_2 <= sqrt(2 L)), which
     is all a normwise analysis gives for a single entry: it costs sqrt(M) against what is observed.
     A half job (even L) is the same on z of length L / 2 followed by the untangling (UNT with sincospi per bin), a pair
     job the same on x1 + i x2 followed by a sum and a halving per bin (2 u), both entering twice as in (3).

 (5) The probabilistic form.  Rounding errors of different operations are independent and of either sign: a sum of c
     worst-case units grows like sqrt(c), not c (Higham and Mary, 2019: gamma_c -> lambda sqrt(c) u).  The primary
     assertion of the tests replaces every c above by LAMBDA sqrt(c) with LAMBDA = 3 (and e3 by LAMBDA sqrt(c_M) u beta
     ||v||: the filter spectrum is wrong by its relative error where it is used).  tests/test_longfft_ref_cpu.py shows that
     numpy's own float64 transform stays inside it on every input the GPU tests use and records by how much; the rigorous
     form stays as the second assertion, and every single bin is held to the rigorous 2-norm bound as well.

 (6) Band signals, float32 out of a float64 inverse: |y_dev - y| <= half an ulp of float32 at (|y| + t) + t,
     t = c_inv u sqrt(2) ||X mask||_2 / n, c_inv the rigorous constant of the inverse path ((3) with the Hermitian
     extension and mask products, 2 + CMUL, in place of the window; (4) for Bluestein lengths, scaled by beta / sqrt(L)):
     the 2-norm of the exact band signal is sqrt(2) ||X mask||_2 / sqrt(n) at most, and the transform's error spreads
     over its n outputs.  Two bands that share a complex transform (y1 + i y2) share its rounding: ||X mask||_2 is then
     that of both masked spectra together (a band whose own mask passes nothing still carries its partner's 1e-17).
"""
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
PI = 4 * np.arctan(LD(1))
DIRECT_BELOW = 8                 # the direct O(L^2) sum below this length
PRIME_DIRECT_MAX = 1024          # prime leaves up to here by the direct sum, larger ones by dft_chirp
CMUL = 5.0 ** 0.5
LIB_ULP = 2.0
LAMBDA = 3.0
SM_MAX_N, SM_MAXP, SM_MAX_RADICES, SM_TW, SM_THREADS = 1024, 6, 12, 66, 256


# ================================================================================================ unit roots and the DFT
def unit_root(idx, L):
    """exp(-2 pi i idx / L) -> (re, im) long double; idx: integers of any sign and size (int64 arithmetic)."""
    L = int(L)
    k = np.mod(np.asarray(idx, dtype=np.int64), L)               # 0 <= k < L
    quad = (4 * k) // L                                          # quarter turn
    r = 4 * k - quad * L                                         # 0 <= r < L: angle inside it = (pi / 2) r / L
    swap = 2 * r > L
    r = np.where(swap, L - r, r)
    ang = PI * (r.astype(LD) / LD(2 * L))
    c0, s0 = np.cos(ang), np.sin(ang)
    c, s = np.where(swap, s0, c0), np.where(swap, c0, s0)
    cq = np.select([quad == 0, quad == 1, quad == 2], [c, -s, -c], s)
    sq = np.select([quad == 0, quad == 1, quad == 2], [s, c, -s], -c)
    return cq, -sq


def smallest_prime_factor(n):
    for p in (2, 3, 5, 7):
        if n % p == 0:
            return p
    p = 11
    while p * p <= n:
        if n % p == 0:
            return p
        p += 2
    return n


def dft_direct(xr, xi, L):
    """The defining sum, (B, L) long double in and out; twiddles from a table of the L unit roots indexed by j k mod L."""
    tc, ts = unit_root(np.arange(L), L)
    j = np.arange(L, dtype=np.int64)
    outr, outi = np.empty_like(xr), np.empty_like(xr)
    step = max(1, (1 << 22) // max(L, 1))
    for k0 in range(0, L, step):
        k = np.arange(k0, min(L, k0 + step), dtype=np.int64)
        idx = (k[None, :] * j[:, None]) % L                      # (L, kk)
        c, s = tc[idx], ts[idx]
        outr[:, k0 : k0 + k.size] = xr @ c - xi @ s
        outi[:, k0 : k0 + k.size] = xr @ s + xi @ c
    return outr, outi


def dft_chirp(xr, xi, L):
    """The same sum for a LARGE prime L (where the direct sum would take minutes) as a chirp convolution in long double:
    X[k] = w_k sum_n (x_n w_n) conj(w_(k-n)), w_n = exp(-i pi n^2 / L) = unit_root(n^2 mod 2 L, 2 L), the convolution by
    two power-of-two dft_ld.  tests/test_longfft_ref_cpu.py holds it to the direct sum at primes both can do."""
    n = np.arange(L, dtype=np.int64)
    wc, ws = unit_root((n * n) % (2 * L), 2 * L)
    M = 1 << (2 * L - 2).bit_length()
    B = xr.shape[0]
    ar, ai = np.zeros((B, M), dtype=LD), np.zeros((B, M), dtype=LD)
    ar[:, :L], ai[:, :L] = xr * wc - xi * ws, xr * ws + xi * wc
    br, bi = np.zeros((1, M), dtype=LD), np.zeros((1, M), dtype=LD)
    br[0, :L], bi[0, :L] = wc, -ws
    br[0, M - n[1:]], bi[0, M - n[1:]] = wc[1:], -ws[1:]
    Ar, Ai = dft_ld(ar, ai, M)
    Br, Bi = dft_ld(br, bi, M)
    pr, pi_ = Ar * Br - Ai * Bi, Ar * Bi + Ai * Br
    yr, yi = dft_ld(pr, -pi_, M)                                  # inverse = conj(DFT(conj .)) / M
    yr, yi = yr[:, :L] / LD(M), -yi[:, :L] / LD(M)
    return yr * wc - yi * ws, yr * ws + yi * wc


def dft_ld(xr, xi, L, direct_below=DIRECT_BELOW):
    """DFT of every row of (B, L) long double arrays: recursion over the prime factors of L."""
    if L == 1:
        return xr.copy(), xi.copy()
    p = smallest_prime_factor(L)
    if L < direct_below or (p == L and L <= PRIME_DIRECT_MAX):
        return dft_direct(xr, xi, L)
    if p == L:
        return dft_chirp(xr, xi, L)
    m, B = L // p, xr.shape[0]
    sub = lambda a: np.ascontiguousarray(a.reshape(B, m, p).transpose(0, 2, 1)).reshape(B * p, m)
    yr, yi = dft_ld(sub(xr), sub(xi), m, direct_below)            # Y[b, r, k] = DFT_m(x[p j + r])
    yr, yi = yr.reshape(B, p, m), yi.reshape(B, p, m)
    outr, outi = np.empty((B, p, m), dtype=LD), np.empty((B, p, m), dtype=LD)
    k = np.arange(m, dtype=np.int64)
    for q in range(p):                                           # X[k + m q] = sum_r W_L^(r (k + m q)) Y_r[k]
        ar, ai = yr[:, 0, :].copy(), yi[:, 0, :].copy()
        for r in range(1, p):
            c, s = unit_root(r * (k + m * q), L)
            ar += yr[:, r, :] * c - yi[:, r, :] * s
            ai += yr[:, r, :] * s + yi[:, r, :] * c
        outr[:, q, :], outi[:, q, :] = ar, ai
    return outr.reshape(B, L), outi.reshape(B, L)


def hann_ld(i, w):
    """hanning(w)[i] in long double from the integer argument; hanning(1) = 1; i may run past w - 1 (module docstring)."""
    i = np.asarray(i, dtype=np.int64)
    if w <= 1:
        return np.ones(i.shape, dtype=LD)
    num = 2 * i + 1 - w                                          # cos(pi num / den) = Re exp(-2 pi i num / (2 den))
    c, _ = unit_root(num, 2 * (w - 1))
    return LD(0.5) + LD(0.5) * c


def windowed_input(x, L, data_len=None, win_len=None, hann=False):
    """(v, xs): the L long-double values that are transformed and the samples read, zero padded (x: (B, >= ...) or 1-D)."""
    x = np.atleast_2d(np.asarray(x))
    d = L if data_len is None else int(data_len)
    w = L if win_len is None else int(win_len)
    take = max(0, min(d, L, x.shape[1]))
    xs = np.zeros((x.shape[0], L), dtype=LD)
    xs[:, :take] = x[:, :take].astype(LD)
    v = xs * hann_ld(np.arange(L), w)[None, :] if hann else xs.copy()
    return v, xs


def rfft_ref(x, L, data_len=None, win_len=None, hann=False, direct_below=DIRECT_BELOW, closed_form=True):
    """numpy.fft.rfft(x[:d] * numpy.hanning(w)[:d], n=L) in long double: (re, im), each (B, L // 2 + 1) -- or 1-D for 1-D x.
    closed_form: a row with a single non-zero sample is written down as a exp(-2 pi i j k / L) instead of transformed (the
    CPU tests hold the two to each other)."""
    v, _ = windowed_input(x, L, data_len, win_len, hann)
    nb = L // 2 + 1
    re, im = np.zeros((v.shape[0], nb), dtype=LD), np.zeros((v.shape[0], nb), dtype=LD)
    nnz = np.count_nonzero(v, axis=1)
    one = np.flatnonzero(nnz == 1) if closed_form else np.zeros(0, dtype=np.int64)
    for b in one:                                                 # a single sample a at j: a exp(-2 pi i j k / L), formed exactly
        j = int(np.flatnonzero(v[b])[0])
        c, s = unit_root(j * np.arange(nb, dtype=np.int64), L)
        re[b], im[b] = v[b, j] * c, v[b, j] * s
    rest = np.flatnonzero((nnz > 1) if closed_form else (nnz > 0))
    if rest.size:
        fr, fi = dft_ld(v[rest], np.zeros_like(v[rest]), L, direct_below)
        re[rest], im[rest] = fr[:, :nb], fi[:, :nb]
    im[:, 0] = 0
    if L % 2 == 0:
        im[:, -1] = 0
    return (re[0], im[0]) if np.ndim(x) == 1 else (re, im)


def irfft_masked_ref(X, mask32, n):
    """numpy.fft.irfft(X * mask, n) in long double.  X: the n // 2 + 1 complex128 bins the device holds, mask32 float32.
    The imaginary parts of bin 0 and (even n) of the Nyquist bin are ignored, as numpy does."""
    X = np.asarray(X, dtype=np.complex128)
    m = np.asarray(mask32, dtype=np.float32).astype(LD)
    nb = n // 2 + 1
    hr, hi = X.real[:nb].astype(LD) * m[:nb], X.imag[:nb].astype(LD) * m[:nb]
    hi[0] = 0
    if n % 2 == 0:
        hi[-1] = 0
    live = np.flatnonzero((hr != 0) | (hi != 0))
    if live.size == 0:
        return np.zeros(n, dtype=LD)
    if live.size == 1:                                            # one bin: an exact cosine, (2 -) Re(H exp(+2 pi i k t / n)) / n
        k0 = int(live[0])
        c, s = unit_root(k0 * np.arange(n, dtype=np.int64), n)    # exp(-2 pi i k t / n) = c + i s
        g = LD(1) if (k0 == 0 or 2 * k0 == n) else LD(2)
        return g * (hr[k0] * c + hi[k0] * s) / LD(n)
    fr, fi = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    fr[:nb], fi[:nb] = hr, hi
    k = np.arange(1, (n - 1) // 2 + 1)
    fr[n - k], fi[n - k] = hr[k], -hi[k]
    # inverse = conj(DFT(conj .)) / n; the result is real: only the real part of the forward transform is needed
    yr, _ = dft_ld(fr[None, :], -fi[None, :], n)
    return yr[0] / LD(n)


# ================================================================================================ the planner, restated
def factor_radices_py(n):
    """The radix chain ira_fftsmooth.hip's factor_radices gives for n, or None (another prime factor / too long)."""
    twos = threes = fives = 0
    while n % 2 == 0:
        n //= 2; twos += 1
    while n % 3 == 0:
        n //= 3; threes += 1
    while n % 5 == 0:
        n //= 5; fives += 1
    if n != 1:
        return None
    out = [8] * (twos // 3)
    twos %= 3
    if twos == 2:
        out.append(4)
    elif twos == 1:
        if fives:
            out.append(10); fives -= 1
        elif threes:
            out.append(6); threes -= 1
        else:
            out.append(2)
    out += [5] * fives + [3] * threes
    return out if len(out) <= SM_MAX_RADICES else None


def smooth_split_py(n):
    """(n1, n2) as ira_fft_smooth_split answers, or None: 64 <= n <= 1024^2, n = 2^a 3^b 5^c, the most balanced split
    with both factors in [2, 1024] (n1 <= n2 on a tie), both radix chains at most SM_MAXP passes long."""
    if n < 64 or n > SM_MAX_N * SM_MAX_N or factor_radices_py(n) is None:
        return None
    best, best_score = 0, -1
    for d in range(2, SM_MAX_N + 1):
        if n % d or n // d > SM_MAX_N or n // d < 2:
            continue
        n2 = n // d
        score = 2 * (SM_MAX_N - abs(d - n2)) + (1 if d <= n2 else 0)
        if score > best_score:
            best, best_score = d, score
    if best < 2:
        return None
    n1, n2 = best, n // best
    r1, r2 = factor_radices_py(n1), factor_radices_py(n2)
    if not r1 or not r2 or len(r1) > SM_MAXP or len(r2) > SM_MAXP:
        return None
    return n1, n2


def pick_columns_py(length, other):
    best = 1
    for c in range(1, 9):
        if other % c == 0 and (c * length + SM_TW) * 16 <= 26 * 1024:
            best = c
    return best


def conv_size_py(need, three_pow2=True):
    need = max(int(need), 16)
    m = 1 << (need - 1).bit_length()
    if three_pow2 and m >= 128 and 3 * (m >> 2) >= need:
        m = 3 * (m >> 2)
    return m


def bluestein_geometry(m):
    """(rad, N1, N2, C) of convolution size m as ira_fftlong.hip's split_of / make_plan choose them."""
    rad = 3 if m % 3 == 0 else 1
    log2p = (m // rad).bit_length() - 1
    if rad == 1:
        lq = min(max((log2p + 1) // 2, 2), log2p - 2)
    else:
        lq = (log2p - 1) // 2
    if log2p - lq > 13:
        lq = log2p - 13
    n1, n2 = rad << lq, 1 << (log2p - lq)
    col = rad * ((1 << lq) + 1)
    c = 8
    while c > 1 and c * col * 16 > 33 * 1024:
        c >>= 1
    return rad, n1, n2, min(c, n2)


def is_direct(L):
    return smooth_split_py(L) is not None


def predict_path(L, half_real_ffts=True, fuse_half_split=True, pair_across_channels=False, three_pow2_sizes=True,
                 padded=False, paired=False):
    """(family, kind, size) of one element of length L: family 'smooth' / 'bluestein'; kind 'half_fused', 'half_split',
    'full' (smooth) or 'half', 'pair', 'single' (Bluestein); size = transform length (smooth) / convolution size."""
    half_ok = (not pair_across_channels and L % 2 == 0 and L >= 128 and half_real_ffts and is_direct(L // 2))
    if half_ok:
        n1 = smooth_split_py(L // 2)[0]
        return "smooth", ("half_fused" if fuse_half_split and n1 % 2 == 0 else "half_split"), L // 2
    if is_direct(L):
        return "smooth", "full", L
    if half_real_ffts and not padded and L % 2 == 0 and L >= 8:
        return "bluestein", "half", conv_size_py(2 * (L // 2) - 1, three_pow2_sizes)
    if paired:
        return "bluestein", "pair", conv_size_py(2 * L - 1, three_pow2_sizes)
    return "bluestein", "single", conv_size_py(L + L // 2, three_pow2_sizes)


def predict_inverse_path(n, paired, half_real_ffts=True, three_pow2_sizes=True):
    """(family, kind, size) of one band_irfft job of length n: pairs take the full-length direct inverse, single bands the
    half-length one where the length allows it; everything else Bluestein over 2 n - 1 lags."""
    half_ok = n % 2 == 0 and n >= 128 and half_real_ffts and is_direct(n // 2)
    if is_direct(n) and (paired or not half_ok):
        return "smooth", "full", n
    if half_ok and not paired:
        return "smooth", "half", n // 2
    return "bluestein", "pair" if paired else "single", conv_size_py(2 * n - 1, three_pow2_sizes)


# ================================================================================================ bounds (units of u)
def mu(theta):
    return 2.35 * abs(theta) + 1.5


_B = {2: 1.0, 4: 2.0, 3: 4.0, 5: 6.0, 8: 3.0 + CMUL}
_B[6] = _B[3] + 1.0 + CMUL
_B[10] = _B[5] + 1.0 + CMUL
INTER = lambda n1: mu(2 * np.pi) + mu(2 * np.pi / n1) + 2 * CMUL
ROT = CMUL + 2.35 * np.pi / 2 + 2.0


def passes_const(N):
    """passes(N) of the module docstring: the stage constants of factor_radices(N), the last pass without twiddles."""
    rad = factor_radices_py(N)
    tot = 0.0
    for i, r in enumerate(rad):
        tot += _B[r]
        if i + 1 < len(rad):
            tot += 2.35 * 2 * np.pi * (r - 1) / r + (r - 1) * (3 + CMUL) + CMUL
    return tot


def win_const(d, w, extra=0.0):
    """c_win: error of one windowed sample in units of u |x_i| (A from the samples read; `extra` the rotation's share)."""
    if w <= 1:
        return 1.0
    i = np.array([0, max(d - 1, 0)], dtype=np.float64)
    A = max(1.0, float(np.max(np.abs(2 * i + 1 - w))) / (w - 1))
    return np.pi * A + LIB_ULP + 2.0 + extra


def _two_forms(c_terms, scale, extra_rig=0.0, extra_prob=0.0):
    """(prob, rig) from {name: (constant in u, scale)} terms that add (rigorous) or add in quadrature-of-counts (docstring 5)."""
    rig = sum(c * s for c, s in c_terms) * U + extra_rig
    prob = sum(LAMBDA * np.sqrt(c) * s for c, s in c_terms if c > 0) * U + extra_prob
    return min(prob, rig), rig


def direct_bound(L, kind, vnorm, xnorm, hann, d=None, w=None):
    """(prob, rig): bounds on ||X_dev - X||_2 over the bins of a direct-transform element of length L (kind from
    predict_path), vnorm = ||v||_2, xnorm = ||x read||_2."""
    d = L if d is None else d
    w = L if w is None else w
    nt = L if kind == "full" else L // 2
    n1, n2 = smooth_split_py(nt)
    c = passes_const(n1) + passes_const(n2) + INTER(n1) + 1.0
    rootn = np.sqrt(float(L))
    terms = []
    if kind == "full":
        terms.append((c, rootn * vnorm))
    else:
        steps = (2 * n2 + SM_THREADS - 1) // SM_THREADS - 1 if kind == "half_fused" else 0
        terms.append((c, np.sqrt(2.0) * rootn * vnorm))
        terms.append((3.0 + CMUL + LIB_ULP + ROT * steps, np.sqrt(2.0) * rootn * vnorm))
    if hann:
        terms.append((win_const(min(d, L), w), rootn * xnorm))
    return _two_forms(terms, 1.0)


def _pow2_stages(log2m):
    """Stage constants of lds_fft_dif / lds_fft_dit over 2^log2m points (docstring 4)."""
    s, tot = log2m, 0.0
    while s >= 4:
        tot += 4 + 2 * CMUL
        if s > 4:
            tot += 2.35 * 2 * np.pi + 15 * (3 + CMUL) + 5 * CMUL
        s -= 4
    while s >= 2:
        tot += 2.0
        if s > 2:
            tot += mu(2 * np.pi) + 1.5 + 2 * CMUL
        s -= 2
    if s == 1:
        tot += 1.0
    # a radix-16 pass that is not the last is followed by passes on its outputs: its twiddles were counted above
    return tot


def conv_const(m):
    rad, n1, n2, C = bluestein_geometry(m)
    c = _pow2_stages((n1 // rad).bit_length() - 1) + _pow2_stages(n2.bit_length() - 1) + INTER(n1)
    if rad == 3:
        c += 4 + mu(2 * np.pi) + 1.5 + 2 * CMUL
    steps = (n1 * C + 255) // 256 - 1
    return c, steps, (256 // C) * n2


def chirp_const(steps):
    d_err = lambda j: (LIB_ULP + 1) + j * (CMUL + LIB_ULP + 1)
    return (LIB_ULP + 1) + sum(CMUL + d_err(j) for j in range(steps))


@functools.lru_cache(maxsize=None)
def filter_gain(l, m):
    """beta = max |Bhat_k|: the chirp filter of transform length l in a convolution of size m, as value_input<IN_FILTER>
    lays it out (the negative side wins where the two sides overlap), transformed in long double."""
    n = np.arange(m, dtype=np.int64)
    neg = m - n
    idx = np.where(neg < l, neg, n)
    live = (neg < l) | (n < l)
    q = (idx * idx) % (2 * l)                                    # exp(+i pi idx^2 / l) = conj unit_root(q, 2 l)
    c, s = unit_root(q, 2 * l)
    br, bi = np.where(live, c, LD(0)), np.where(live, -s, LD(0))
    fr, fi = dft_ld(br[None, :], bi[None, :], m)
    return float(np.max(np.hypot(fr, fi)))


def bluestein_bound(L, kind, m, vnorm, xnorm, hann, d=None, w=None):
    """(prob, rig) for a Bluestein element of length L: kind 'single' / 'half' / 'pair', m its convolution size; for a pair
    vnorm / xnorm are those of x1 + i x2."""
    d = L if d is None else d
    w = L if w is None else w
    l = L // 2 if kind == "half" else L
    cM, steps, dn = conv_const(m)
    beta = filter_gain(l, m)
    cch = chirp_const(steps)
    twice = 1.0 if kind == "single" else 2.0
    s = twice * beta * vnorm
    terms = [(cch, s), (cM, s), (CMUL, s), (cM, s), (cch + 2.0, s)]
    e3_rig = twice * cM * U * np.sqrt(float(m)) * np.sqrt(2.0 * l) * vnorm
    e3_prob = twice * LAMBDA * np.sqrt(cM) * U * beta * vnorm
    if kind == "half":
        terms.append((3.0 + CMUL + LIB_ULP, s))
    elif kind == "pair":
        terms.append((2.0, s))
    if hann:
        st = 2 if kind == "half" else 1
        a = 2.0 * st * dn / max(w - 1, 1)
        terms.append((win_const(min(d, L), w, steps * (CMUL + 2.35 * np.pi * a + LIB_ULP + 1)), twice * beta * xnorm))
    return _two_forms(terms, 1.0, e3_rig, e3_prob)


def forward_bound(L, vnorm, xnorm, hann, d=None, w=None, **switches):
    """The bound of the path predict_path(L, **switches) names: (prob, rig, (family, kind, size))."""
    path = predict_path(L, **switches)
    if path[0] == "smooth":
        p, r = direct_bound(L, path[1], vnorm, xnorm, hann, d, w)
    else:
        p, r = bluestein_bound(L, path[1], path[2], vnorm, xnorm, hann, d, w)
    return p, r, path


def inverse_const(n, family, kind, size):
    """c_inv of docstring (6) in units of u, relative to sqrt(2) ||X mask||_2 / n."""
    if family == "smooth":
        n1, n2 = smooth_split_py(size)
        c = passes_const(n1) + passes_const(n2) + INTER(n1) + 1.0 + 2.0 + CMUL
        if kind == "half":
            steps = 4                                           # sincospi restarts every batch of SM_UC = 5 elements
            c = 2.0 * (c + 3.0 + CMUL + LIB_ULP + ROT * steps)
        return c + 14.0 * 4                                     # the narrow path sums <= 2 * 14 products instead of pass 1
    cM, steps, _ = conv_const(size)
    beta = filter_gain(n, size)
    rig_rel = (2 * chirp_const(steps) + 2 * cM + CMUL + 4.0 + CMUL) * beta + cM * np.sqrt(float(size)) * np.sqrt(2.0 * n)
    return rig_rel / np.sqrt(float(n))


def band_bound(y_ref, xm_norm, n, family, kind, size):
    """Elementwise bound on |y_dev - y_ref| (docstring 6); y_ref long double."""
    t = inverse_const(n, family, kind, size) * U * np.sqrt(2.0) * xm_norm / n
    a = (np.abs(y_ref) + LD(t)).astype(np.float32)
    a = np.maximum(a, np.float32(2.0 ** -126))
    return 0.5 * np.spacing(a).astype(np.float64) + t, t


# ================================================================================================ input families
FAMILY_NAMES = ("impulse", "constant", "alternating", "cosine", "noise")


def impulse_positions(L, n2=None, run=None):
    """j of the unit impulses: ends, the middle, the first / last index of the second column of a direct plan (n2, n2 - 1)
    and of a thread's second window-rotation step (run, run - 1)."""
    js = [0, 1, L // 2, L - 2, L - 1]
    for v in (n2, run):
        if v is not None:
            js += [v - 1, v]
    return sorted({j for j in js if 0 <= j < L})


def make_inputs(L, n2=None, run=None, seed=0, families=FAMILY_NAMES):
    """(names, x): float32 rows of length L, one per input."""
    names, rows = [], []
    n = np.arange(L)
    if "impulse" in families:
        for j in impulse_positions(L, n2, run):
            e = np.zeros(L, np.float32); e[j] = 1.0
            names.append(f"impulse j={j}"); rows.append(e)
    if "constant" in families:
        names.append("constant"); rows.append(np.full(L, 0.75, np.float32))
    if "alternating" in families:
        names.append("alternating"); rows.append(np.where(n % 2 == 0, 1.0, -1.0).astype(np.float32))
    if "cosine" in families and L >= 8:
        k0 = max(1, L // 7)
        k1 = (k0 + 40) % (L // 2 + 1) if L // 2 >= 41 else max(1, L // 2 - 1)
        c = np.cos(2 * np.pi * ((k0 * n) % L) / L) + 1e-6 * np.cos(2 * np.pi * ((k1 * n) % L) / L)
        names.append(f"cosine k={k0}+{k1}"); rows.append(c.astype(np.float32))
    if "noise" in families:
        rng = np.random.default_rng(1000 + seed + L)
        names.append("noise"); rows.append((rng.standard_normal(L) * np.exp(-n / max(L / 4.0, 1.0))).astype(np.float32))
    return names, np.stack(rows)


def direct_lengths(lo=64, hi=8192):
    return [n for n in range(lo, hi + 1) if is_direct(n)]


PLAN_EXTREMES = (3 ** 12, 5 ** 8, 1 << 20, 1024 * 1000, 729 * 720)


def bluestein_lengths(max_m=3 << 13, small_to=320):
    """Every non-direct L <= small_to, and every non-direct L within +-2 of each boundary of conv_size (single rule
    L + L // 2, half / pair rule 2 l - 1) up to max_m, with three_pow2_sizes on and off."""
    out = {L for L in range(1, small_to + 1) if not is_direct(L)}
    sizes = set()
    k = 16
    while k <= max_m:
        sizes.add(k)
        if 3 * (k >> 2) >= 96:
            sizes.add(3 * (k >> 2))
        k <<= 1
    for m in sorted(sizes):
        if m > max_m:
            continue
        single = max(L for L in range(1, m + 1) if L + L // 2 <= m)          # largest single length the size holds
        halfl = (m + 1) // 2                                                  # largest l with 2 l - 1 <= m
        for c in (single, halfl, 2 * halfl):                                  # (pair of length l, half job of L = 2 l)
            for L in range(c - 2, c + 3):
                if L >= 1 and not is_direct(L):
                    out.add(L)
    return sorted(out)


# ================================================================================================ planted errors
PLANTED = ("twiddle", "periodic_hann", "window_shift", "last_sample", "bin_swap", "chirp_wrap", "mirror_tile",
           "nyquist_imag")


def _dft_matrix64(n):
    c, s = unit_root((np.arange(n)[:, None] * np.arange(n)[None, :]) % n, n)
    return c.astype(np.float64) + 1j * s.astype(np.float64)


def planted_spectrum(x, L, kind, hann=True):
    """float64 half spectrum of the float32 row x (length L) with ONE thing wrong (a four-step restatement n1 x n2 of the
    direct transform for lengths it takes, the defining sum otherwise).  kind: one of PLANTED but 'nyquist_imag'."""
    x = np.asarray(x, dtype=np.float64)[:L]
    n = np.arange(L)
    win = hann_ld(n, L).astype(np.float64) if hann else np.ones(L)
    if kind == "periodic_hann":
        win = 0.5 - 0.5 * np.cos(2 * np.pi * n / L)
    elif kind == "window_shift":
        win = hann_ld(n + 1, L).astype(np.float64)
    v = x * win
    if kind == "last_sample":
        v[-1] = 0.0
    if kind == "chirp_wrap":
        # the input chirp exp(-i pi n^2 / L) with n * n wrapped to 32 bits: every other factor of Bluestein's identity is
        # right, so the result is the DFT of v[n] * w'[n] / w[n]
        q_ok = (n.astype(np.int64) ** 2) % (2 * L)
        q_bad = ((n.astype(np.int64) ** 2) & 0xFFFFFFFF) % (2 * L)
        c, s = unit_root(q_bad - q_ok, 2 * L)
        re, im = dft_ld((v.astype(LD) * c)[None, :], (v.astype(LD) * s)[None, :], L)
        return (re[0].astype(np.float64) + 1j * im[0].astype(np.float64))[: L // 2 + 1]
    if kind == "mirror_tile":
        nt = L // 2
        Z = _dft_matrix64(nt) @ (v[0::2] + 1j * v[1::2])
        k = np.arange(nt + 1)
        zk, zl = Z[k % nt], Z[(nt - k) % nt]
        k_bad = nt // 3
        zl[k_bad] = Z[(nt - k_bad - 1) % nt]
        E, O = 0.5 * (zk + np.conj(zl)), -0.5j * (zk - np.conj(zl))
        cw, sw = unit_root(k, L)
        X = E + (cw.astype(np.float64) + 1j * sw.astype(np.float64)) * O
        X[0], X[-1] = X[0].real, X[-1].real
        return X
    split = smooth_split_py(L)
    if split is None and L > 4096:
        re, im = dft_ld(v.astype(LD)[None, :], np.zeros((1, L), dtype=LD), L)
        X = re[0].astype(np.float64) + 1j * im[0].astype(np.float64)
    elif split is None:
        X = _dft_matrix64(L) @ v
    else:
        n1, n2 = split                                              # x[a n2 + b] -> X[k1 + n1 k2]
        Y = _dft_matrix64(n1) @ v.reshape(n1, n2)                   # (k1, b)
        c, s = unit_root((np.arange(n1)[:, None] * np.arange(n2)[None, :]) % L, L)
        tf = c.astype(np.float64) + 1j * s.astype(np.float64)
        if kind == "twiddle":
            tf[1, 1] *= 1.0 + 1e-13
        X = ((Y * tf) @ _dft_matrix64(n2)).T.reshape(L)             # (k2, k1) -> k1 + n1 k2
    X = X[: L // 2 + 1].copy()
    if kind == "bin_swap":
        kb = L // 5
        X[[kb, kb + 1]] = X[[kb + 1, kb]]
    return X


def planted_band_signal(X, mask32, n):
    """The half-size inverse (E + i O packing, ira_fftsmooth.hip smooth_value<HALF>) in float64 with the Nyquist bin's
    imaginary part left in: float64 band signal of even length n."""
    nt = n // 2
    Xm = np.asarray(X, dtype=np.complex128)[: nt + 1] * np.asarray(mask32, dtype=np.float32)[: nt + 1].astype(np.float64)
    Xm[0] = Xm[0].real
    i = np.arange(nt)
    a, b = Xm[i], np.conj(Xm[nt - i])
    c, s = unit_root(-i, n)
    Z = 0.5 * (a + b) + 1j * (c.astype(np.float64) + 1j * s.astype(np.float64)) * 0.5 * (a - b)
    z = np.conj(_dft_matrix64(nt) @ np.conj(Z)) / nt
    y = np.empty(n)
    y[0::2], y[1::2] = z.real, z.imag
    return y
