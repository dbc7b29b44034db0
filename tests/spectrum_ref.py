"""
Restatement of the spectrum post-processing kernels (ira_spectrum.hip: dB magnitude and angle, numpy.unwrap, group delay,
order statistics, summary statistics, log-frequency smoothing) in NumPy alone, for the tests: no torch, no scipy, nothing
of the package.  Every function takes the operands the kernel sees and returns what NumPy's definition gives for them.

Three kinds of quantity:
  * fixed sequences of float64 operations (unwrap, gradient, k-th smallest, the index fields of the statistics) are
    restated operation by operation, so that the kernels can be held to the BIT;
  * everything the kernels approximate (dB, angle, packed bins, sums, smoothing) is evaluated in np.longdouble (64-bit
    mantissa), together with the condition numbers the bounds need;
  * the bounds themselves (phase_bound, db_bound, PACKED_C, unwrap_bound, sums_bound, smooth_bound) are derived here from
    the kernels' operation counts, never from their output.
The inputs of the GPU tests are built here as well, so that tests/test_spectrum_ref_cpu.py can prove on a CPU that every
planted condition (ties, equal maxima, branch taken, margins) is what tests/test_gpu_spectrum.py assumes.
"""
import functools

import numpy as np

LD = np.longdouble
F32 = np.float32
U = 2.0 ** -53                    # unit roundoff of float64 (half an ulp, relative)
PI_LD = LD("3.14159265358979323846264338327950288")
KPI = 3.14159265358979323846      # the kernels' constant: the double nearest pi
LIB_ULP = 2.0                     # documented bound of the device library's float64 atan / atan2 / sincospi, in ulp
                                  # (HIP math API: 2 ulp; log2 / log10 / exp2 / exp10 / hypot are listed at 1, budgeted 2)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def ulp64(x):
    """Spacing of float64 at |x| (the smallest subnormal below the normal range)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)))


# ============================================================================================== dB magnitude and angle
def floor_lin_of(floor_db):
    return float(10.0 ** (float(floor_db) / 20.0))            # the entry point's std::pow(10.0, floor_db / 20.0)


def twiddle_ld(k, l):
    """exp(-i pi k / l) for 0 <= k <= l in long double, the argument reduced exactly (k against l) before pi enters."""
    k = np.asarray(k, dtype=np.int64)
    neg = 2 * k > l                                            # cos(pi - x) = -cos x, sin(pi - x) = sin x
    j = np.where(neg, l - k, k)                                # 0 <= j <= l/2
    swap = 4 * j > l                                           # cos x = sin(pi/2 - x)
    m = np.where(swap, l - 2 * j, 2 * j)                       # angle = pi m / (2 l), 0 <= m <= l/2
    ang = PI_LD * (m.astype(LD) / LD(2 * l))
    c0, s0 = np.cos(ang), np.sin(ang)
    c = np.where(swap, s0, c0)
    s = np.where(swap, c0, s0)
    c = np.where(neg, -c, c)
    c = np.where(2 * k == l, LD(0), c)
    s = np.where((k == 0) | (k == l), LD(0), s)
    return c, -s


def packed_bins_ld(z, L):
    """Bins 0 .. l of the real signal whose packed half-length transform is z[0 .. l-1] (l = L / 2): long-double real and
    imaginary parts and the conditioning weight (|Z[k]| + |Z[l-k]|) / |X[k]|."""
    l = L // 2
    k = np.arange(l + 1)
    zk = z[np.where(k == l, 0, k)]
    zl = z[np.where((k == 0) | (k == l), 0, l - k)]
    ar, ai, br, bi = zk.real.astype(LD), zk.imag.astype(LD), zl.real.astype(LD), zl.imag.astype(LD)
    er, ei = (ar + br) / 2, (ai - bi) / 2                      # E = (Z[k] + conj(Z[l-k])) / 2
    orr, oi = (ai + bi) / 2, (br - ar) / 2                     # O = -i (Z[k] - conj(Z[l-k])) / 2
    c, s = twiddle_ld(k, l)
    xr = er + (c * orr - s * oi)
    xi = ei + (c * oi + s * orr)
    xi = np.where((k == 0) | (k == l), LD(0), xi)
    a = np.hypot(ar, ai) + np.hypot(br, bi)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = a / np.hypot(xr, xi)
    return xr, xi, w, a


def mag_db_phase(spec, L, floor_db, packed=False):
    """spec: the element's complex128 values as the kernel reads them (L/2 + 1 bins, or the L/2 packed values first).
    Returns a dict: db and phase (long double), re / im of the bin, weight (1 for unpacked), floor32 (the float32 the floor
    gives), cls (0 below the floor, 1 at it, 2 above, 3 NaN, -1 within 2^-50 of it: the kernel compares rounded squares and
    may land on either side, both within the dB bound), lib_db / lib_phase (the bin takes the library routines)."""
    nb = L // 2 + 1
    spec = np.asarray(spec, dtype=np.complex128)
    fl = floor_lin_of(floor_db)
    if packed:
        xr, xi, w, a = packed_bins_ld(spec, L)
        re64, im64 = xr.astype(np.float64), xi.astype(np.float64)
    else:
        re64, im64 = spec.real[:nb].copy(), spec.imag[:nb].copy()
        xr, xi = re64.astype(LD), im64.astype(LD)
        w, a = np.ones(nb, dtype=LD), np.hypot(xr, xi)
    mag = np.hypot(xr, xi)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        m = np.where(np.isnan(mag), mag, np.maximum(mag, LD(fl)))       # numpy.maximum keeps NaN
        db = 20 * np.log10(m)
        phase = np.arctan2(xi, xr)
        p64 = re64 * re64 + im64 * im64                                 # the kernel's float64 power
    floor32 = F32(20 * np.log10(LD(fl)))
    tol = LD(2.0 ** -50)
    cls = np.where(np.isnan(mag), 3, np.where(mag == LD(fl), 1, np.where(mag < LD(fl) * (1 - tol), 0,
                                                                       np.where(mag > LD(fl) * (1 + tol), 2, -1))))
    lib_db = ~((p64 > 1.0e-280) & (p64 < 1.0e280) & (fl > 1.0e-140))
    ax, ay = np.abs(re64), np.abs(im64)
    with np.errstate(invalid="ignore"):
        lib_phase = ~((ax > 1.0e-300) & (ay > 1.0e-300) & (ax < 1.0e300) & (ay < 1.0e300))     # atan2_table's own test
    return dict(db=db, phase=phase, re=xr, im=xi, weight=w, absz=a, floor32=floor32, cls=cls, lib_db=lib_db,
                lib_phase=lib_phase, floor_lin=fl)


def db_bound(ref_db, lib):
    """Bound d of |float64 dB before its rounding to float32 - exact| for a bin above the floor.
    Table path, 3.0103 * log2_table(p) with p = re^2 + im^2:
      p: two products and a sum, relative (2 U + U)(1 + U) at most -> 10 / ln 10 * 3 U dB;
      log2_table: r = fma(m, 1/c, -1) one rounding of |r| <= 2^-7 (the table's reciprocal is rounded, its log2 is that of
      the ROUNDED value, so r carries no table error); series to r^6 in five fma, truncation r^7 / 7 < 2^-51 |r|; the
      sum's roundings are relative to s ~ 1 and enter times |r|: log1p error <= |r| (6 U) <= 2^-7 * 6 U; table log2_c
      from the library, LIB_ULP ulp of a value below 1 -> 2 LIB_ULP U; the final fma U (value below 1); e + ... and the
      product with 3.0103 one rounding each, relative: 2 U |dB| (and the constant's own rounding, 1 U |dB|).
    Library path (p beyond 1e+-280, or a floor below 1e-140): hypot and log10 at 2 ulp each, fmax exact, one product:
      (4 U) 20 / ln 10 for hypot, (4 U + U) |dB| for log10 and the product."""
    ref = np.abs(np.asarray(ref_db, dtype=np.float64))
    table = 3.0 * U * ref + 3.0103 * U * (6.0 / 128 + 2 * LIB_ULP + 1.0) + (10.0 / np.log(10.0)) * 3.0 * U * (1 + U)
    library = 5.0 * U * ref + (20.0 / np.log(10.0)) * 4.0 * U
    return np.where(lib, library, table)


def phase_bound(re, im, lib):
    """Absolute bound of the kernel's angle against atan2 in exact arithmetic, from the operations of atan2_table.
    With t = min / max, a = atan t, k the table index (t0 = k / 64), T = atan t0:
      t: one division, U t -> U t / (1 + t^2) <= 1.28 U a (a >= pi t / 4);
      t - t0 is exact (Sterbenz; k = 0: t itself); fma(t, t0, 1) and the division: 2 U |r|, and |r| <= 1/128 <= 1.0001 a
      for k >= 1; for k = 0 the divisor is exactly 1 and r = t;
      series: four fma at s ~ 1: U (1 + r^2 ...) |r s| <= 1.001 U a; truncation r^11 / 11 < 1e-24: nothing;
      final fma(r, s, T): U a;   T from the library: 2 LIB_ULP U T, and T <= a + 1/128;
    so E_a = U (5.3 a + 2 LIB_ULP (a + 1/128)) for t >= 1/129, 3 U a below (k = 0, T = 0 exactly).  In ulp of a that is
    up to 5.3 + 4 * 2 = 13.3 where t is just above 1/128 (T = 2 a: the table entry's two library ulp count twice) and a
    sits at the bottom of its binade, and 4.7 to 9.3 elsewhere; the part that is the kernel's own arithmetic is 5.3 U, at
    most 5.3 ulp and 2.7 ulp in the middle of a binade.  It is the worst case of every rounding at once; the measured worst
    is printed beside it.  Then the octant steps: pi/2 - a with the constant's error 6.2e-17 and one rounding, pi - a with
    1.3e-16 and one rounding.  Subnormal quotients (min / max below 2^-1022) add their absolute rounding.
    Library path: LIB_ULP ulp of the result (2 LIB_ULP U relative) and the same subnormal term."""
    re, im = np.asarray(re, dtype=LD), np.asarray(im, dtype=LD)
    ax, ay = np.abs(re), np.abs(im)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        t = (mn / mx).astype(np.float64)
        a = np.arctan(mn / mx).astype(np.float64)
    e = np.where(t >= 1.0 / 129, U * (5.3 * a + 2 * LIB_ULP * (a + 1.0 / 128)), 3.0 * U * a)
    r1 = np.where(ay > ax, np.pi / 2 - a, a)
    e = np.where(ay > ax, e + 6.2e-17 + U * r1, e)
    r2 = np.where(re < 0, np.pi - r1, r1)
    e = np.where(re < 0, e + 1.3e-16 + U * r2, e)
    e = np.where(lib, 2 * LIB_ULP * U * r2, e)
    return e + 4 * 2.0 ** -1074


# The packed branch: X[k] = E + W O with E, O = hermitian_parts(Z[k], Z[l-k]) and W by rotation.  With A = |Z[k]| + |Z[l-k]|:
#   E and O: one addition per component (the halving is exact): U |E| + U |O| <= U A / 2 + U A / 2 ... 1.0 U A in all;
#   W: start value from sincospi (2 LIB_ULP U), then one complex product per bin of the thread with the step (rc, rs), itself
#   2 LIB_ULP U off: each step adds 2 LIB_ULP U + sqrt(5) U (a complex product in float64).  A thread has at most
#   PACKED_STEPS = 16 bins: the launch has ceil(bins / 4096) blocks of 256 threads, so the grid stride covers the bins in
#   at most 16 trips.  W is then off by (4 + 16 (4 + 2.24)) U = 103.8 U;  W O: (103.8 + 2.24) U |O| <= 53.1 U A;
#   E + W O: U |X| <= U A per component pair.  Sum: 55.1 -> PACKED_C = 56.
PACKED_STEPS = 16
PACKED_C = 56.0
PACKED_MAX_WEIGHT = 1.0e3


def packed_bin_bound(absz):
    return PACKED_C * U * np.asarray(absz, dtype=np.float64)


def pack_real(x):
    """The packed half-length transform of an even-length real signal: Z = DFT_l(x[2m] + i x[2m+1]), float64."""
    x = np.asarray(x, dtype=np.float64)
    assert x.size % 2 == 0 and x.size >= 2
    return np.fft.fft(x[0::2] + 1j * x[1::2])


MP_LENGTHS = [0, 1, 2, 3, 4, 6, 510, 8190, 8192, 8194, 16386]
MP_PACKED_LENGTHS = [2, 4, 6, 8190, 8194, 16386]
# -300 dB is a floor of 1e-15 and still takes the table; only a floor below 1e-140 (-2800 dB) reaches the branch that sends
# EVERY bin through the library's hypot and log10, so -2900 dB stands beside the three everyday floors
MP_FLOORS = [-120.0, -300.0, 0.0, -2900.0]


def planted_bins():
    """(re, im) pairs every table index, octant, sign of zero, library fallback and floor tie goes through."""
    inf, nan = np.inf, np.nan
    out = []
    for a in (1.0, 3.7e-9, 2.5e11):
        for s1 in (1.0, -1.0):
            for s2 in (1.0, -1.0):
                out += [(s1 * a, s2 * 0.0), (s1 * 0.0, s2 * a), (s1 * a, s2 * a)]
    out += [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)]
    signs = [(1, 1), (-1, 1), (1, -1), (-1, -1)]
    for k in range(65):                                        # the table knots k/64 and midway between them
        for j, t in enumerate((k / 64.0, (k + 0.5) / 64.0)):
            if t > 1.0:
                continue
            s1, s2 = signs[(2 * k + j) % 4]
            m = 2.0 ** ((7 * k) % 41 - 20)
            out += [(s1 * m, s2 * t * m), (s2 * t * m, s1 * m)]
            out += [(s1 * m, s2 * np.nextafter(t, 2.0) * m), (s1 * m, s2 * np.nextafter(t, -1.0) * m)]
    out += [(1.0, 2.0 ** -1010), (-3.0, 3 * 2.0 ** -1005), (2.0 ** -1008, -5.0), (2.0 ** -1030, 1.0 * 2.0 ** 20),
            (2.0 ** 40, 2.0 ** -1000), (7.0e299, 7.0e-299), (-7.0e-299, 7.0e299)]             # min / max below 2^-1000
    out += [(1.0e-305, 1.0), (1.0e-310, -1.0e-305), (-1.0e-305, 1.0e-305), (3.0e-301, 2.0e-301), (5e-324, 5e-324),
            (1.0e301, 1.0), (1.0e305, -1.0e302), (-1.0e301, -1.0e301), (1.0, 1.0e300), (1.0e-300, 1.0)]   # library branch
    out += [(inf, 1.0), (-inf, 1.0), (1.0, inf), (1.0, -inf), (inf, inf), (-inf, inf), (-inf, -inf), (inf, -inf),
            (inf, 0.0), (inf, -0.0), (-inf, 0.0), (-inf, -0.0), (0.0, inf), (-0.0, -inf),
            (nan, 1.0), (1.0, nan), (nan, inf), (nan, nan), (-nan, 0.0), (0.0, nan)]
    for fdb in MP_FLOORS:                                      # bins AT the floor, just above and just below it
        f = floor_lin_of(fdb)
        out += [(f, 0.0), (0.0, -f), (-f, -0.0), (np.nextafter(f, 2.0), 0.0), (0.0, np.nextafter(f, 0.0)),
                (f * (1 + 2.0 ** -20), 0.0), (f * (1 - 2.0 ** -20), 0.0)]
    return np.array([complex(a, b) for a, b in out])


def floor_tie_bins(floor_db):
    f = floor_lin_of(floor_db)
    return np.array([complex(f, 0.0), complex(0.0, -f), complex(-f, -0.0)])


def random_bins(rng, n):
    """Magnitudes spread over 2^+-60, angles uniform."""
    mag = 2.0 ** rng.uniform(-60.0, 60.0, n)
    ang = rng.uniform(-np.pi, np.pi, n)
    return mag * np.cos(ang) + 1j * (mag * np.sin(ang))


@functools.lru_cache(maxsize=None)
def mag_phase_batch():
    """[(L, spectrum)] of the ragged unpacked batch; the planted bins sit in every element long enough, around the 4096-bin
    block edge of the long ones."""
    rng = np.random.default_rng(20240611)
    pl = planted_bins()
    out = []
    for L in MP_LENGTHS:
        nb = L // 2 + 1
        s = random_bins(rng, nb)
        if nb >= 4096:
            at = 4096 - pl.size // 2 if nb >= 4096 + pl.size else nb - pl.size
            s[at : at + pl.size] = pl
        elif nb >= 256:
            s[:] = pl[rng.permutation(pl.size)[:nb]]
        else:
            s[:] = pl[rng.permutation(pl.size)[:nb]] if L % 4 == 2 else s
        out.append((L, s))
    return out


def mag_phase_packed_batch():
    """[(L, values, packed)]: the even lengths packed (built from real decaying noise), odd unpacked ones between them."""
    rng = np.random.default_rng(77)
    out = []
    for i, L in enumerate(MP_PACKED_LENGTHS):
        x = rng.standard_normal(L) * np.exp(-np.arange(L) / (0.2 * L + 3.0)) * 2.0 ** (5 * i - 12)
        z = np.zeros(L // 2 + 1, dtype=np.complex128)
        z[: L // 2] = pack_real(x)
        z[L // 2] = complex(np.nan, np.nan)                    # never read by a packed element
        out.append((L, z, 1, x))
        Lo = [1, 3, 511, 8191][i % 4]
        out.append((Lo, random_bins(rng, Lo // 2 + 1), 0, None))
    return out


# ============================================================================================================ unwrap
def unwrap_corrections(p):
    """numpy.unwrap's ph_correct (period 2 pi, discont pi), operation by operation in float64."""
    p = np.asarray(p, dtype=np.float64)
    period = 2.0 * KPI
    dd = p[1:] - p[:-1]
    a = dd - (-KPI)
    with np.errstate(invalid="ignore"):
        md = np.fmod(a, period)                                # numpy's floor-mod for a positive divisor
        md = np.where(md != 0.0, np.where(md < 0.0, md + period, md), 0.0)
        ddmod = md + (-KPI)
        ddmod = np.where((ddmod == -KPI) & (dd > 0.0), KPI, ddmod)
        corr = ddmod - dd
        corr = np.where(np.abs(dd) < KPI, 0.0, corr)
    return corr


def unwrap(p):
    """numpy.unwrap(p): the corrections summed one after another in float64, as numpy's cumsum does."""
    p = np.asarray(p, dtype=np.float64)
    out = p.copy()
    acc = np.float64(0.0)
    first = True
    for i, c in enumerate(unwrap_corrections(p)):
        acc = c if first else acc + c
        first = False
        out[i + 1] = p[i + 1] + acc
    return out


def unwrap_ld(p):
    """The same corrections (they are float64 values) summed in long double: (unwrapped, largest |prefix sum|)."""
    p = np.asarray(p, dtype=np.float64)
    cs = np.concatenate([[LD(0)], np.cumsum(unwrap_corrections(p).astype(LD))])
    return p.astype(LD) + cs, float(np.max(np.abs(cs)))


UW_THREADS, UW_PER, UW_WAVE = 1024, 4, 64
UW_TILE = UW_THREADS * UW_PER


def unwrap_tree(p):
    """The kernel's order of the same additions: four bins per thread, a 64-lane inclusive scan in six doubling steps, the
    wave totals one after another, the tile carry from the last thread -- float64, so the device result is these bits."""
    p = np.asarray(p, dtype=np.float64)
    n = p.size
    corr = np.concatenate([[0.0], unwrap_corrections(p)])
    out = np.empty(n)
    carry = np.float64(0.0)
    for base in range(0, n, UW_TILE):
        c = np.zeros(UW_TILE)
        v = np.zeros(UW_TILE)
        m = min(UW_TILE, n - base)
        c[:m], v[:m] = corr[base : base + m], p[base : base + m]
        c = c.reshape(UW_THREADS, UW_PER).copy()
        for r in range(1, UW_PER):
            c[:, r] += c[:, r - 1]
        incl = c[:, UW_PER - 1].reshape(-1, UW_WAVE).copy()
        o = 1
        while o < UW_WAVE:
            nxt = incl.copy()
            nxt[:, o:] = incl[:, o:] + incl[:, :-o]
            incl, o = nxt, o * 2
        excl = np.concatenate([np.zeros((incl.shape[0], 1)), incl[:, :-1]], axis=1)
        before = np.zeros(incl.shape[0])
        for w in range(1, incl.shape[0]):
            before[w] = before[w - 1] + incl[w - 1, -1]
        add = (carry + (before[:, None] + excl)).reshape(-1)
        u = v.reshape(UW_THREADS, UW_PER) + (c + add[:, None])
        out[base : base + m] = u.reshape(-1)[:m]
        carry = c[-1, -1] + add[-1]
    return out


def unwrap_bound(ref_ld, max_prefix, n):
    """|device - long-double scan| for ANY order the kernel may add the (bit-identical) corrections in: a bin's correction
    goes through at most 3 additions in its thread, 6 in the wave scan, 15 over the wave totals, and one each for
    before + excl, carry + ., c + add: 27, plus one per earlier tile for the carry; every partial sum is a difference of
    two prefix sums, so at most 2 max|prefix| in size: (27 + tiles) U 2 max|prefix|, and U |result| for the last addition."""
    tiles = (n + UW_TILE - 1) // UW_TILE
    return (27 + tiles) * U * 2.0 * max_prefix * (1 + 64 * U) + U * np.abs(np.asarray(ref_ld, dtype=np.float64)) * (1 + 2 * U)


UNWRAP_BINS = [1, 2, 3, 4, 5, 4095, 4096, 4097, 8191, 8192, 8193, 12289]


def _step_positions(n):
    """Where steps are planted: tile edges, inside a thread's four bins, between threads, the wave edge, the last bin."""
    want = [1, 2, 3, 4, 5, 6, 7, 8, 255, 256, 257, 1023, 1024, 4094, 4095, 4096, 4097, 8191, 8192, 8193, n - 2, n - 1]
    return sorted({i for i in want if 1 <= i < n})


UNWRAP_NAMES = [f"{k} n={n}" for n in UNWRAP_BINS for k in ("steps", "winding", "mixed")] + [f"caller n={n}" for n in (5, 4097, 12289)]


@functools.lru_cache(maxsize=None)
def unwrap_cases():
    """[(name, phase)]: wrapped phases (|p| <= pi) with exact +-pi, just-inside and +-2 pi steps at every structural
    position, a steady winding whose carry reaches thousands of radians, and a caller's array with |dd| up to 50."""
    out = []
    inside = np.nextafter(KPI, 0.0)
    steps = [KPI, -KPI, inside, -inside, 2 * KPI, -2 * KPI]
    for n in UNWRAP_BINS:
        rng = np.random.default_rng(1000 + n)
        # (a) planted steps on a quiet phase: values are chosen so that the DIFFERENCE is the step exactly
        p = np.zeros(n)
        pos = _step_positions(n)
        lvl = 0.0
        j = 0
        for i in range(1, n):
            if i in pos:
                s = steps[j % len(steps)]
                j += 1
                nxt = lvl + s
                if abs(nxt) > 2 * KPI or (nxt - lvl) != s:     # keep the level small and the step exact
                    s = -s
                    nxt = lvl + s
                lvl = nxt
            p[i] = lvl
        out.append((f"steps n={n}", p))
        # (b) a steadily winding wrapped phase with noise: many corrections, carry of thousands of radians
        k = np.arange(n)
        w = -2.9 * k + 0.2 * rng.standard_normal(n)
        out.append((f"winding n={n}", np.angle(np.exp(1j * w))))
        # (c) the same with exact 0 | pi | 0 and pi | -pi neighbours around the structural positions
        q = np.angle(np.exp(1j * (1.7 * k + 0.1 * rng.standard_normal(n))))
        for i in pos:
            if i + 1 < n:
                q[i - 1], q[i] = (0.0, KPI) if i % 2 else (KPI, -KPI)
        out.append((f"mixed n={n}", q))
    rng = np.random.default_rng(5)
    for n in (5, 4097, 12289):
        out.append((f"caller n={n}", rng.uniform(-25.0, 25.0, n)))               # |dd| up to 50: the library fmod branch
    return out


# ======================================================================================================== group delay
def gd_axis(nbins, val, sr):
    return (2.0 * np.pi) * ((np.arange(nbins, dtype=np.float64) * val) / sr)


def gd_is_uniform(nbins, val, sr):
    """numpy.gradient's rule: the uniform formula only if every diff of the coordinate array is bit-identical."""
    d = np.diff(gd_axis(nbins, val, sr))
    return bool(d.size == 0 or np.all(d == d[0]))


def gradient(phase, nbins, val, sr):
    """-numpy.gradient(phase, w), w = gd_axis: both formulas written out in float64, operation by operation."""
    f = np.asarray(phase, dtype=np.float64)
    assert f.size == nbins >= 2
    w = gd_axis(nbins, val, sr)
    d = w[1:] - w[:-1]
    g = np.empty(nbins)
    g[0] = (f[1] - f[0]) / d[0]
    g[-1] = (f[-1] - f[-2]) / d[-1]
    if nbins > 2:
        if gd_is_uniform(nbins, val, sr):
            g[1:-1] = (f[2:] - f[:-2]) / (2.0 * d[0])
        else:
            dx1, dx2 = d[:-1], d[1:]
            a = -(dx2) / (dx1 * (dx1 + dx2))
            b = (dx2 - dx1) / (dx1 * dx2)
            c = dx1 / (dx2 * (dx1 + dx2))
            g[1:-1] = a * f[:-2] + b * f[1:-1] + c * f[2:]
    return -g


GD_SR = 48000.0
GD_NFFT = [2, 4, 6, 512, 1000, 4800, 48000]
# The double nearest 2 pi ends in three zero bits, so k * (2 pi) is exact up to k = 8: with a step that makes (k * step) / sr a
# power-of-two multiple of k, the nine-bin axis of a 16-point transform is uniform to the bit -- the longest there is at this
# sample rate; seven interior bins take the uniform formula.
GD_UNIFORM_LONG = [(16, 46.875), (16, 3000.0), (16, 1.0)]


def gd_cases():
    """[(n_fft, bin step)]: every length with the step 1.0 and with the rfftfreq step 1 / (n (1 / sr))."""
    out = []
    for n in GD_NFFT:
        out.append((n, 1.0))
        out.append((n, 1.0 / (n * (1.0 / GD_SR))))
    return out + GD_UNIFORM_LONG


def gd_phase(nbins, seed):
    rng = np.random.default_rng(seed)
    k = np.arange(nbins)
    return -0.37 * k + 40.0 * np.sin(k / 9.0) + rng.standard_normal(nbins)


# ==================================================================================================== order statistics
def sort_key(v):
    """The order-preserving 64-bit image of the NUMBERS among float64: -0.0 before +0.0, -inf first, +inf last.  (NaNs have no
    place in it: kth sets them aside.)"""
    u = bits64(v)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def unkey(k):
    k = np.asarray(k, dtype=np.uint64)
    u = np.where(k >> np.uint64(63) != 0, k & np.uint64((1 << 63) - 1), ~k)
    return u.view(np.float64)


QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


def kth(values, ranks):
    """sorted(values)[rank], ranks clamped to [0, n-1]: the numbers in key order (so -0.0 before +0.0), then every NaN,
    whatever its sign or payload, as numpy.sort places them; a rank that lands on a NaN gives the quiet NaN QNAN (numpy.sort
    keeps some payload there, in no defined order), and so does an empty segment."""
    v = np.asarray(values, dtype=np.float64)
    r = np.asarray(ranks, dtype=np.int64)
    if v.size == 0:
        return np.full(r.shape, QNAN)
    num = v[~np.isnan(v)]
    ordered = np.concatenate([unkey(np.sort(sort_key(num))), np.full(v.size - num.size, QNAN)])
    return ordered[np.clip(r, 0, v.size - 1)]


OS_CAP = 1536


def values_with_top16(rng, top16, n):
    """n distinct positive doubles whose key shares its top 16 bits (sign, exponent, four mantissa bits)."""
    low = (rng.choice(1 << 40, size=n, replace=False).astype(np.uint64) << np.uint64(8)) | rng.integers(0, 256, n).astype(np.uint64)
    return ((np.uint64(top16) << np.uint64(48)) | low).view(np.float64)


@functools.lru_cache(maxsize=None)
def order_stat_segments():
    """[(name, values)]: the sizes 1, 2, 1535 .. 16385 and 100003 with the contents that stress the radix select."""
    rng = np.random.default_rng(99)
    segs = [("one", np.array([42.0])), ("two", np.array([3.0, -3.0])), ("empty", np.zeros(0))]
    for n in (1535, 1536, 1537, 16383, 16384, 16385):
        segs.append((f"wide {n}", rng.standard_normal(n) * 2.0 ** rng.integers(-400, 400, n)))   # every leading digit
    segs.append(("all equal 100003", np.full(100003, -7.25)))
    two = np.where(rng.random(16385) < 0.5, 1.5, np.nextafter(1.5, 2.0))
    segs.append(("two values 16385", two))
    for cnt in (OS_CAP, OS_CAP + 1):                          # the bucket after two digits holds exactly cnt values
        inside = values_with_top16(rng, 0x4005, cnt)          # 0x4005...: values in [2.625, 2.75)
        rest = np.concatenate([rng.uniform(-100.0, 2.0, 9000), rng.uniform(3.0, 100.0, 9000 - cnt)])
        segs.append((f"bucket {cnt}", rng.permutation(np.concatenate([inside, rest]))))
    z = np.where(rng.random(1537) < 0.5, 0.0, -0.0)
    z[::7] = rng.standard_normal(z[::7].size) * 1e-3
    segs.append(("signed zeros 1537", z))
    inf = rng.standard_normal(1536)
    inf[::5], inf[1::5] = np.inf, -np.inf
    segs.append(("infinities 1536", inf))
    sub = rng.integers(-4000, 4000, 16384).astype(np.float64) * 5e-324
    segs.append(("subnormals 16384", sub))
    lowbyte = (np.float64(1.0).view(np.uint64) + rng.integers(0, 256, 1535).astype(np.uint64)).view(np.float64)
    segs.append(("lowest byte 1535", lowbyte))
    nans = rng.standard_normal(1537)
    nans[[3, 700, 1500]] = np.nan
    nans[[4, 701]] = -np.nan                                  # sign bit set: x86 arithmetic's own default NaN
    nans[[5]] = np.array([0x7FF8000000000123], dtype=np.uint64).view(np.float64)
    segs.append(("nans 1537", nans))
    return segs


def fullest_bucket(v):
    """[lo, hi): the sorted positions of the values that share the most frequent leading 16 key bits (two digits)."""
    top = np.sort(sort_key(v)) >> np.uint64(48)
    vals, first, cnt = np.unique(top, return_index=True, return_counts=True)
    j = int(np.argmax(cnt))
    return int(first[j]), int(first[j] + cnt[j])


def order_stat_ranks(n, kind, v=None):
    """Eight ranks: 'spread' (more than four distinct buckets: no compaction), 'median' (clustered: compaction), 'edges'
    (below 0 and above n - 1, clamped), 'bucket' (all inside the fullest two-digit bucket of v, its LAST positions first:
    one leader, so only the bucket's size decides the compaction, and a list that lost any one value misses them)."""
    if kind == "bucket":
        lo, hi = fullest_bucket(v) if n else (0, 0)
        mid = lo + (hi - lo) // 2
        return np.array([hi - 1, hi - 2, hi - 3, mid, mid + 1, lo, lo + 1, hi - 1], dtype=np.int64)
    if kind == "spread":
        return np.array([0] + [(j * n) // 8 for j in range(1, 7)] + [n - 1], dtype=np.int64)
    if kind == "median":
        return np.array([n // 2 + d for d in (-3, -2, -1, 0, 0, 1, 2, 3)], dtype=np.int64)
    return np.array([-5, -1, 0, n // 3, n - 2, n - 1, n, n + 100], dtype=np.int64)


# ================================================================================================ summary statistics
def stats(mag_db, L, val, f_min, f_max, probe, dtype=LD):
    """The eight-field record of stats_kernel and the sums of absolute terms its bound needs.
    Frequencies are float32(k * val), the comparisons float32, argmax / argmin first-wins with numpy's NaN rule, the sums
    in `dtype` (long double for the reference, float64 to compare the expressions with NumPy's own)."""
    n = L // 2 + 1
    m = np.asarray(mag_db, dtype=F32)[:n]
    f = (np.arange(n, dtype=np.float64) * float(val)).astype(F32)
    sel = (f >= F32(f_min)) & (f <= F32(f_max))
    idx = np.flatnonzero(sel)
    rec = np.zeros(8)
    rec[0] = idx.size
    with np.errstate(over="ignore", invalid="ignore"):
        lin = dtype(10) ** (m[idx].astype(dtype) / dtype(20))
        sfl = f[idx].astype(dtype) * lin
    if idx.size:
        sub = m[idx]
        isn = np.isnan(sub)
        j = int(np.flatnonzero(isn)[0]) if isn.any() else int(np.flatnonzero(sub == sub.max())[0])
        rec[1] = idx[j]
        rec[5] = float(f[idx[0]])
    rec[2] = float(f[int(rec[1])])
    d = np.abs(f - F32(probe))
    assert d.dtype == F32
    i1k = int(np.flatnonzero(d == d.min())[0])
    rec[6], rec[7] = i1k, float(m[i1k])
    s3, s4 = np.sum(sfl), np.sum(lin)
    rec[3], rec[4] = float(s3), float(s4)
    return rec, dict(s3=s3, s4=s4, abs3=float(np.sum(np.abs(sfl))), abs4=float(np.sum(np.abs(lin))), n_in=int(idx.size))


# exp10_table's unit error, in ulp (2^-52) of the result: the table entry from the library's exp2 (1 ulp listed -> 1.0),
# the final fma (0.5), the truncated series p^6 / 720 <= 3.4e-17 (0.16), and the roundings of r, p, s that enter times
# |p| <= 0.0054 (0.02): 1.68 -> 1.7.  (A correctly rounded table gives 1.2; the measured 1.03 of a host build sits below.)
EXP10_U = 1.7


def sums_bound(abs_sum, n_in):
    """2^-53 n_in S_abs for the additions in any order (and the product f * lin), EXP10_U 2^-52 S_abs for the terms."""
    return U * n_in * abs_sum + EXP10_U * 2.0 ** -52 * abs_sum


ST_BINS = [1, 2, 1025, 16384, 16385, 40001]


ST_KINDS = ["plain", "edges", "empty", "below", "above", "extremes", "nan"]


@functools.lru_cache(maxsize=None)
def stats_cases():
    """[dict(name, mag, L, val, f_min, f_max, probe)] -- the calls share (f_min, f_max, probe) per launch, so cases come in
    groups keyed by those three; each group is one ragged batch over ST_BINS with a different val per element."""
    groups = []
    nanp, nann, pay = 0x7FC00000, 0xFFC00000, 0x7FC00123      # NaN bit patterns: both signs and a payload
    for gi, kind in enumerate(ST_KINDS):
        rng = np.random.default_rng(300 + gi)
        elems = []
        for ei, nb in enumerate(ST_BINS):
            L = 2 * (nb - 1) + (ei % 2 if nb > 1 else 0)       # L // 2 + 1 == nb, odd and even lengths
            val = [1.0, 24000.0, 46.875, 1.46484375, 2.9296875, 0.6][ei]
            m = (-30.0 + 12.0 * rng.standard_normal(nb)).astype(F32)
            f = (np.arange(nb, dtype=np.float64) * val).astype(F32)
            elems.append([L, val, m, f])
        if kind == "plain":                                    # two equal maxima, probe midway between two frequencies
            f_min, f_max = 20.0, 20000.0
            for L, val, m, f in elems:
                inr = np.flatnonzero((f >= F32(f_min)) & (f <= F32(f_max)))
                if inr.size >= 4:
                    m[inr[inr.size // 3]] = m[inr[2 * inr.size // 3]] = F32(50.0)
            probe = float((np.float64(elems[2][3][21]) + np.float64(elems[2][3][22])) / 2)     # 46.875 * 21.5: exact
        elif kind == "edges":                                  # f_min and f_max ARE frequencies; maxima at both ends
            f_min, f_max = float(F32(46.875 * 2)), float(F32(46.875 * 400))
            probe = 1000.0
            for ei, (L, val, m, f) in enumerate(elems):
                inr = np.flatnonzero((f >= F32(f_min)) & (f <= F32(f_max)))
                if inr.size >= 2:
                    m[inr[0] if ei % 2 else inr[-1]] = F32(77.0)
                    if inr[0] > 0:
                        m[inr[0] - 1] = F32(99.0)              # just outside: must not win
                    if inr[-1] + 1 < m.size:
                        m[inr[-1] + 1] = F32(99.0)
        elif kind == "empty":                                  # a range that selects nothing anywhere
            f_min, f_max, probe = 0.25, 0.5, 1000.0
        elif kind == "below":
            f_min, f_max, probe = 0.0, 1.0e9, -5.0
        elif kind == "above":
            f_min, f_max, probe = 0.0, 1.0e9, 1.0e9
        elif kind == "extremes":                               # -inf, -0.0, and both sides of the |y| < 15 switch
            f_min, f_max, probe = 10.0, 22000.0, 1000.0
            for L, val, m, f in elems:
                inr = np.flatnonzero((f >= F32(f_min)) & (f <= F32(f_max)))
                sp = [F32(-np.inf), F32(-0.0), F32(299.0), F32(-299.0), F32(301.0), F32(-301.0), F32(299.99), F32(-300.01)]
                for j, v in zip(inr[1::3], sp):
                    m[j] = v
        else:                                                  # NaNs of both signs and payloads among finite values
            f_min, f_max, probe = 20.0, 20000.0, 1000.0
            for ei, (L, val, m, f) in enumerate(elems):
                inr = np.flatnonzero((f >= F32(f_min)) & (f <= F32(f_max)))
                if inr.size >= 6:
                    a, b, c = inr[inr.size // 2], inr[inr.size // 2 + 2], inr[-1]
                    m.view(np.uint32)[[a, b, c]] = [(nann, nanp, pay), (nanp, nann, pay), (pay, nanp, nann), (nann, pay, nanp)][ei % 4]
                    m[inr[0]] = F32(120.0)                     # a large finite value BEFORE the NaNs: NaN still wins
        groups.append(dict(name=kind, f_min=f_min, f_max=f_max, probe=probe, elems=[(L, val, m) for L, val, m, _ in elems]))
    return groups


# ============================================================================================== log-frequency smoothing
LS_MAX = 2048
LS_2048_NSEL = 3561               # bins from k_lo = 14 of a 32768-point transform at 256 per octave: exactly 2048 grid points,
                                  # one more bin gives 2049 (asserted in tests/test_spectrum_ref_cpu.py)


def ls_freq(k, fstep):
    return (np.asarray(k, dtype=np.float64) * float(fstep)).astype(F32).astype(np.float64)


def ls_geometry(k_lo, nsel, fstep, bpo):
    """(a, b, count) as the reference computes them on the host, float64."""
    with np.errstate(divide="ignore"):
        a = float(np.log2(ls_freq(k_lo, fstep)))
        b = float(np.log2(ls_freq(k_lo + nsel - 1, fstep)))
    bpo = int(max(16, bpo))
    count = int(max(8, np.ceil((b - a) * bpo))) + 1
    return a, b, count


def _interp(x, xp, fp):
    """numpy.interp(x, xp, fp) for increasing xp, in the dtype of the operands: slope * (x - xp[j]) + fp[j]."""
    j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, xp.size - 2) if xp.size > 1 else np.zeros(x.size, dtype=np.int64)
    if xp.size == 1:
        return np.full(x.shape, fp[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])
        v = slope * (x - xp[j]) + fp[j]
    v = np.where(x <= xp[0], fp[0], v)
    return np.where(x >= xp[-1], fp[-1], v)


def log_smooth(curve, k_lo, nsel, fstep, window, bpo, through_f32, dtype=LD, parts=False):
    """The smoothed float32 values of the nsel selected bins (curve[k_lo : k_lo + nsel]).  The grid exponents are NumPy's
    float64 linspace (the operands the kernel derives them from are float64); everything after is in `dtype`.
    parts=True also returns the two inner curves before their float32 rounding (for the tie margins)."""
    a, b, count = ls_geometry(k_lo, nsel, fstep, bpo)
    y = np.linspace(a, b, count)
    grid = dtype(2) ** y.astype(dtype)
    fs = ls_freq(k_lo + np.arange(nsel), fstep).astype(dtype)
    ms = np.asarray(curve, dtype=F32)[k_lo : k_lo + nsel].astype(dtype)
    on = _interp(grid, fs, ms)
    on_r = on.astype(F32).astype(dtype) if through_f32 else on
    sm = np.convolve(on_r, np.ones(window, dtype=dtype) / dtype(window), mode="same") if window <= count else None
    assert sm is not None and sm.size == count
    sm_r = sm.astype(F32).astype(dtype) if through_f32 else sm
    out = _interp(fs, grid, sm_r)
    if not parts:
        return out.astype(F32)
    # Conditioning on the GRID: the interpolations are linear in their ordinates but not in their abscissae, and the kernel's
    # grid is the library's exp2, GRID_D = 2 LIB_ULP U relative off this one.  Onto the grid a point moves by GRID_D x along
    # a segment of slope s: |s| x GRID_D, carried through the (convex) average and interpolation at most once: g_on is its
    # maximum.  Back onto the bins both ends of the grid cell move: the offset x - xg[j] by GRID_D xg and the cell's width
    # by 2 GRID_D xg, which the slope multiplies: 3 GRID_D xg |s| per bin (t_back).  Zero beyond the ends of "same" makes
    # the first and last half-windows steep, which is where t_back matters.
    gd = 2 * LIB_ULP * U
    g_on = 0.0
    if nsel > 1:
        j = np.clip(np.searchsorted(fs, grid, side="right") - 1, 0, nsel - 2)
        s_on = np.abs((ms[j + 1] - ms[j]) / (fs[j + 1] - fs[j]))
        g_on = float(np.max(s_on * grid)) * gd
    t_back = np.zeros(nsel)
    if grid[-1] > grid[0]:
        j = np.clip(np.searchsorted(grid, fs, side="right") - 1, 0, count - 2)
        s_b = np.abs((sm_r[j + 1] - sm_r[j]) / (grid[j + 1] - grid[j]))
        t_back = (3 * gd * s_b * grid[j + 1]).astype(np.float64)
    return dict(out32=out.astype(F32), out=out, on=on, sm=sm, g_on=g_on, t_back=t_back, count=count)


def smooth_bound(parts, window, cmax, inner=False):
    """(window + 8) U max|curve| for the float64 evaluation of two linear interpolations and a window-term average (the
    issue's figure, linear in the ordinates), the grid's conditioning (g_on, t_back: see log_smooth), and half a float32
    ulp of the result for the final rounding.  inner=True: the bound of the two inner curves (no t_back, no rounding)."""
    base = (window + 8) * U * cmax + parts["g_on"]
    if inner:
        return base
    r = np.abs(np.asarray(parts["out"], dtype=np.float64))
    return base + parts["t_back"] + 2.0 ** -24 * r * (1 + 2.0 ** -20) + 2.0 ** -150


def tie_margin32(v):
    """Distance of each long-double value from the nearest float32 rounding tie (midpoint of neighbouring floats)."""
    v = np.asarray(v, dtype=LD)
    f = v.astype(F32)
    lo = np.where(f.astype(LD) > v, np.nextafter(f, F32(-np.inf)), f)
    hi = np.nextafter(lo, F32(np.inf))
    mid = (lo.astype(LD) + hi.astype(LD)) / 2
    return np.abs(v - mid).astype(np.float64)


def smooth_curve(nbins, fstep, seed):
    """A dB curve that is smooth in log frequency (|d curve / d ln f| below half its size: the grid's own float64 rounding,
    which the two interpolations multiply by the bin index, stays inside the bound)."""
    rng = np.random.default_rng(seed)
    k = np.arange(nbins)
    lf = np.log(np.maximum(k, 1) * fstep)
    c = -40.0 + 9.0 * np.sin(1.3 * lf + rng.uniform(0, 6)) + 6.0 * np.cos(0.7 * lf + rng.uniform(0, 6)) - 1.5 * lf
    return c.astype(F32)


def smooth_cases():
    """[dict(name, window, bpo, through, curves=[dict(nbins, stride, col, ncols, k_lo, nsel, fstep, seed)])]: one entry per
    launch, several curves of different geometry in each."""
    fstep = 48000.0 / 32768
    n2048 = LS_2048_NSEL
    geo = [
        dict(nbins=40, stride=1, k_lo=3, nsel=2, fstep=fstep),                    # nsel 2, 9 grid points
        dict(nbins=40, stride=1, k_lo=5, nsel=1, fstep=fstep),                    # nsel 1
        dict(nbins=64, stride=1, k_lo=8, nsel=9, fstep=fstep),                    # span of one octave: 8 -> 16
        dict(nbins=2049, stride=1, k_lo=1, nsel=2048, fstep=1.0),                 # first and last bins are grid points: 1, 2048
        dict(nbins=1500, stride=7, col=3, k_lo=14, nsel=1200, fstep=fstep),       # a column of a (bins, 7) matrix
        dict(nbins=16385, stride=1, k_lo=14, nsel=13640, fstep=fstep),            # 20 Hz .. 20 kHz of a 32768-point transform
    ]
    out = []
    for wi, window in enumerate([1, 2, 8, 9]):
        for through in (False, True):
            out.append(dict(name=f"w{window} f32={int(through)}", window=window, bpo=48 if window > 2 else 16, through=through,
                            # (one selected bin and an even window: first == last frequency picks sm[0] or sm[count-1], which
                            # differ then, by the last bit of exp2(log2(f)) -- ill-posed in the reference itself)
                            curves=[dict(g, seed=10 * wi + j) for j, g in enumerate(geo)
                                    if not (g["nsel"] == 1 and window % 2 == 0)]))
    big = dict(nbins=14 + n2048 + 3, stride=1, k_lo=14, nsel=n2048, fstep=fstep, seed=77)
    for through in (False, True):
        out.append(dict(name=f"grid 2048 f32={int(through)}", window=9, bpo=256, through=through, curves=[big, dict(geo[2], seed=78)]))
        out.append(dict(name=f"window == count f32={int(through)}", window=9, bpo=16, through=through,
                        curves=[dict(geo[0], seed=79), dict(geo[2], seed=80)]))
    return out, dict(big, nsel=n2048 + 1, nbins=big["nbins"] + 1)


def smooth_case_arrays(curve_spec):
    """(flat float32 storage, offset of bin 0 within it) of one curve: a column of a (nbins, stride) matrix."""
    stride, col = curve_spec["stride"], curve_spec.get("col", 0)
    c = smooth_curve(curve_spec["nbins"], curve_spec["fstep"], curve_spec["seed"])
    mat = np.empty((curve_spec["nbins"], stride), dtype=F32)
    for j in range(stride):
        mat[:, j] = c if j == col else smooth_curve(curve_spec["nbins"], curve_spec["fstep"], 1000 + curve_spec["seed"] + j)
    return mat, col
