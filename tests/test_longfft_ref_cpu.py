"""The long-FFT reference (tests/longfft_ref.py) proved on a CPU: the recursion against the defining sum, exactly formed
impulse spectra, the round trip, the derived bounds against numpy's own float64 transform on every input family and length
list tests/test_gpu_longfft_edges.py uses (pocketfft's worst error / bound ratio is printed), every planted error against the
bound, and the path predictions against engine_plan.plan_rfft with hand-built Switches.  No device, no library."""
import numpy as np
import pytest

import longfft_ref as R
from audio_analysis_amd.engine_plan import BLUESTEIN, SMOOTH, Switches, plan_rfft

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)


def _c(re, im):
    return np.asarray(re, dtype=np.float64) + 1j * np.asarray(im, dtype=np.float64)


def _norm(a):
    return float(np.sqrt(np.sum(np.asarray(a, dtype=np.float64) ** 2)))


def test_recursion_equals_the_direct_sum():
    """Every L from 1 to 64 and a sample of larger composite and prime lengths: a few long-double ulps * log L."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for L in list(range(1, 65)) + [97, 100, 194, 243, 360, 625, 1000, 1021, 1024, 2 * 3 * 5 * 7 * 11]:
        xr, xi = rng.standard_normal((2, L)).astype(LD), rng.standard_normal((2, L)).astype(LD)
        ar, ai = R.dft_ld(xr, xi, L, direct_below=0)
        br, bi = R.dft_direct(xr, xi, L)
        err = float(np.max(np.hypot(ar - br, ai - bi)))
        scale = float(np.max(np.hypot(br, bi)))
        tol = 8 * EPS_LD * (np.log2(L) + 1) * max(scale, 1e-300)       # a few long-double ulps * log L of the largest bin
        assert err <= tol, (L, err, tol)
        worst = max(worst, err / tol)
    print(f"recursion vs direct sum: worst error / tolerance {worst:.3f}")


def test_large_prime_leaf_equals_the_direct_sum():
    """dft_chirp (prime leaves above PRIME_DIRECT_MAX) against the direct sum at primes both can do."""
    rng = np.random.default_rng(4)
    for L in (97, 1031, 2053):
        xr, xi = rng.standard_normal((2, L)).astype(LD), rng.standard_normal((2, L)).astype(LD)
        ar, ai = R.dft_chirp(xr, xi, L)
        br, bi = R.dft_direct(xr, xi, L)
        err = float(np.max(np.hypot(ar - br, ai - bi))) / float(np.max(np.hypot(br, bi)))
        assert err <= 64 * EPS_LD * np.log2(4 * L), (L, err)


def test_impulses_are_exactly_formed():
    """rfft_ref of a unit impulse at j is unit_root(j k, L) itself (closed form) and the recursion gives the same to long-
    double rounding; the symmetric points are exact: 1 at k j = 0, -1 at half a turn, 0 real part at quarter turns."""
    for L in (8, 12, 60, 64, 97, 360):
        for j in R.impulse_positions(L, n2=4, run=7):
            x = np.zeros(L, np.float32); x[j] = 1.0
            re, im = R.rfft_ref(x, L)
            k = np.arange(L // 2 + 1)
            c, s = R.unit_root(j * k, L)
            s = s.copy(); s[0] = 0
            if L % 2 == 0:
                s[-1] = 0
            assert np.array_equal(re, c) and np.array_equal(im, s), (L, j)
            fr, fi = R.rfft_ref(x, L, closed_form=False, direct_below=0)
            assert float(np.max(np.hypot(fr - re, fi - im))) <= 8 * EPS_LD * (np.log2(L) + 1), (L, j)
            turn = (j * k) % L
            assert np.all(re[turn == 0] == 1) and np.all(im[turn == 0] == 0)
            assert np.all(re[2 * turn == L] == -1) and np.all(im[2 * turn == L] == 0)
            assert np.all(re[(4 * turn) % (2 * L) == L] == 0)
    assert R.hann_ld(np.arange(1), 1)[0] == 1 and np.all(R.hann_ld(np.arange(2), 2) == 0)
    assert np.array_equal(R.hann_ld(np.arange(3), 3), np.array([0, 1, 0], dtype=LD))


@pytest.mark.parametrize("n", [1, 2, 9, 10, 64, 97, 194, 360])
def test_round_trip(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    re, im = R.rfft_ref(x, n)
    y = R.irfft_masked_ref(_c(re, im), np.ones(n // 2 + 1, np.float32), n)
    # (the spectrum passes through float64 on its way, as the device's does)
    assert float(np.max(np.abs(y - x.astype(LD)))) <= 4 * R.U * np.sqrt(n) * float(np.max(np.abs(x)))
    X = _c(re, im) + 0j
    X[0] += 0.5j
    if n % 2 == 0:
        X[-1] -= 0.25j
    y2 = R.irfft_masked_ref(X, np.ones(n // 2 + 1, np.float32), n)
    assert np.array_equal(y2, y)                                   # imaginary parts of bin 0 / Nyquist are ignored


WORST = {}                       # (label, path, family) -> [probabilistic, rigorous, per-bin, where]: printed per test


def _record(label, path, name, e2, emax, prob, rig, where):
    if prob == 0.0:
        assert e2 == 0.0, (label, name, where)
        return
    assert e2 <= prob and e2 <= rig and emax <= rig, (label, path, name, where, e2 / prob, e2 / rig, emax / rig)
    w = WORST.setdefault((label, f"{path[0]} {path[1]}", name.split()[0]), [0.0, 0.0, 0.0, ""])
    if e2 / prob > w[0]:
        w[3] = where
    w[0], w[1], w[2] = max(w[0], e2 / prob), max(w[1], e2 / rig), max(w[2], emax / rig)


def _print_worst(label):
    for (lab, path, fam), (p, r, b, where) in sorted(WORST.items()):
        if lab == label:
            print(f"POCKETFFT-RATIO {lab + ' ' + path:28s} {fam:12s} worst error/bound: probabilistic {p:.4f} rigorous {r:.5f} "
                  f"per-bin {b:.5f}  ({where})")


def _numpy_rfft(x, L, d, w, hann):
    """numpy.fft.rfft(x[:d] * numpy.hanning(w)[:d], n=L) in float64, rows of x; None where numpy does not define it."""
    seg = x[:, : max(d, 0)].astype(np.float64)
    if hann and w != 1:
        if w < d:
            return None
        seg = seg * np.hanning(w)[:d]
    return np.fft.rfft(seg, n=L, axis=1)


def _pocketfft_forward(label, L, names, x, hann, variants, d=None, w=None, padded=False, pair_norm_rows=None):
    """numpy's transform of every row against the reference, held to the bound of every switch variant in `variants`."""
    d = L if d is None else d
    w = L if w is None else w
    got = _numpy_rfft(x, L, d, w, hann)
    if got is None:
        return
    re, im = R.rfft_ref(x, L, data_len=d, win_len=w, hann=hann)
    v, xs = R.windowed_input(x, L, d, w, hann)
    vn, xn = [_norm(r) for r in v], [_norm(r) for r in xs]
    for sw in variants:
        for i, name in enumerate(names):
            paired = pair_norm_rows is not None and i in pair_norm_rows
            path = R.predict_path(L, padded=padded, paired=paired, **sw)
            a, b = vn[i], xn[i]
            if paired and path[1] == "pair":
                j = pair_norm_rows[i]
                a, b = float(np.hypot(vn[i], vn[j])), float(np.hypot(xn[i], xn[j]))
            if path[0] == "smooth":
                prob, rig = R.direct_bound(L, path[1], a, b, hann, d, w)
            else:
                prob, rig = R.bluestein_bound(L, path[1], path[2], a, b, hann, d, w)
            err = np.abs(got[i] - _c(re[i], im[i]))
            _record(label, path, name, float(np.sqrt(np.sum(err ** 2))), float(err.max()), prob, rig,
                    f"L={L} hann={hann}" + (f" d={d} w={w}" if padded else ""))


def _direct_inputs(L, **kw):
    n2 = R.smooth_split_py(L)[1]
    half = R.predict_path(L)[1] != "full"
    return R.make_inputs(L, n2=n2, run=2 * R.smooth_split_py(L // 2)[1] if half else None, **kw)


def _thread_run(L):
    path = R.predict_path(L)
    if path[0] != "bluestein":
        return None
    _, n1, n2, C = R.bluestein_geometry(path[2])
    run = (256 // C) * n2
    return run if run < L else None


DIRECT_VARIANTS = [dict(), dict(fuse_half_split=False), dict(half_real_ffts=False)]
THREE_VARIANTS = [dict(three_pow2_sizes=True), dict(three_pow2_sizes=False)]


@pytest.mark.parametrize("hann", [False, True])
def test_numpy_float64_transform_satisfies_the_direct_bounds(hann):
    """Every direct length 64..8192, every family, the bound of every switch variant the GPU test runs (default,
    fuse_half_split = False, half_real_ffts = False: half fused, half split and full at the same even length)."""
    for L in R.direct_lengths():
        names, x = _direct_inputs(L)
        _pocketfft_forward("direct", L, names, x, hann, DIRECT_VARIANTS if L % 2 == 0 else DIRECT_VARIANTS[:1])
    _print_worst("direct")


@pytest.mark.parametrize("L", R.PLAN_EXTREMES)
def test_numpy_float64_transform_satisfies_the_plan_extreme_bounds(L):
    names, x = _direct_inputs(L, families=("impulse", "noise"))
    for hann in (False, True):
        _pocketfft_forward("extreme", L, names, x, hann, [dict()])
    _print_worst("extreme")


@pytest.mark.parametrize("hann", [False, True])
def test_numpy_float64_transform_satisfies_the_bluestein_bounds(hann):
    """Every Bluestein length the GPU tests list -- all of 1..320 with every family, all size-boundary lengths with impulses
    and noise -- under the bounds of three_pow2_sizes on and off; the offset and packed tests' lengths as well."""
    blue = R.bluestein_lengths()
    for L in blue:
        small = L <= 320
        names, x = R.make_inputs(L, run=_thread_run(L), families=R.FAMILY_NAMES if small else ("impulse", "noise"))
        _pocketfft_forward("small" if small else "boundary", L, names, x, hann, THREE_VARIANTS)
    for L in (360, 450, 225, 194, 97, 4099, 4800):
        names, x = R.make_inputs(L, families=("noise",))
        _pocketfft_forward("offsets", L, names, x, hann, [dict()])
    if hann:
        for L in (14, 194, 254, 2 * 683, 97):
            names, x = R.make_inputs(L, families=("noise",))
            _pocketfft_forward("packed", L, names, x, hann, [dict()])
    for label in ("small", "boundary", "offsets", "packed"):
        _print_worst(label)


@pytest.mark.parametrize("hann", [False, True])
def test_numpy_float64_transform_satisfies_the_padded_bounds(hann):
    """The padding / window combinations of the GPU test wherever numpy defines x[:d] * hanning(w)[:d] (w >= d, or w = 1)."""
    for L in (360, 450, 225, 194, 97):
        names, x = R.make_inputs(2 * L, families=("noise", "constant"))
        for d in (0, 1, 2, L - 1, L, L + 1, 2 * L):
            for w in sorted({1, 2, 3, d - 1, d, d + 1, 2 * d}):
                if w >= 1 and (hann or w == max(d, 1)):
                    _pocketfft_forward("padded", L, names, x, hann, [dict()], d=d, w=w, padded=True)
    _print_worst("padded")


@pytest.mark.parametrize("hann", [False, True])
def test_numpy_float64_transform_satisfies_the_pair_bound(hann):
    for L in (7, 97, 194, 683, 2 * 683 + 1):
        for count in (2, 3):
            names, x = R.make_inputs(L, families=("noise", "alternating", "constant"))
            x = x[:count] * np.array([1.0, 1e-3, 0.3], np.float32)[:count, None]
            _pocketfft_forward("pairs", L, names[:count], x, hann, [dict(pair_across_channels=True)],
                               pair_norm_rows={0: 1, 1: 0})
    _print_worst("pairs")


@pytest.mark.parametrize("n", [64, 128, 130, 4800, 28800, 97, 194, 23257])
def test_numpy_float64_inverse_satisfies_the_band_bound(n):
    """numpy.fft.irfft rounded to float32 against the band bound of every inverse path of every length the GPU test runs:
    alone (half-length where the length allows) and as one of a pair (the partner's masked spectrum in the float64 term)."""
    rng = np.random.default_rng(5 + n)
    x = rng.standard_normal(n).astype(np.float32)
    X = np.fft.rfft(x.astype(np.float64))
    masks = [np.clip(rng.random(n // 2 + 1) * 1.5 - 0.25, 0, 1).astype(np.float32) for _ in range(2)]
    for paired in (False, True):
        y = R.irfft_masked_ref(X, masks[0], n)
        got = np.fft.irfft(X * masks[0].astype(np.float64), n).astype(np.float32)
        fam, kind, size = R.predict_inverse_path(n, paired=paired)
        xm = _norm(np.abs(X) * masks[0])
        if paired:
            xm = float(np.hypot(xm, _norm(np.abs(X) * masks[1])))
        bound, t = R.band_bound(y, xm, n, fam, kind, size)
        ratio = float(np.max(np.abs(got.astype(LD) - y).astype(np.float64) / bound))
        print(f"POCKETFFT-RATIO inverse {fam} {kind} n={n}: worst error / band bound {ratio:.4f} "
              f"(float64 term / half a float32 ulp of the peak: {t / (0.5 * np.spacing(np.float32(np.max(np.abs(got))))):.2e})")
        assert ratio <= 1.0, (n, paired, ratio)


# where every planted error is caught: (kind, length, hann, family); the smallest length at which the error applies
PLANTED_CASES = [
    ("twiddle", 64, False, "impulse j=9"),          # x[a n2 + b], a = b = 1, n2 = 8: the one column whose twiddle is wrong
    ("periodic_hann", 64, True, "constant"),
    ("window_shift", 64, True, "constant"),
    ("last_sample", 64, False, "constant"),
    ("bin_swap", 64, False, "impulse j=1"),
    ("chirp_wrap", 65537, False, "impulse j=65536"),   # n * n first wraps at n = 65536: needs a sample there
    ("mirror_tile", 128, False, "noise"),           # the first length with a half-length fused job
]


@pytest.mark.parametrize("kind,L,hann,family", PLANTED_CASES)
def test_every_planted_error_breaks_the_bound(kind, L, hann, family):
    n2 = (R.smooth_split_py(L) or (None, None))[1]
    if family.startswith("impulse"):
        x = np.zeros((1, L), np.float32); x[0, int(family.split("=")[1])] = 1.0
        names = [family]
    else:
        names, x = R.make_inputs(L, n2=n2, families=(family,))
    re, im = R.rfft_ref(x, L, hann=hann)
    v, xs = R.windowed_input(x, L, hann=hann)
    prob, rig, path = R.forward_bound(L, _norm(v[0]), _norm(xs[0]), hann)
    good = R.planted_spectrum(x[0], L, "none", hann)
    bad = R.planted_spectrum(x[0], L, kind, hann)
    e_good = float(np.sqrt(np.sum(np.abs(good - _c(re[0], im[0])) ** 2)))
    e_bad = float(np.sqrt(np.sum(np.abs(bad - _c(re[0], im[0])) ** 2)))
    print(f"planted {kind:14s} L={L} hann={hann} family '{names[0]}' path {path}: error / bound {e_bad / prob:.3g} "
          f"(the same restatement without the error: {e_good / prob:.3g})")
    assert e_good <= prob, (kind, e_good, prob)                    # the restatement itself is inside the bound
    assert e_bad > prob, (kind, e_bad, prob)                       # ... and the planted error is not


def test_planted_nyquist_imaginary_part_breaks_the_band_bound():
    """The half-size inverse that leaves the Nyquist bin's imaginary part in, on a hand-made spectrum that has one, at 128
    (the smallest length with a half-length inverse)."""
    n = 128
    X = np.zeros(n // 2 + 1, np.complex128)
    X[3], X[-1] = 2.0 - 1.0j, 1.0 + 0.75j
    mask = np.ones(n // 2 + 1, np.float32)
    y = R.irfft_masked_ref(X, mask, n)
    fam, kind, size = R.predict_inverse_path(n, paired=False)
    assert (fam, kind, size) == ("smooth", "half", 64)
    bound, _ = R.band_bound(y, _norm(np.abs(X)), n, fam, kind, size)
    bad = R.planted_band_signal(X, mask, n).astype(np.float32)
    Xc = X.copy(); Xc[-1] = Xc[-1].real
    good = R.planted_band_signal(Xc, mask, n).astype(np.float32)
    r_bad = float(np.max(np.abs(bad.astype(LD) - y).astype(np.float64) / bound))
    r_good = float(np.max(np.abs(good.astype(LD) - y).astype(np.float64) / bound))
    print(f"planted nyquist_imag n={n} hand-made spectrum: error / bound {r_bad:.3g} (without the error: {r_good:.3g})")
    assert r_good <= 1.0 < r_bad


def _switches(**kw):
    base = dict(pair_real_ffts=True, pair_across_channels=False, half_real_ffts=True, fuse_half_split=True,
                sparse_bands=True, three_pow2_sizes=True, workspace_budget_bytes=1 << 30)
    base.update(kw)
    return Switches(**base)


@pytest.mark.parametrize("kw", [dict(), dict(fuse_half_split=False), dict(half_real_ffts=False),
                                dict(three_pow2_sizes=False), dict(pair_across_channels=True)])
def test_path_predictions_agree_with_the_planner(kw):
    """predict_path against engine_plan.plan_rfft (launch family, half or full, transform / convolution size) for every
    length the GPU tests list, with smooth_split restated in Python (compared with the library's in the GPU file)."""
    lengths = np.array(R.direct_lengths() + list(R.PLAN_EXTREMES) + R.bluestein_lengths(), dtype=np.int32)
    sw = _switches(**kw)
    pairing = bool(kw.get("pair_across_channels"))
    reps = 2 if pairing else 1
    lens = np.repeat(lengths, reps)
    xoff = np.arange(lens.size, dtype=np.int64) * 0
    _, launches, _ = plan_rfft(xoff, lens, None, None, False, sw, R.smooth_split_py)
    seen = {}
    for ln in launches:
        for j, e in enumerate(ln.jobs):
            L = int(lens[e])
            if ln.family == SMOOTH:
                fused = ln.half and ln.tables["x2"] is None
                kind = ("half_fused" if fused else "half_split") if ln.half else "full"
            else:
                il = ln.tables["il"]
                kind = "half" if (il is not None and il[j]) else ("pair" if ln.partner[j] >= 0 else "single")
            seen[L] = (ln.family, kind, ln.size)
    for L in lengths.tolist():
        flags = {k: v for k, v in kw.items()}
        want = R.predict_path(L, paired=pairing, **flags)
        assert seen[L] == want, (L, kw, seen[L], want)
    kinds = {v[1] for v in seen.values()}
    if not kw:
        assert {"half_fused", "half_split", "full", "half", "single"} <= kinds, kinds


def test_smooth_split_restatement_basics():
    assert R.smooth_split_py(480000) == (640, 750) and R.smooth_split_py(64) == (8, 8)
    assert R.smooth_split_py(63) is None and R.smooth_split_py(2 * 3 * 5 * 7 * 64) is None
    assert R.smooth_split_py(1 << 20) == (1024, 1024) and R.smooth_split_py((1 << 20) + 1024) is None
    assert R.factor_radices_py(640) == [8, 8, 10] and R.factor_radices_py(750) == [10, 5, 5, 3]
    assert R.conv_size_py(97 + 48) == 192 and R.conv_size_py(20) == 32 and R.conv_size_py(65537 + 65537 // 2) == 1 << 17
