"""poly_roots_kernel (Aberth-Ehrlich) and fir_numerator_kernel of ira_roots.hip, through Engine.poly_roots and
Engine.fir_numerator, against the yardsticks of tests/roots_ref.py: the backward error of every returned root in long double
(bound 4 n u, derived there), a Vieta completeness check (a duplicated root passes the backward error), and for the numerator
a long-double convolution with the bound (p + 3) u sum_k |a_k h_(n-k)|.  numpy.roots is NOT the reference above degree 129:
its own backward error is 1e3 .. 1e13 u there where the kernel's stays under one n u.

Degrees on both sides of every launch boundary (four lanes per root up to 256 in 256-, 512- and 1024-thread workgroups, one
lane per root in 512- and 1024-thread workgroups above), roots outside the unit circle, multiple roots, z^n - 1, roots of
modulus 1e-3, every trimming rule in one 37-row launch with bit-identity against single-row launches, and the product path
at zero order 512 and AR order 1024.  test_zz_report prints the worst figure of every group.

Outside the unit circle plain Horner overflows (|z|^n), and one NaN iterate reaches every other root's pair sum on the next
sweep: the outside cases, the degree-1024 ring (an early sweep overshoots) and the product case at zero order 512 are the
ones that come back all NaN from a kernel that evaluates p that way.  At the triple root the sweeps are driven by rounding
noise: without the kernel's "p is zero to within roundoff" test the last of 200 random jumps is what comes back.

Multiple roots: the forward distance to the m-fold root is at most 10 x numpy.roots' on the same coefficients.  Where
numpy.roots returns the m-fold root EXACTLY (z^2 - 2 z + 1: distance 0) that cannot be met; there, and only there, the
allowance is the distance a root finder with the backward error 4 n u may leave at an m-fold root r,
(4 n u sum_k |c_k| |r|^(n-k) / |p^(m)(r) / m!|)^(1/m), near u^(1/m).
"""
import math

import numpy as np
import pytest

import roots_ref as R
from oracle import ira_oracle as O

pytestmark = pytest.mark.gpu
SR = 48000
STATS = {}                                    # group -> {figure: worst}, printed by test_zz_report


@pytest.fixture(scope="module")
def eng():
    R.need_longdouble()
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def _note(group, **kv):
    st = STATS.setdefault(group, {})
    for k, v in kv.items():
        st[k] = max(st.get(k, v), v)


def _launch(eng, rows, trail_eps=R.TRAIL_EPS):
    """(raw roots (npoly, ncoef - 1, 2), counts) of the rows (npoly, ncoef) in ONE launch."""
    rows = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.float64)
    roots, cnt = eng.poly_roots(eng.to_dev(rows), rows.shape[0], rows.shape[1], trail_eps)
    return roots.cpu().numpy().copy(), cnt.cpu().numpy().copy()


def _solve(eng, c):
    """Roots of ONE polynomial, nothing trimmed (trail_eps = 0): the trailing coefficients of the high-degree rings and of the
    small-modulus case lie below the product's 1e-14 and would be dropped with it; trimming has its own tests below."""
    raw, cnt = _launch(eng, c, trail_eps=0.0)
    assert int(cnt[0]) == raw.shape[1] == c.size - 1, (int(cnt[0]), c.size - 1)
    return raw[0, :, 0] + 1j * raw[0, :, 1]


def _check_backward(group, name, c, z):
    """Finite, and every root within the backward bound of the trimmed polynomial c (degree n = c.size - 1)."""
    n = c.size - 1
    assert z.size == n, (name, z.size, n)
    finite = int(np.sum(np.isfinite(z.real) & np.isfinite(z.imag)))
    be = R.backward_error(c, z)
    worst = float(np.max(be)) if finite == n else float("nan")
    print(f"{group}/{name}: n {n}, finite {finite}, backward error {worst / (n * R.U):.3g} n u (bound 4)")
    assert finite == n, (name, f"{n - finite} of {n} roots are not finite")
    _note(group, backward_error_over_nu=worst / (n * R.U))
    assert worst <= R.bound(n), (name, worst / (n * R.U))


def _check_complete(group, name, c, z):
    tol = R.completeness_tolerance(c)
    got = R.completeness(c, z)
    print(f"{group}/{name}: completeness {got:.3g}, tolerance {tol:.3g}")
    _note(group, completeness_over_tolerance=got / tol)
    assert got <= tol, (name, got, tol)


# ------------------------------------------------------------------------------------------------ single polynomials
@pytest.mark.parametrize("n", R.DEGREES)
def test_ring_degrees_across_the_launch_boundaries(eng, n):
    c, known = R.degree_case(n)
    z = _solve(eng, c)
    _check_backward("ring", f"ring{n}", c, z)
    _check_complete("ring", f"ring{n}", c, z)
    if n == 1:
        ref = -c[1] / c[0]
        assert abs(z[0] - ref) <= np.spacing(abs(ref)), (z[0], ref)
    if n <= R.MATCH_MAX_DEGREE:
        tol = max(10.0 * R.match(np.roots(c), known), 1e-13)
        got = R.match(z, known)
        print(f"ring/ring{n}: matching distance {got:.3g}, allowance {tol:.3g}")
        _note("ring", matching_over_allowance=got / tol)
        assert got <= tol, (n, got, tol)


@pytest.mark.parametrize("n,extra", R.OUTSIDE, ids=[f"{n}" for n, _ in R.OUTSIDE])
def test_roots_outside_the_unit_circle(eng, n, extra):
    c, _ = R.outside_case(n, extra)
    z = _solve(eng, c)
    _check_backward("outside", f"outside{n}", c, z)
    _check_complete("outside", f"outside{n}", c, z)
    # the roots given outside are found outside; that no OTHER root is outside holds only while the ring roots of the
    # float64-rounded polynomial stay where they were generated: at degree 1024 they move by 4e-2, 38 of them across the circle
    outside = int(np.sum(np.abs(z) > 1.0))
    assert outside >= len(extra) and (n > R.MATCH_MAX_DEGREE or outside == len(extra)), (n, outside)


def test_badly_scaled_ring_1024_meets_the_backward_bound(eng):
    """max |c| around 1e14: the kernel converges on wide-range coefficients too.  The backward bound only (see
    roots_ref.badly_scaled_case)."""
    c = R.badly_scaled_case()
    _check_backward("badly_scaled", "ring1024", c, _solve(eng, c))


@pytest.mark.parametrize("case", R.multiple_cases(), ids=lambda t: t[0])
def test_multiple_roots(eng, case):
    name, c, root, m = case
    n = c.size - 1
    z = _solve(eng, c)
    _check_backward("multiple", name, c, z)
    cl = c.astype(R.LD)
    s = np.polyval(np.abs(cl), R.LD(abs(root)))
    am = abs(np.polyval(np.polyder(cl, m), R.LD(root))) / math.factorial(m)
    ref = R.multiple_root_distance(np.roots(c), root, m)
    tol = 10.0 * ref if ref > 0.0 else float((R.bound(n) * s / am) ** (R.LD(1) / m))
    got = R.multiple_root_distance(z, root, m)
    print(f"multiple/{name}: distance to the {m}-fold root {got:.3g}, allowance {tol:.3g}")
    _note("multiple", distance_over_allowance=got / tol)
    assert got <= tol, (name, got, tol)


@pytest.mark.parametrize("case", R.special_cases(), ids=lambda t: t[0])
def test_special_shapes(eng, case):
    name, c = case
    z = _solve(eng, c)
    _check_backward("special", name, c, z)
    _check_complete("special", name, c, z)


# ------------------------------------------------------------------------------------------- trimming and layout
NCOEF, NPOLY, KINDS = R.NCOEF, R.NPOLY, R.KINDS


def _check_row(group, name, row, raw, count, trail_eps):
    core, tz = R.trim(row, trail_eps)
    if core is None:
        assert count == 0, (name, count)
        return
    n = core.size - 1
    assert count == n + tz, (name, count, n, tz)
    z = raw[:count, 0] + 1j * raw[:count, 1]
    assert np.all(z[n:] == 0.0), name                       # the roots at the origin come after the others
    if n:
        _check_backward(group, name, core, z[:n])
        _check_complete(group, name, core, z[:n])


def test_trimming_and_layout_in_one_launch(eng):
    from audio_analysis_amd.analyse.zplane import _to_complex
    rows = R.trim_rows()
    roots_dev, cnt_dev = eng.poly_roots(eng.to_dev(rows), NPOLY, NCOEF, R.TRAIL_EPS)
    raw, cnt = roots_dev.cpu().numpy().copy(), cnt_dev.cpu().numpy().copy()
    host = _to_complex(roots_dev, cnt_dev)
    want = R.KIND_COUNTS
    for i in range(NPOLY):
        kind = KINDS[i % len(KINDS)]
        assert int(cnt[i]) == want[kind] == O.poly_roots(rows[i]).size, (i, kind, int(cnt[i]))
        assert host[i].size == int(cnt[i])                   # entries beyond the count never reach the caller
        assert np.array_equal(host[i], raw[i, : cnt[i], 0] + 1j * raw[i, : cnt[i], 1])
        _check_row("trimming", f"row{i}_{kind}", rows[i], raw[i], int(cnt[i]), R.TRAIL_EPS)
    # one workgroup per polynomial and Jacobi sweeps: a row's roots do not depend on its neighbours or its place
    back, cnt_back = _launch(eng, rows[::-1])
    assert np.array_equal(cnt_back[::-1], cnt)
    for i in range(NPOLY):
        k = int(cnt[i])
        assert np.array_equal(back[NPOLY - 1 - i, :k], raw[i, :k]), i
        alone, cnt_alone = _launch(eng, rows[i])
        assert int(cnt_alone[0]) == k and np.array_equal(alone[0, :k], raw[i, :k]), i


def test_exact_trailing_zeros_become_roots_at_the_origin(eng):
    """With trail_eps = 0 nothing is dropped for being small: exact trailing zeros are roots at 0, reported after the others
    (numpy.roots' rule).  With the product's 1e-14 the same zeros are dropped with the small coefficients (test above)."""
    rows = R.trim_rows()
    pick = [i for i in range(NPOLY) if KINDS[i % len(KINDS)] in ("trailing_zeros", "all_zero", "leading_zeros", "full65")]
    rows = rows[pick]
    rows[-1] = 0.0
    rows[-1, 2] = 5.0                                        # 5 z^63: a constant times z^63, 63 roots at the origin
    raw, cnt = _launch(eng, rows, trail_eps=0.0)
    for j, i in enumerate(pick):
        assert int(cnt[j]) == np.roots(rows[j]).size, (i, int(cnt[j]))
        _check_row("trimming", f"eps0_row{i}", rows[j], raw[j], int(cnt[j]), 0.0)
    assert int(cnt[-1]) == 63 and np.all(raw[-1, :63] == 0.0)
    assert sorted(set(int(c) for c in cnt)) == [0, 63, 65]


# --------------------------------------------------------------------------------------------------- FIR numerator
FIR_ORDERS = ((1, 0), (8, 200), (64, 64), (64, 127), (64, 128), (256, 64), (300, 513))
FIR_ROWS = 4


@pytest.mark.parametrize("p,q", FIR_ORDERS)
def test_fir_numerator_against_long_double_convolution(eng, p, q):
    rng = np.random.default_rng(1000 * p + q)
    x = rng.standard_normal(4 * 5000 + 64).astype(np.float32)
    x_dev = eng.to_dev(x)
    xoff = np.array([3, 5017, 10040, 15061], dtype=np.int64)
    a = np.stack([R.ring(p, 700 + p + r)[0] for r in range(FIR_ROWS)])
    a[1] *= -2.5                                              # the kernel does not assume a[0] = 1
    a_dev = eng.to_dev(a)
    for n_len in sorted({max(1, q), q + 1, q + 2, 1, 5000}):
        lens = np.full(FIR_ROWS, n_len, dtype=np.int32)
        for div in (None, np.array([1.0, 0.37, 3.0, 1e-3])):
            b = eng.fir_numerator(a_dev, p, x_dev, xoff, lens, div, q).cpu().numpy().copy()
            assert b.shape == (FIR_ROWS, q + 1)
            for r in range(FIR_ROWS):
                ref, s = R.fir_numerator(a[r], x[xoff[r]:], n_len, 1.0 if div is None else div[r], q)
                err = np.abs(b[r].astype(R.LD) - ref)
                allow = (p + 3) * R.U * s
                with np.errstate(all="ignore"):
                    share = float(np.max(np.where(err == 0, R.LD(0), err / allow)))
                _note("fir_numerator", error_over_allowance=share)
                assert np.all(err <= allow), (p, q, n_len, div is not None, r, share)
                one = eng.fir_numerator(eng.to_dev(a[r]), p, x_dev, xoff[r : r + 1], lens[r : r + 1],
                                        None if div is None else div[r : r + 1], q).cpu().numpy()
                assert np.array_equal(one[0], b[r]), (p, q, n_len, r)
    print(f"fir_numerator/p{p}_q{q}: worst error {STATS['fir_numerator']['error_over_allowance']:.3g} of the allowance so far")


# ------------------------------------------------------------------------------------------------------ end to end
def _device_polynomials(eng, chans, order, zero_order=None):
    """The AR coefficients (and the numerator) zplane_device computes for trim_to_peak=False, normalise_segment=True: the same
    launches on the same data, so the same bits."""
    batch = eng.upload(chans)
    lens = batch.length.astype(np.int32)
    div = eng.segment_peaks(batch.x, batch.off, batch.length)
    div = np.where(div > 0.0, div, 1.0)
    co, _ = eng.ar_fit(batch.x, batch.off, lens, div, order, 0.0)
    b = None
    if zero_order is not None:
        b = eng.fir_numerator(co, order, batch.x, batch.off, lens, div, zero_order).cpu().numpy().copy()
    return co.cpu().numpy().copy(), b, div


def test_end_to_end_zero_order_512_with_pre_onset_noise(eng):
    """derive_zeros at zero order 512 on a segment that starts 8 samples of 1e-6-level noise before the peak
    (trim_to_peak=False): the numerator's leading coefficients are tiny, its largest zeros lie far outside the unit circle."""
    from audio_analysis_amd.analyse import zplane as zp
    from audio_analysis_amd.synth import synth_ir
    quiet = synth_ir(3, 0, 12000, rt60_seconds=0.3, pre_delay=8)
    quiet[:8] = (1e-6 * np.random.default_rng(8).standard_normal(8)).astype(np.float32)
    chans = [quiet, synth_ir(4, 0, 12000, rt60_seconds=0.25, pre_delay=0)]
    s = zp.ZPlaneAnalysisSettings(derive_zeros=True, zero_order=512, ar_order=64, trim_to_peak=False)
    res = zp.analyse_zplane_batch(chans, SR, ["quiet", "normal"], s)
    co, b, div = _device_polynomials(eng, chans, 64, 512)
    for i, (x, r) in enumerate(zip(chans, res)):
        name = r.channel_name
        ref, sabs = R.fir_numerator(co[i], x, x.size, div[i], 512)
        err = np.abs(b[i].astype(R.LD) - ref)
        assert np.all(err <= (64 + 3) * R.U * sabs), name
        core, tz = R.trim(b[i])
        assert tz == 0 and core.size == 513, (name, tz, core.size)
        assert r.zeros.size == 512
        _check_backward("end_to_end", f"{name}_zeros", core, r.zeros)
        _note("end_to_end", largest_zero_modulus=float(np.max(np.abs(r.zeros))))
        poles_core, poles_tz = R.trim(co[i])
        assert poles_tz == 0 and poles_core.size == 65, name
        _check_backward("end_to_end", f"{name}_poles", poles_core, r.poles)
        o = O.analyse_zplane(x, SR, ar_order=64, derive_zeros=True, zero_order=512, trim_to_peak=False)
        assert r.poles.size == o["poles"].size == 64 and r.zeros.size == o["zeros"].size
        assert int(np.sum(np.abs(r.poles) >= 1.0)) == o["unstable"]      # order 64: numpy.roots is trustworthy


def test_end_to_end_ar_order_1024(eng):
    """1024 finite poles within the backward bound of the device's own coefficients; the number of poles and of unstable poles
    are the oracle's.  Radii are not compared: numpy.roots carries a backward error of thousands of u at this degree.  The
    unstable count can be: the oracle's largest radius on this response is 0.9995, 5e-4 inside the unit circle, and
    numpy.roots and the restated iteration agree on the oracle's largest radii to eight digits."""
    from audio_analysis_amd.analyse import zplane as zp
    from audio_analysis_amd.synth import synth_ir
    chans = [synth_ir(5, 0, 12000, rt60_seconds=0.3)]
    s = zp.ZPlaneAnalysisSettings(ar_order=1024, trim_to_peak=False)
    r = zp.analyse_zplane_batch(chans, SR, ["m"], s)[0]
    co, _, _ = _device_polynomials(eng, chans, 1024)
    core, tz = R.trim(co[0])
    assert tz == 0 and core.size == 1025 and r.poles.size == 1024
    _check_backward("end_to_end", "order1024_poles", core, r.poles)
    o = O.analyse_zplane(chans[0], SR, ar_order=1024, trim_to_peak=False)
    unstable = int(np.sum(np.abs(r.poles) >= 1.0))
    print(f"end_to_end/order1024: unstable {unstable} (oracle {o['unstable']}), largest radius {np.max(np.abs(r.poles)):.9f} "
          f"(oracle {o['max_radius']:.9f})")
    assert r.poles.size == o["poles"].size
    assert unstable == o["unstable"]


def test_zz_report(capsys):
    """Prints the worst figure of every group: backward error in units of n u (bound 4), completeness, matching and multiple-root
    distances and the numerator's error as shares of their allowances.  Asserts nothing."""
    with capsys.disabled():
        for group in sorted(STATS):
            print(f"\n{group}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(STATS[group].items())), end="")
        print()
