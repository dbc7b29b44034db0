"""
Holds the spectrum restatement (tests/spectrum_ref.py) to NumPy's own functions, and shows that the inputs the GPU tests
share with it test what they claim (ties tie, branches are taken, margins hold) -- on a machine without a GPU.
"""
import numpy as np
import pytest

import spectrum_ref as R

LD, F32 = R.LD, R.F32


# ------------------------------------------------------------------------------------------------------------ unwrap
@pytest.mark.parametrize("name", R.UNWRAP_NAMES)
def test_unwrap_is_numpys_bit_for_bit(name):
    p = dict(R.unwrap_cases())[name]
    got, want = R.unwrap(p), np.unwrap(p)
    assert got.tobytes() == want.tobytes(), name
    # the kernel's order of the same additions stays within the derived bound of the long-double scan, and so does NumPy's
    ref, mx = R.unwrap_ld(p)
    bar = R.unwrap_bound(ref, mx, p.size)
    tree = R.unwrap_tree(p)
    assert np.all(np.abs(tree.astype(LD) - ref) <= bar), name
    seq_err = float(np.max(np.abs(got.astype(LD) - ref)))
    print(f"SPEC-REF unwrap {name}: numpy's own sequential sum is {seq_err:.3e} off the long-double scan (max prefix {mx:.1f})")
    if mx == 0.0:
        assert tree.tobytes() == p.tobytes()


def test_unwrap_cases_plant_what_they_claim():
    UNWRAP = R.unwrap_cases()
    assert [n for n, _ in UNWRAP] == R.UNWRAP_NAMES
    seen = {"pi_up": 0, "pi_down": 0, "inside": 0, "two_pi": 0, "fmod": 0}
    for name, p in UNWRAP:
        dd = np.diff(p)
        if name.startswith(("steps", "mixed", "winding")):
            assert np.all(np.abs(p) <= 2 * R.KPI), name
            assert np.all(np.abs(dd + R.KPI) < 4 * R.KPI)
        if name.startswith("steps"):
            seen["pi_up"] += int(np.sum(dd == R.KPI))
            seen["pi_down"] += int(np.sum(dd == -R.KPI))
            seen["inside"] += int(np.sum(np.abs(dd) == np.nextafter(R.KPI, 0.0)))
            seen["two_pi"] += int(np.sum(np.abs(dd) == 2 * R.KPI))
        if name.startswith("caller"):
            a = dd + R.KPI
            seen["fmod"] += int(np.sum((a >= 4 * R.KPI) | (a <= -2 * R.KPI)))
            assert p.size < 100 or np.max(np.abs(dd)) > 40.0
        if name.startswith("winding") and p.size >= 12289:
            assert R.unwrap_ld(p)[1] > 3000.0                                   # the carry across three tiles
    assert all(v > 0 for v in seen.values()), seen
    # a step sits on both sides of each structural position of a three-tile spectrum
    p = dict(UNWRAP)["steps n=12289"]
    at = set(np.flatnonzero(np.diff(p) != 0.0) + 1)
    assert {1, 3, 4, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 12288} <= at


# -------------------------------------------------------------------------------------------------------- group delay
GD = R.gd_cases()
# which formula numpy.gradient takes, per (n_fft, step) in the order of gd_cases(): only the two- and three-bin axes are
# uniform to the bit (w[2] = 2 w[1] exactly); from four bins on some neighbouring differences differ in their last bit
# (the nine-bin axes of GD_UNIFORM_LONG with power-of-two quotients are the longest uniform ones: k * (2 pi) is exact to k = 8)
GD_UNIFORM = [True, True, True, True] + [False] * 10 + [True, True, False]


@pytest.mark.parametrize("n_fft,val", GD)
def test_gradient_is_numpys_bit_for_bit(n_fft, val):
    nb = n_fft // 2 + 1
    f = R.gd_phase(nb, n_fft)
    w = (2.0 * np.pi) * ((np.arange(nb) * val) / R.GD_SR)
    want = -np.gradient(f, w)
    got = R.gradient(f, nb, val, R.GD_SR)
    assert got.tobytes() == want.tobytes(), (n_fft, val)


def test_gradient_cases_take_each_branch_at_least_twice():
    uni = [R.gd_is_uniform(n // 2 + 1, v, R.GD_SR) for n, v in GD]
    for (n, v), u, want in zip(GD, uni, GD_UNIFORM):
        print(f"SPEC-REF gd axis n_fft {n} step {v!r}: {'uniform' if u else 'non-uniform'}")
        assert u == want, (n, v, u)
    inner_uniform = [u for (n, v), u in zip(GD, uni) if n >= 4 and u]
    inner_nonuni = [u for (n, v), u in zip(GD, uni) if n >= 4 and not u]
    assert len(inner_uniform) >= 2 and len(inner_nonuni) >= 2, uni
    assert sum(n // 2 - 1 for (n, v), u in zip(GD, uni) if u) >= 16           # interior bins that take the uniform formula


# --------------------------------------------------------------------------------------------------- order statistics
def test_kth_is_the_sorted_value_bit_for_bit():
    for name, v in R.order_stat_segments():
        if v.size == 0:
            assert np.all(np.isnan(R.kth(v, R.order_stat_ranks(0, "edges"))))
            continue
        for kind in ("spread", "median", "edges", "bucket"):
            r = R.order_stat_ranks(v.size, kind, v)
            got = R.kth(v, r)
            rc = np.clip(r, 0, v.size - 1)
            if np.isnan(v).any():
                # np.sort puts every NaN last, whatever its sign, and so does kth; which payload np.sort leaves at which NaN
                # position is not defined, kth gives the quiet NaN there
                want = np.sort(v)[rc]
                isn = np.isnan(want)
                assert np.array_equal(np.isnan(got), isn) and isn.any() == (kind in ("spread", "edges")), (name, kind)
                assert np.array_equal(R.bits64(got[~isn]), R.bits64(want[~isn])), (name, kind)
                assert np.all(R.bits64(got[isn]) == R.bits64([R.QNAN])[0]), (name, kind)
                assert not np.isnan(R.kth(v, [0])[0])                        # a NaN with the sign bit set is not the minimum
                continue
            want = np.sort(v)[rc]
            if np.any(v == 0.0):
                # np.sort leaves +-0 in arrival order; the key order puts -0.0 first: same values, and the signs by count
                assert np.array_equal(got, want), (name, kind)
                nneg0 = int(np.sum((v == 0.0) & np.signbit(v)))
                below = int(np.sum(v < 0.0))
                z = got == 0.0
                assert np.array_equal(np.signbit(got[z]), rc[z] < below + nneg0), (name, kind)
            else:
                assert np.array_equal(R.bits64(got), R.bits64(want)), (name, kind)


def test_order_stat_segments_are_what_they_claim():
    segs = dict(R.order_stat_segments())
    assert {0, 1, 2, 1535, 1536, 1537, 16383, 16384, 16385, 100003} <= {v.size for v in segs.values()}
    for cnt in (R.OS_CAP, R.OS_CAP + 1):
        v = segs[f"bucket {cnt}"]
        top = R.sort_key(v) >> np.uint64(48)
        med = R.sort_key(R.kth(v, [v.size // 2])) >> np.uint64(48)
        assert int(np.sum(top == med[0])) == cnt                                # the median's bucket after two digits
        r = R.order_stat_ranks(v.size, "median")
        lead = {int(x) for x in R.sort_key(R.kth(v, r)) >> np.uint64(48)}
        assert len(lead) <= 4                                                    # few leaders: only the size decides
        lo, hi = R.fullest_bucket(v)
        rb = R.order_stat_ranks(v.size, "bucket", v)
        assert hi - lo == cnt and np.all((rb >= lo) & (rb < hi)) and rb[0] == hi - 1     # one leader, the bucket's last value
        assert {int(x) for x in R.sort_key(R.kth(v, rb)) >> np.uint64(48)} == {int(med[0])}
    v = segs["wide 16385"]
    lead = {int(x) for x in R.sort_key(R.kth(v, R.order_stat_ranks(v.size, "spread"))) >> np.uint64(56)}
    assert len(lead) > 4                                                         # spread ranks: more than four lists wanted
    assert len(np.unique(R.bits64(segs["lowest byte 1535"]) >> np.uint64(8))) <= 2


# ------------------------------------------------------------------------------------------------- summary statistics
def test_stats_float64_evaluation_equals_numpys_expressions():
    for g in R.stats_cases():
        for L, val, m in g["elems"]:
            rec, aux = R.stats(m, L, val, g["f_min"], g["f_max"], g["probe"], dtype=np.float64)
            f = (np.arange(L // 2 + 1) * val).astype(F32)
            sel = (f >= F32(g["f_min"])) & (f <= F32(g["f_max"]))
            assert rec[0] == np.sum(sel)
            assert rec[6] == int(np.argmin(np.abs(f - F32(g["probe"])))) and rec[7] == float(m[int(rec[6])])
            if not sel.any():
                assert rec[1] == 0 and rec[5] == 0.0 and rec[3] == 0.0 and rec[4] == 0.0
                continue
            assert rec[1] == np.flatnonzero(sel)[0] + int(np.argmax(m[sel])), (g["name"], L)
            assert rec[2] == float(f[int(rec[1])]) and rec[5] == float(f[sel][0])
            with np.errstate(over="ignore", invalid="ignore"):
                lin = 10.0 ** (m[sel].astype(np.float64) / 20.0)
                want3, want4 = np.sum(f[sel].astype(np.float64) * lin), np.sum(lin)
            assert np.array_equal([rec[3], rec[4]], [want3, want4], equal_nan=True), (g["name"], L)
            # and the long-double sums the GPU test uses stay within the bound of NumPy's float64 ones
            rl, al = R.stats(m, L, val, g["f_min"], g["f_max"], g["probe"])
            if np.isfinite(want3):
                assert abs(LD(want3) - al["s3"]) <= R.sums_bound(al["abs3"], al["n_in"])
                assert abs(LD(want4) - al["s4"]) <= R.sums_bound(al["abs4"], al["n_in"])


def test_stats_cases_plant_what_they_claim():
    gs = {g["name"]: g for g in R.stats_cases()}
    tie = 0
    for L, val, m in gs["plain"]["elems"]:
        g = gs["plain"]
        f = (np.arange(L // 2 + 1) * val).astype(F32)
        sel = np.flatnonzero((f >= F32(g["f_min"])) & (f <= F32(g["f_max"])))
        if sel.size >= 4:
            top = np.flatnonzero(m[sel] == m[sel].max())
            assert top.size == 2 and R.bits32(m[sel][top])[0] == R.bits32(m[sel][top])[1]     # the planted maxima are equal floats
        d = np.abs(f - F32(g["probe"]))
        tie += int(np.sum(d == d.min()) == 2)                                                 # the probe distances tie in float32
    assert tie >= 1
    g = gs["edges"]
    hit = 0
    for L, val, m in g["elems"]:
        f = (np.arange(L // 2 + 1) * val).astype(F32)
        hit += int(np.any(f == F32(g["f_min"])) and np.any(f == F32(g["f_max"])))
        sel = np.flatnonzero((f >= F32(g["f_min"])) & (f <= F32(g["f_max"])))
        if sel.size >= 2:
            assert int(np.argmax(m[sel])) in (0, sel.size - 1) and m.max() == F32(99.0)
    assert hit >= 3
    assert all(R.stats(m, L, val, gs["empty"]["f_min"], gs["empty"]["f_max"], 1000.0)[0][0] == 0 for L, val, m in gs["empty"]["elems"])
    n_nan = 0
    for L, val, m in gs["nan"]["elems"]:
        rec, _ = R.stats(m, L, val, 20.0, 20000.0, 1000.0)
        if np.isnan(m).any():
            n_nan += 1
            first = int(np.flatnonzero(np.isnan(m))[0])
            assert rec[1] == first and np.isnan(rec[3]) and np.isnan(rec[4])
            assert len({int(b) for b in R.bits32(m[np.isnan(m)])}) == 3                       # both signs and a payload
            assert np.nanmax(m[:first]) == F32(120.0)
    assert n_nan >= 4
    for L, val, m in gs["extremes"]["elems"]:
        if m.size > 100:
            y = np.abs(m.astype(np.float64) * 0.05)
            assert np.any(np.isinf(m)) and np.any((y < 15.0) & (y > 14.9)) and np.any((y > 15.0) & (y < 15.1))


# --------------------------------------------------------------------------------------------------------- smoothing
SMOOTH, SMOOTH_OVER = R.smooth_cases()


@pytest.mark.parametrize("case", SMOOTH, ids=[c["name"] for c in SMOOTH])
def test_log_smooth_float64_evaluation_equals_numpys(case):
    w = case["window"]
    for cs in case["curves"]:
        mat, col = R.smooth_case_arrays(cs)
        curve = mat[:, col]
        k_lo, nsel, fstep = cs["k_lo"], cs["nsel"], cs["fstep"]
        a, b, count = R.ls_geometry(k_lo, nsel, fstep, case["bpo"])
        assert 9 <= count <= R.LS_MAX and w <= count
        fs = R.ls_freq(k_lo + np.arange(nsel), fstep)
        ms = curve[k_lo : k_lo + nsel].astype(np.float64)
        grid = 2 ** np.linspace(a, b, count)
        on = np.interp(grid, fs, ms)
        if case["through"]:
            on = on.astype(F32).astype(np.float64)
        sm = np.convolve(on, np.ones(w) / w, mode="same")
        if case["through"]:
            sm = sm.astype(F32).astype(np.float64)
        want = np.interp(fs, grid, sm) if nsel > 1 or w % 2 == 1 else None
        got = R.log_smooth(curve, k_lo, nsel, fstep, w, case["bpo"], case["through"], dtype=np.float64, parts=True)
        cmax = float(np.max(np.abs(ms)))
        assert np.max(np.abs(got["out"] - want)) <= 4 * w * 2.0 ** -53 * cmax, (case["name"], cs)
        # the long-double evaluation: inner curves keep clear of float32 ties by more than their error bound
        ref = R.log_smooth(curve, k_lo, nsel, fstep, w, case["bpo"], case["through"], parts=True)
        if case["through"]:
            inner = R.smooth_bound(ref, w, cmax, inner=True)
            assert np.min(R.tie_margin32(ref["on"])) > 2 * inner, (case["name"], cs)
            # the averaged curve: clear of ties as well, or -- windows of 1, 2, 8 points: the weights are powers of two, the
            # terms float32 values of one size, so every float64 partial sum is exact in any order -- exactly representable
            clear = R.tie_margin32(ref["sm"]) > 2 * inner
            if w in (1, 2, 8):
                o = np.abs(ref["on"].astype(np.float64))
                assert o.max() / o.min() < 2.0 ** 20
                clear |= ref["sm"].astype(np.float64).astype(LD) == ref["sm"]
            assert np.all(clear), (case["name"], cs)
        assert np.max(np.abs(ref["out"] - got["out"].astype(LD)) - R.smooth_bound(ref, w, cmax) ) <= 0


def test_smooth_geometry_is_what_it_claims():
    counts = set()
    for case in SMOOTH:
        for cs in case["curves"]:
            a, b, count = R.ls_geometry(cs["k_lo"], cs["nsel"], cs["fstep"], case["bpo"])
            counts.add(count)
            if case["name"].startswith("window == count"):
                counts.add(("w==c", count == case["window"]))
            if cs["fstep"] == 1.0:                                     # first and last selected bins are grid points exactly
                assert 2.0 ** a == cs["k_lo"] and 2.0 ** b == cs["k_lo"] + cs["nsel"] - 1
    assert 9 in counts and R.LS_MAX in counts and ("w==c", True) in counts
    assert R.ls_geometry(SMOOTH_OVER["k_lo"], SMOOTH_OVER["nsel"], SMOOTH_OVER["fstep"], 256)[2] == R.LS_MAX + 1
    # the half-window convention of "same" for an even window: numpy keeps one MORE point on the left
    assert np.convolve([0.0, 0.0, 1.0, 0.0, 0.0], np.ones(2), mode="same").tolist() == [0.0, 0.0, 1.0, 1.0, 0.0]


# --------------------------------------------------------------------------------------------------- dB and angle
def test_packed_reference_reproduces_rfft():
    for L, z, pk, x in R.mag_phase_packed_batch():
        if not pk:
            continue
        xr, xi, w, a = R.packed_bins_ld(z, L)
        X = np.fft.rfft(x)
        err = np.hypot(xr - X.real.astype(LD), xi - X.imag.astype(LD))
        assert float(np.max(err)) <= 64 * 2.0 ** -53 * np.max(np.abs(X)), L
        assert xi[0] == 0 and xi[-1] == 0
        # every packed bin is used for the dB bound: none needs a mask
        assert float(np.max(w)) <= R.PACKED_MAX_WEIGHT, (L, float(np.max(w)))
        assert R.PACKED_STEPS >= -(-(L // 2 + 1) // (-(-(max(R.MP_PACKED_LENGTHS) // 2 + 1) // 4096) * 256))


def test_twiddle_is_reduced_exactly():
    for l in (1, 2, 3, 4097, 8193):
        c, s = R.twiddle_ld(np.arange(l + 1), l)
        assert c[0] == 1 and s[0] == 0 and c[-1] == -1 and s[-1] == 0
        if l % 2 == 0:
            assert c[l // 2] == 0 and s[l // 2] == -1
        assert float(np.max(np.abs(c * c + s * s - 1))) < 4 * 2.0 ** -64
        assert np.all(c[: (l + 1) // 2] == -c[::-1][: (l + 1) // 2]) and np.all(s == s[::-1])


@pytest.mark.parametrize("floor_db", R.MP_FLOORS)
def test_mag_phase_inputs_are_what_they_claim(floor_db):
    seen_lib_phase = seen_lib_db = seen_tie = seen_below = 0
    for L, s in R.mag_phase_batch():
        r = R.mag_db_phase(s, L, floor_db)
        # no bin is silently excluded: the two planted one ulp beside the floor may fall on either side of the kernel's
        # comparison of squares (both answers are within the dB bound); every other bin is below, at or above for certain
        near = int(np.sum(r["cls"] < 0))
        assert near <= 2 and near <= 0.01 * max(200, r["cls"].size), (L, floor_db, near)
        seen_tie += int(np.sum(r["cls"] == 1))
        seen_below += int(np.sum(r["cls"] == 0))
        seen_lib_phase += int(np.sum(r["lib_phase"]))
        seen_lib_db += int(np.sum(r["lib_db"]))
    assert seen_tie >= 3 and seen_below >= (100 if floor_db > -1000 else 4) and seen_lib_phase >= 30 and seen_lib_db >= 10
    big = dict(R.mag_phase_batch())[16386]
    for z in R.floor_tie_bins(floor_db):                                         # the floor-tie bins really tie, in both domains
        f = R.floor_lin_of(floor_db)
        assert np.hypot(LD(z.real), LD(z.imag)) == LD(f)
        assert z.real * z.real + z.imag * z.imag == f * f
    assert R.floor_lin_of(-2900.0) < 1e-140 < R.floor_lin_of(-300.0) < R.floor_lin_of(-120.0)
    assert (floor_db == -2900.0) == bool(np.all(R.mag_db_phase(big, 16386, floor_db)['lib_db']))
    pl = R.planted_bins()
    assert all(np.any(R.bits64(big.real) == R.bits64([z.real])[0]) for z in pl[:40])
    with np.errstate(all="ignore"):
        t = np.abs(pl.imag) / np.abs(pl.real)
        for k in range(65):                                                      # every table knot, and midway to the next
            assert np.any(t == k / 64.0) and (k == 64 or np.any(t == (k + 0.5) / 64.0))


def test_phase_bound_is_a_few_ulp():
    rng = np.random.default_rng(1)
    s = R.random_bins(rng, 20000)
    r = R.mag_db_phase(s, 2 * (s.size - 1), -120.0)
    b = R.phase_bound(r["re"], r["im"], r["lib_phase"])
    ulps = b / R.ulp64(r["phase"].astype(np.float64))
    print(f"SPEC-REF phase bound: {ulps.min():.2f} .. {ulps.max():.2f} ulp of the result (median {np.median(ulps):.2f})")
    assert ulps.max() <= 13.3 + 0.1 and np.median(ulps) <= 6.0
