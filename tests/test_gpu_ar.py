"""
GPU: the AR normal-equation kernels in front of the root finder (ira_ar.hip: ar_lag_kernel<16|13|12|10|8>, ar_gram_kernel,
ar_solve_wave_kernel, ar_solve_kernel LDS and blocked, ar_grad_kernel, ar_lag_dd_kernel / ar_solve_dd_kernel,
ar_minnorm_kernel) held to the long-double and exact references of tests/ar_ref.py (pinned by tests/test_ar_ref_cpu.py).

Two drivers: Engine.ar_fit, and poisoned_fit -- the same calls through eng.lib with every scratch and output buffer filled
with NaN first, so that a kernel which reads a slot it did not write (a short element of a ragged batch reading the chunk
slots of the longest one) shows up as NaN.  Every ragged batch goes through poisoned_fit and every element is run alone as
well: coefficients and info must be the batch's bits.

  (a) backward error eta(G_ld, r_ld, a_dev) <= (rows + 4 p + 8) u on the lag-sum path: one order per lag-kernel instantiation,
      both sides of every solver boundary (wave | workgroup | blocked, panel 32 | 16), the API limit, row counts 2p+1 and
      4096 k +- 1, ridge, float64 samples with a divisor;
  (b) the same on the dense matrix-core Gram (rows = 1, 2, 3 mod 4, 1024 +- 1, 8192 +- 1);
  (c) fewer rows than unknowns and exactly periodic signals: numpy.linalg.lstsq's minimum-norm solution to 1e-8;
  (d) forward error against the EXACT rational solution where float64 lstsq is itself the limit: refined (class R) and
      double-double (class D) fits through the wave, workgroup and blocked kernels, low- and high-passed, with teeth;
  (e) the info record: pivots against a long-double Cholesky, the condition estimate within [0.25, p] cond_2(G);
  (f) a NaN or infinite sample: status 3 at every order, with or without a ridge.

Measured on an MI355X (AR-ERR lines print the same per case):
  share of the eta allowance   lag path 2.6 % at worst (order 1, where the allowance is smallest; <= 1.4 % from order 2 on,
                               <= 0.2 % from order 63 on), dense matrix-core Gram 4.5 % at worst (order 1 with 4 rows;
                               <= 0.8 % otherwise).  A dropped boundary row exceeds the allowance >= 3e5 fold (CPU teeth).
  forward error, class R       device / lstsq 0.03 .. 0.54 (device 4e-13 .. 3e-12 of the largest coefficient, lstsq
                               2e-12 .. 2e-11); without refinement 2e-7 .. 1e-5.
  forward error, class D       device / lstsq < 1e-6 (device 0 .. 1e-16: the correctly rounded exact solution or its
                               neighbour; lstsq 4e-11 .. 8e-9); without the double-double path 3e-8 .. 1e-2 -- the
                               narrowest teeth are order 130 low-passed, 2.9e-8 against an allowed 1.4e-9.
  est / cond_2(G)              minimum 1.000 (order 1), 2.1 on the high-passed class inputs (order 64), maximum 92 (order
                               385): inside [0.25, p].  The float64 emulation goes down to 0.31 on mildly high-passed
                               noise at even order (tests/test_ar_ref_cpu.py), which is why the floor is 0.25 and not 1.
"""
import functools

import numpy as np
import pytest

import ar_ref as R

pytestmark = pytest.mark.gpu


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


# ------------------------------------------------------------------------------------------------------- drivers
def _upload(eng, chans, f64=False):
    """One flat device buffer; the first element starts at an ODD index (no element is aligned to more than its type)."""
    dt = np.float64 if f64 else np.float32
    lens = np.array([c.size for c in chans], np.int64)
    off = 1 + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    flat = np.zeros(1 + int(lens.sum()), dt)
    for c, o in zip(chans, off):
        assert c.dtype == dt
        flat[o : o + c.size] = c
    return eng.to_dev(flat), off, lens.astype(np.int32)


def engine_fit(eng, chans, order, ridge=0.0, f64=False, divisor=None):
    x, off, lens = _upload(eng, chans, f64)
    div = None if divisor is None else np.full(len(chans), divisor, np.float64)
    co, info = eng.ar_fit(x, off, lens, div, order, ridge=ridge, x_is_f64=f64)
    return co.cpu().numpy().copy(), info.cpu().numpy().copy()


def poisoned_fit(eng, chans, order, ridge=0.0, f64=False, divisor=None):
    """Engine.ar_fit call for call, condition for condition -- on buffers of its own, all NaN before the first launch."""
    from audio_analysis_amd._lib import check
    from audio_analysis_amd.engine import _ptr
    t, lib = eng.torch, eng.lib
    x_dev, xoff, lengths = _upload(eng, chans, f64)
    n, max_len = len(chans), int(lengths.max())

    def nan(count):
        return t.full((int(max(count, 1)),), float("nan"), dtype=t.float64, device=eng.device)

    per = int(lib.ira_ar_partial_doubles(int(order), max_len))
    assert per > 0
    part = nan(n * per)
    gs = nan(n * order * order) if order > 128 else None
    coeffs, info = nan(n * (order + 1)), nan(n * 4)
    # the job tables stay referenced (tables) until every launch that reads them is enqueued: the function returns after that
    tables = eng.job_tables(np.ascontiguousarray(xoff, np.int64), lengths,
                            np.full(n, divisor, np.float64) if divisor is not None else None)
    d_xo, d_l, d_div = tables
    flags = (1 if eng.ar_dense_gram else 0) | (2 if eng.ar_workgroup_solve else 0)
    x32, x64 = (0, _ptr(x_dev)) if f64 else (_ptr(x_dev), 0)
    st = eng.stream
    check(lib.ira_ar_gram(x32, x64, _ptr(d_xo), _ptr(d_l), _ptr(d_div), n, max_len, int(order), _ptr(part), flags, st),
          "ira_ar_gram")
    check(lib.ira_ar_solve(_ptr(part), _ptr(d_l), n, max_len, int(order), float(ridge), _ptr(gs), _ptr(coeffs), _ptr(info),
                           flags, st), "ira_ar_solve")
    keep = [part, gs, tables, x_dev]
    if eng.ar_exact_cond > 0.0 and not eng.ar_dense_gram:
        ddp = nan(n * int(lib.ira_ar_exact_doubles(int(order), max_len, 0)))
        dds = nan(n * int(lib.ira_ar_exact_doubles(int(order), max_len, 1)))
        keep += [ddp, dds]
        check(lib.ira_ar_exact(x32, x64, _ptr(d_xo), _ptr(d_l), _ptr(d_div), n, max_len, int(order), float(ridge), _ptr(part),
                               _ptr(ddp), _ptr(dds), _ptr(coeffs), _ptr(info), float(eng.ar_exact_cond), st), "ira_ar_exact")
    if ridge == 0.0 and order <= 512 and eng.ar_minnorm_cut > 0.0 and not eng.ar_dense_gram:
        scratch2 = nan(n * 2 * order * order)
        keep.append(scratch2)
        check(lib.ira_ar_minnorm(_ptr(part), _ptr(d_l), n, max_len, int(order), _ptr(scratch2), _ptr(coeffs), _ptr(info),
                                 float(eng.ar_minnorm_cut), st), "ira_ar_minnorm")
    if ridge == 0.0 and eng.ar_refine_steps > 0:
        nchunks = -(-(max_len - int(order)) // 4096)
        grad = nan(n * nchunks * (order + 1))
        keep.append(grad)
        check(lib.ira_ar_refine(x32, x64, _ptr(d_xo), _ptr(d_l), _ptr(d_div), n, max_len, int(order), _ptr(part), _ptr(gs),
                                _ptr(coeffs), _ptr(info), _ptr(grad), float(eng.ar_refine_cond), int(eng.ar_refine_steps),
                                flags, st), "ira_ar_refine")
    co = coeffs.view(n, order + 1).cpu().numpy().copy()          # the copy waits for the stream; `keep` is alive until here
    inf = info.view(n, 4).cpu().numpy().copy()
    del keep
    return co, inf


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _batch_and_solo(eng, chans, order, **kw):
    """The ragged batch through poisoned_fit; every element alone through Engine.ar_fit: the same bits."""
    co, info = poisoned_fit(eng, chans, order, **kw)
    for i, c in enumerate(chans):
        co1, info1 = engine_fit(eng, [c], order, **kw)
        assert _same_bits(co1[0], co[i]), ("coefficients of element", i, "differ between the batch and the solo run", order)
        assert _same_bits(info1[0], info[i]), ("info of element", i, info1[0], info[i], order)
    return co, info


def test_poisoned_fit_is_engine_ar_fit():
    eng = _eng()
    chans = [R.grid_signal(64, rows) for rows in (5000, 9000, 700)]
    for order in (12, 64, 130):
        a, ia = engine_fit(eng, chans, order)
        b, ib = poisoned_fit(eng, chans, order)
        assert _same_bits(a, b) and _same_bits(ia, ib), order
        assert np.all(ia[:, 0] == 0.0)


# ------------------------------------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def _ref(p, rows, f64=False, ridge=0.0):
    """Long-double G, r and the info yardsticks of a grid case: computed once, shared by (a) and (e), never modified."""
    x = R.grid_signal(p, rows, f64=f64)
    s = R.samples(x, 0.3 if f64 else None, f64)
    G, r = R.gram_ld(s, p, ridge=ridge)
    G.setflags(write=False), r.setflags(write=False), x.setflags(write=False)
    return dict(x=x, G=G, r=r, cond=R.cond2(s, p, ridge), piv=R.pivots_ld(G))


def _check_eta(tag, p, rows, ref, a_dev, info_dev, shares):
    assert info_dev[0] == 0.0, (tag, p, rows, info_dev)
    assert a_dev[0] == 1.0 and np.all(np.isfinite(a_dev))
    share = R.eta(ref["G"], ref["r"], a_dev[1:]) / R.eta_allowance(rows, p)
    shares.append(share)
    print(f"AR-ERR {tag} p={p} rows={rows}: {100 * share:.3f} % of the allowance")
    assert share <= 1.0, (tag, p, rows, share)
    return share


def _check_info(p, rows, ref, info_dev):
    """(e): pivots within 8 p cond u of the long-double Cholesky's, the estimate within [0.25, p] cond_2(G)."""
    cond = ref["cond"]
    tol = 8 * p * cond * R.U
    hi, lo = ref["piv"]
    assert abs(info_dev[1] - hi) <= tol * hi, (p, rows, info_dev[1], hi, tol)
    assert abs(info_dev[2] - lo) <= tol * lo, (p, rows, info_dev[2], lo, tol)
    ratio = info_dev[3] / cond
    print(f"AR-ERR est/cond p={p} rows={rows}: {ratio:.3f}")
    assert info_dev[3] <= p * cond * (1 + 1e-6), (p, rows, info_dev[3], cond)
    assert info_dev[3] >= 0.25 * cond, (p, rows, info_dev[3], cond)
    return ratio


# ------------------------------------------------------------------------------------------------------- (a) + (e)
@pytest.mark.parametrize("order", R.ORDERS_A)
def test_backward_error_and_info_on_the_lag_path(order):
    R.need_longdouble()
    eng = _eng()
    rows_list = R.rows_for(order)
    assert max(rows_list) != rows_list[-1]                        # the longest element is not the last one
    refs = [_ref(order, rows) for rows in rows_list]
    for ref in refs:
        assert order * ref["cond"] < 1e9                          # stays clear of refinement: status 0 is the right answer
    co, info = _batch_and_solo(eng, [ref["x"] for ref in refs], order)
    assert not np.any(np.isnan(co)) and not np.any(np.isnan(info)), "a kernel read scratch it had not written"
    shares, ratios = [], []
    for i, (rows, ref) in enumerate(zip(rows_list, refs)):
        _check_eta("lag", order, rows, ref, co[i], info[i], shares)
        ratios.append(_check_info(order, rows, ref, info[i]))
    print(f"AR-ERR lag p={order}: worst share {100 * max(shares):.3f} %, est/cond {min(ratios):.3f} .. {max(ratios):.3f}")
    assert max(shares) <= 1.0, (order, list(zip(rows_list, shares)))


@pytest.mark.parametrize("order", (64, 130))
def test_backward_error_with_a_ridge(order):
    R.need_longdouble()
    eng = _eng()
    rows_list = R.rows_for(order)
    refs = [_ref(order, rows, ridge=1e-3) for rows in rows_list]
    co, info = _batch_and_solo(eng, [ref["x"] for ref in refs], order, ridge=1e-3)
    shares = []
    for i, (rows, ref) in enumerate(zip(rows_list, refs)):
        _check_eta("lag+ridge", order, rows, ref, co[i], info[i], shares)
        _check_info(order, rows, ref, info[i])
    assert max(shares) <= 1.0, (order, list(zip(rows_list, shares)))


@pytest.mark.parametrize("order", (12, 65, 130))
def test_backward_error_on_float64_samples_with_a_divisor(order):
    R.need_longdouble()
    eng = _eng()
    rows_list = R.rows_for(order)
    refs = [_ref(order, rows, f64=True) for rows in rows_list]
    assert all(np.any(ref["x"] != ref["x"].astype(np.float32)) for ref in refs)          # genuinely 53-bit samples
    co, info = _batch_and_solo(eng, [ref["x"] for ref in refs], order, f64=True, divisor=0.3)
    shares = []
    for i, (rows, ref) in enumerate(zip(rows_list, refs)):
        _check_eta("lag+f64", order, rows, ref, co[i], info[i], shares)
        _check_info(order, rows, ref, info[i])
    assert max(shares) <= 1.0, (order, list(zip(rows_list, shares)))


# ------------------------------------------------------------------------------------------------------- (b)
def _dense_rows(p):
    return (p + 3, 1023, 8193, 1025, 8191, 1101, 1102, 1103)      # 1101, 1102, 1103 = 1, 2, 3 mod 4; the longest not last


@pytest.mark.parametrize("order", (1, 63, 64, 65, 130))
def test_backward_error_on_the_dense_matrix_core_gram(order):
    R.need_longdouble()
    eng = _eng()
    rows_list = _dense_rows(order)
    assert {r % 4 for r in rows_list} >= {1, 2, 3}
    refs = [_ref(order, rows) for rows in rows_list]
    try:
        eng.ar_dense_gram = True
        co, info = _batch_and_solo(eng, [ref["x"] for ref in refs], order)
    finally:
        eng.ar_dense_gram = False
    shares = []
    for i, (rows, ref) in enumerate(zip(rows_list, refs)):
        _check_eta("dense", order, rows, ref, co[i], info[i], shares)
    print(f"AR-ERR dense p={order}: worst share {100 * max(shares):.3f} %")
    assert max(shares) <= 1.0, (order, list(zip(rows_list, shares)))


# ------------------------------------------------------------------------------------------------------- (c)
def _lstsq(x, p):
    A, y = R.design(R.samples(x), p)
    return np.linalg.lstsq(A, y, rcond=None)[0]


def _check_minnorm(tag, order, chans, max_rank, co, info):
    for i, x in enumerate(chans):
        assert info[i, 0] == 4.0, (tag, order, i, info[i])
        assert 1 <= info[i, 3] <= max_rank[i] and info[i, 3] == int(info[i, 3]), (tag, order, i, info[i])
        ref = _lstsq(x, order)
        err = float(np.max(np.abs(co[i, 1:] - ref)))
        scale = max(1.0, float(np.max(np.abs(ref))))
        print(f"AR-ERR {tag} p={order} rows={x.size - order}: rank {int(info[i, 3])}, |a - lstsq| = {err:.2e} (allowed {1e-8 * scale:.1e})")
        assert co[i, 0] == 1.0 and err <= 1e-8 * scale, (tag, order, i, err)


MINNORM_ORDERS = (8, 33, 65, 129, 257)


@pytest.mark.parametrize("order", MINNORM_ORDERS)
def test_fewer_rows_than_unknowns(order):
    eng = _eng()
    rows_list = (2, order - 1, 1)
    chans = [R.stationary(50 * order + rows, order + rows, R.POLES[rows % 3]) for rows in rows_list]
    co, info = _batch_and_solo(eng, chans, order)
    _check_minnorm("short", order, chans, rows_list, co, info)


def _periodic(seed, period, n):
    v = np.random.default_rng(seed).integers(-3, 4, period)
    v[0] = 3                                                       # not all zero
    return np.tile(v, n // period + 1)[:n].astype(np.float32)


PERIODIC_ORDERS = (33, 65, 129, 257)


@pytest.mark.parametrize("order", PERIODIC_ORDERS)
def test_exactly_periodic_signals(order):
    """Small integers with period 3, 6, 20: every entry of the Gram matrix is an integer below 2^53, exact in float64, and its
    rank is at most the period.  (Order 512, the cap of ar_minnorm_kernel, has a test of its own below.)"""
    eng = _eng()
    periods = (6, 20, 3)
    chans = [_periodic(order + per, per, n) for per, n in zip(periods, (2 * order + 50, 4 * order + 1, 3 * order + 7))]
    co, info = _batch_and_solo(eng, chans, order)
    _check_minnorm("periodic", order, chans, periods, co, info)


def test_order_512_the_cap_of_the_minimum_norm_kernel():
    """Timed once on an MI355X: this batch of three (periods 6, 20, 3 at order 512) takes ar_minnorm_kernel 7.4 s -- too slow
    for the suite; its period-6 element alone takes 3.5 s and is what runs here (every strided loop of the 256-thread
    workgroup wraps twice, the LDS vectors are full).  All three elements agreed with lstsq to 2e-15 in that run."""
    eng = _eng()
    chans = [_periodic(512 + 6, 6, 2 * 512 + 50)]
    co, info = poisoned_fit(eng, chans, 512)
    _check_minnorm("periodic", 512, chans, (6,), co, info)


def test_order_513_rank_deficient_is_status_1():
    """Above order 512 ar_minnorm_kernel does not run: include/ira.h promises status 1 (a pivot was not positive) there."""
    eng = _eng()
    chans = [_periodic(9, 6, 2000), R.grid_signal(513, 1027)]
    co, info = engine_fit(eng, chans, 513)
    assert info[0, 0] == 1.0 and info[1, 0] == 0.0, info[:, 0]


# ------------------------------------------------------------------------------------------------------- (d)
@functools.lru_cache(maxsize=None)
def _class_ref(case):
    p, rows, kind, cls, width = case
    x = R.class_signal(p, rows, kind, width)
    s = R.samples(x)
    A, y = R.design(s, p)
    sv = np.linalg.svd(A, compute_uv=False)
    exact = R.exact_fit(s, p)
    lstsq = np.linalg.lstsq(A, y, rcond=None)[0]
    scale = float(np.max(np.abs(exact)))
    x.setflags(write=False), exact.setflags(write=False)
    return dict(x=x, exact=exact, scale=scale, cond=float((sv[0] / sv[-1]) ** 2), ratio=float(sv[-1] / sv[0]),
                err_lstsq=float(np.max(np.abs(lstsq - exact))) / scale)


def _class_id(case):
    return f"p{case[0]}-{case[2]}-{case[3]}"


@pytest.mark.parametrize("case", R.CLASS_CASES, ids=_class_id)
def test_forward_error_against_the_exact_solution(case):
    p, rows, kind, cls, width = case
    ref = _class_ref(case)
    assert R.in_class(cls, p, rows, ref["cond"], ref["ratio"]), (case, ref["cond"], ref["ratio"])    # before the device is asked
    eng = _eng()
    allowed = max(4.0 * ref["err_lstsq"], 1e-13)

    def fit():
        co, info = engine_fit(eng, [ref["x"]], p)
        return float(np.max(np.abs(co[0, 1:] - ref["exact"]))) / ref["scale"], co, info

    err, co, info = fit()
    print(f"AR-ERR class {cls} {kind} p={p}: cond {ref['cond']:.2e}, device {err:.2e}, lstsq {ref['err_lstsq']:.2e}, "
          f"device/lstsq {err / ref['err_lstsq']:.3f}, est/cond {info[0, 3] / ref['cond']:.3f}")
    assert info[0, 0] == (2.0 if cls == "R" else 5.0), (case, info[0])
    assert co[0, 0] == 1.0 and err <= allowed, (case, err, ref["err_lstsq"])
    assert info[0, 3] >= 0.25 * ref["cond"], (case, info[0, 3], ref["cond"])
    # teeth: without the path under test the same assertion fails
    name, off = ("ar_refine_steps", 0) if cls == "R" else ("ar_exact_cond", 0.0)
    saved = getattr(eng, name)
    try:
        setattr(eng, name, off)
        err0, _, info0 = fit()
    finally:
        setattr(eng, name, saved)
    print(f"AR-ERR class {cls} {kind} p={p}: with {name} = 0: {err0:.2e} (status {info0[0, 0]:.0f})")
    assert not (err0 <= allowed), (case, err0, allowed)


# ------------------------------------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("order,ridge", [(16, 0.0), (130, 0.0), (513, 0.0), (64, 1e-3)])
@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_a_sample_that_is_not_finite_is_status_3(order, ridge, poison):
    eng = _eng()
    good = R.grid_signal(order, 2 * order + 1)
    bad = R.grid_signal(order, 4097).copy()
    # in the middle; the very last sample (no diagonal entry of A^T A squares it); the first (only a head correction sees it)
    bad[{16: order + 1500, 130: bad.size - 1, 513: 0, 64: order + 1500}[order]] = poison
    co, info = engine_fit(eng, [bad, good], order, ridge=ridge)
    assert info[0, 0] == 3.0, (order, ridge, info[0])
    assert co[0, 0] == 1.0 and np.all(np.isnan(co[0, 1:]))
    co1, info1 = engine_fit(eng, [good], order, ridge=ridge)
    assert info1[0, 0] == 0.0 and _same_bits(co1[0], co[1]) and _same_bits(info1[0], info[1])
    if order == 513 or ridge > 0.0:                               # where no minimum-norm kernel runs: the drop-in API raises
        from audio_analysis_amd.analyse import zplane                 # like the reference's lstsq
        with pytest.raises(np.linalg.LinAlgError):
            zplane._fit_ar_least_squares(bad.astype(np.float64), order, ridge)
    if order <= 64:                                               # the workgroup kernel reports it like the one-wave kernel
        try:
            eng.ar_workgroup_solve = True
            cow, infow = engine_fit(eng, [bad, good], order, ridge=ridge)
        finally:
            eng.ar_workgroup_solve = False
        assert infow[0, 0] == 3.0 and cow[0, 0] == 1.0 and np.all(np.isnan(cow[0, 1:]))
        assert _same_bits(cow[1], co[1]) and _same_bits(infow[1], info[1])


@pytest.mark.parametrize("where", ["middle", "last"])
def test_not_finite_on_the_dense_gram_is_status_3(where):
    """The dense Gram never squares the last sample (no column of A holds s[N-1]): there only the right-hand side is NaN."""
    eng = _eng()
    order = 65
    good = R.grid_signal(order, 1023)
    bad = R.grid_signal(order, 1025).copy()
    bad[700 if where == "middle" else bad.size - 1] = np.nan
    try:
        eng.ar_dense_gram = True
        co, info = engine_fit(eng, [bad, good], order)
        co1, info1 = engine_fit(eng, [good], order)
    finally:
        eng.ar_dense_gram = False
    assert info[0, 0] == 3.0 and co[0, 0] == 1.0 and np.all(np.isnan(co[0, 1:])), info[0]
    assert info1[0, 0] == 0.0 and _same_bits(co1[0], co[1]) and _same_bits(info1[0], info[1])
