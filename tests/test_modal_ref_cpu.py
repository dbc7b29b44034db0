"""tests/modal_ref.py on a machine without a GPU: the restatements agree with the oracle, and the case tables of
tests/test_gpu_modal_kernels.py, judged by the comparison functions those tests use, reject every subtly wrong kernel
modelled here in NumPy (and accept the right one)."""
import numpy as np
import pytest

import modal_ref as R
from oracle import ira_oracle as O


@pytest.fixture(scope="module", autouse=True)
def _longdouble():
    R.need_longdouble()


# ----------------------------------------------------------------------------------------------------------- waterfall
def _formula(m, k_lo, nsel, slice_max, dyn):
    """The reference's lines (waterfall.py:308-341, as the oracle's analyse_waterfall states them)."""
    sl = m[k_lo:k_lo + nsel].T.astype(np.float32)
    with np.errstate(invalid="ignore"):
        rel = sl - np.max(sl, axis=1, keepdims=True) if slice_max else sl - float(np.max(sl))
        return np.clip(rel, -float(dyn), 0.0).astype(np.float32)


@pytest.mark.parametrize("k_lo,nsel", R.WF_SELECTIONS)
def test_waterfall_rel_is_the_references_formula_bit_for_bit(k_lo, nsel):
    for slice_max in (False, True):
        for dyn in (d for d in R.WF_DYN if float(np.float32(d)) == d):
            for m in R.waterfall_case(k_lo, nsel, slice_max, dyn):
                got, ref = R.waterfall_rel(m, k_lo, nsel, slice_max, dyn), _formula(m, k_lo, nsel, slice_max, dyn)
                assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape == (m.shape[1], nsel)
                assert np.array_equal(got.view(np.uint32)[~np.isnan(ref)], ref.view(np.uint32)[~np.isnan(ref)])
                assert np.array_equal(np.isnan(got), np.isnan(ref))


def test_waterfall_table_holds_what_it_says():
    seen = dict(nan=0, posinf=0, dead=0, at=0, below=0, above=0, tie=0)
    for k_lo, nsel, sm, dyn in R.waterfall_cases():
        for m in R.waterfall_case(k_lo, nsel, sm, dyn):
            sel = m[k_lo:k_lo + nsel]
            out = np.delete(m, np.s_[k_lo:k_lo + nsel], axis=0)
            assert np.isnan(out).any() and np.nanmax(out) > 0.0 >= np.nanmax(np.where(np.isinf(sel), -1.0, sel))
            seen["nan"] += int(np.isnan(sel).any())
            seen["posinf"] += int(np.isposinf(sel).any())
            seen["dead"] += int(np.any(np.all(np.isneginf(sel), axis=0)))
            with np.errstate(invalid="ignore"):
                level = np.max(sel, axis=0, keepdims=True) if sm else np.max(sel)
                rel = sel - level
                seen["tie"] += int(np.any(np.sum(rel == 0, axis=0) > 1) if sm else np.sum(rel == 0) > 1)
            lo = -np.float32(dyn)
            seen["at"] += int(np.any(rel == lo))
            seen["below"] += int(np.any((rel < lo) & (rel > lo - np.float32(1e-3))))
            seen["above"] += int(np.any((rel > lo) & (rel < lo + np.float32(1e-3))))
    assert all(v > 0 for v in seen.values()), seen


def _wf_model(m, k_lo, nsel, slice_max, dyn, shift=0, outside=False, drop_nan=False):
    sel = m[k_lo + shift:k_lo + shift + nsel]
    src = m if outside else sel
    red = np.fmax.reduce if drop_nan else np.maximum.reduce
    with np.errstate(invalid="ignore"):
        level = red(src, axis=0)[None, :] if slice_max else red(src, axis=None)
        rel = sel - level
        return np.ascontiguousarray(np.minimum(np.maximum(rel, -np.float32(dyn)), np.float32(0)).T)


WF_MUTANTS = {
    "k_lo off by one": lambda m, k, n, sm, d: _wf_model(m, k, n, sm, d, shift=1),
    "global maximum where the per-slice one is asked for": lambda m, k, n, sm, d: _wf_model(m, k, n, False, d),
    "per-slice maximum where the global one is asked for": lambda m, k, n, sm, d: _wf_model(m, k, n, True, d),
    "maximum over the rows outside the selection too": lambda m, k, n, sm, d: _wf_model(m, k, n, sm, d, outside=True),
    "NaN dropped from the maximum": lambda m, k, n, sm, d: _wf_model(m, k, n, sm, d, drop_nan=True),
}


def _wf_rejections(model):
    hits = 0
    for k_lo, nsel, sm, dyn in R.waterfall_cases():
        for m in R.waterfall_case(k_lo, nsel, sm, dyn):
            try:
                R.check_waterfall(model(m, k_lo, nsel, sm, dyn), R.waterfall_rel(m, k_lo, nsel, sm, dyn))
            except AssertionError:
                hits += 1
    return hits


def test_waterfall_table_accepts_the_right_kernel():
    assert _wf_rejections(_wf_model) == 0


@pytest.mark.parametrize("name", sorted(WF_MUTANTS))
def test_waterfall_table_rejects(name):
    assert _wf_rejections(WF_MUTANTS[name]) > 0, name


# ------------------------------------------------------------------------------------------------------------- log bins
@pytest.mark.parametrize("nrows,k_base", [g for g in R.LB_GEOMETRIES if g[0] < 8193])
def test_logbin_agrees_with_the_oracle(nrows, k_base):
    """The oracle takes bins as frequency edges: row indices as frequencies, and the packed bins of the table as edges
    (an empty bin has equal edges).  Its float64 numpy.mean and this long-double sum agree to one float32 ulp."""
    first, count, mats, refs = R.logbin_case(nrows, k_base)
    edges = np.zeros(count.size + 1, np.float32)
    edges[-1] = first[-1] + count[-1]
    for b in range(count.size - 1, -1, -1):
        edges[b] = first[b] if count[b] > 0 else edges[b + 1]
        assert count[b] == 0 or first[b] + count[b] == edges[b + 1]        # the bins of this geometry are packed
    freq = np.arange(nrows - k_base, dtype=np.float32)
    _, f_o, c_o = O.log_bin_membership(freq, edges)
    assert np.array_equal(c_o, count) and np.array_equal(f_o[count > 0], first[count > 0])
    for m, ref in zip(mats, refs):
        with np.errstate(all="ignore"):
            _, want = O.aggregate_log_bins(freq, m[k_base:], edges)
        got = ref.astype(np.float32)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        inf = np.isinf(want)
        assert np.array_equal(got[inf], want[inf])
        ok = ~np.isnan(want) & ~inf
        assert np.all(np.abs(got[ok].astype(np.float64) - want[ok]) <= np.spacing(np.abs(want[ok])))
        # the restatement of the frame-major layout is the same numbers
        assert np.array_equal(R.logbin(np.ascontiguousarray(m.T), k_base, first, count, True)[1], got, equal_nan=True)


def test_logbin_table_holds_what_it_says():
    for nrows, k_base in R.LB_GEOMETRIES:
        first, count, mats, refs = R.logbin_case(nrows, k_base)
        assert sorted(count) == sorted(R.LB_COUNTS) and k_base + first[-1] + count[-1] == nrows
        for e, (m, ref) in enumerate(zip(mats, refs)):
            T = m.shape[1]
            by = {int(c): ref[b] for b, c in enumerate(count)}
            assert np.all(by[8].astype(np.float32) == np.float32(-600.0)) and np.all(np.isnan(by[0]))
            assert np.isposinf(by[10][T - 1]) and np.isfinite(by[9]).all() and np.all(np.abs(by[2] + 6.0206) < 1e-4)
            nan = np.zeros(ref.shape, bool)
            nan[list(count).index(0)] = True
            nan[list(count).index(18), T // 2] = True
            nan[list(count).index(300), 0] = e == 1
            assert np.array_equal(np.isnan(ref), nan)


def test_logbin_bound_is_the_stated_allowance():
    assert R.logbin_bound_db(1) == 20.0 / np.log(10.0) * 10.0 * 2.0 ** -53
    assert float(R.ulp32(np.longdouble(-600.0))) == 2.0 ** -14 and float(R.ulp32(np.longdouble(1.0))) == 2.0 ** -23
    assert float(R.ulp32(np.longdouble(0.999))) == 2.0 ** -24


def _lb_model(m, k_base, first, count, shift=0, div_extra=0, fmax_clamp=False, skip_last_of=()):
    """The device's chain in float64 NumPy, with the mistakes a kernel could make as options."""
    out = np.full((count.size, m.shape[1]), np.nan, np.float32)
    with np.errstate(all="ignore"):
        lin = 10.0 ** (m.astype(np.float64) / 20.0)
        for b, c in enumerate(count):
            if c <= 0:
                continue
            rows = lin[k_base + first[b] + shift:k_base + first[b] + shift + c]
            if c in skip_last_of:
                rows = rows[:-1]
            acc = rows[0].copy()
            for r in rows[1:]:
                acc = acc + r
            mean = acc / float(c + div_extra)
            mean = np.fmax(mean, 1e-30) if fmax_clamp else np.maximum(mean, 1e-30)
            out[b] = (20.0 * np.log10(mean)).astype(np.float32)
    return out


LB_MUTANTS = {
    "rows first + 1": dict(shift=1),
    "divisor count + 1": dict(div_extra=1),
    "fmax loses the NaN": dict(fmax_clamp=True),
    "last of 9 rows left out": dict(skip_last_of=(9,)),
    "last of 17 rows left out": dict(skip_last_of=(17,)),
}


def _lb_rejections(**kw):
    hits = 0
    for nrows, k_base in R.LB_GEOMETRIES:
        first, count, mats, refs = R.logbin_case(nrows, k_base)
        for m, ref in zip(mats, refs):
            try:
                R.check_logbin(_lb_model(m, k_base, first, count, **kw), ref, count)
            except AssertionError:
                hits += 1
    return hits


def test_logbin_table_accepts_the_right_kernel():
    assert _lb_rejections() == 0


@pytest.mark.parametrize("name", sorted(LB_MUTANTS))
def test_logbin_table_rejects(name):
    assert _lb_rejections(**LB_MUTANTS[name]) > 0, name


def test_fmax_mutant_is_rejected_for_the_nan_alone():
    """The parent commit's kernels: -600 dB where a row holds a NaN, everything else right."""
    first, count, mats, refs = R.logbin_case(383, 0)
    got = _lb_model(mats[2], 0, first, count, fmax_clamp=True)
    with pytest.raises(AssertionError, match="NaN cells differ"):
        R.check_logbin(got, refs[2], count)
    b, t = list(count).index(18), mats[2].shape[1] // 2
    assert got[b, t] == np.float32(-600.0)
    got[b, t] = np.nan
    R.check_logbin(got, refs[2], count)
