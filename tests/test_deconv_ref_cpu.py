"""tests/deconv_ref.py on a machine without a GPU: the restatements, composed with numpy.fft, agree with the oracle on the
small ragged batch of tests/test_gpu_deconvolve.py (and sit far inside its tolerance, by a direct long-double DFT at
the sizes that allow one), and the case tables of tests/test_gpu_deconv_kernels.py, judged by the comparison functions
those tests use, reject every subtly wrong kernel modelled here in NumPy (and accept the right one)."""
import numpy as np
import pytest

import deconv_ref as R
from oracle import ira_oracle as O

LD = np.longdouble


@pytest.fixture(scope="module", autouse=True)
def _longdouble():
    R.need_longdouble()


def _close(got, ref, what, factor=1.0):
    """The tolerance of tests/test_gpu_deconvolve.py: |dh| <= 2e-7 peak + 2e-7 |h|."""
    assert got.shape == ref.shape, what
    peak = float(np.max(np.abs(ref)))
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    assert np.all(err <= factor * (2e-7 * peak + 2e-7 * np.abs(ref))), (what, float(err.max()), peak)


# ---------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("mode,reg", R.E2E_SETTINGS)
def test_restatements_with_numpy_fft_agree_with_the_oracle(mode, reg):
    for i, (rec, sweep) in enumerate(R.e2e_files()):
        got, _ = R.deconvolve_f64(rec, sweep, reg, mode=mode)
        ref = O.deconvolve(rec, sweep, regularization_relative=reg, output_length_mode=mode)
        assert got.dtype == ref.dtype == np.float32
        _close(got, ref, f"file {i} {mode} {reg}")
        raw, _ = R.deconvolve_f64(rec, sweep, reg, normalise_peak=False, remove_dc=False, mode=mode)
        _close(raw, O.deconvolve(rec, sweep, regularization_relative=reg, normalise_peak=False, remove_dc=False,
                                 output_length_mode=mode), f"file {i} raw {mode} {reg}")


def test_batch_is_what_the_gpu_test_needs():
    files = R.e2e_files()
    n_fft = [R.next_power_of_two(max(rec.shape[0], sw.size)) for rec, sw in files]
    assert n_fft == [8, 64, 1024, 1024, 8192] and [rec.shape for rec, _ in files] == [(8, 2), (9, 1), (100, 2), (1000, 1), (5000, 1)]
    assert any(sw.size > rec.shape[0] for rec, sw in files) and any(sw.size < rec.shape[0] for rec, sw in files)
    assert all(float(np.max(np.abs(rec))) < 1.0 for rec, _ in files)             # the oracle clips a recording to [-1, 1]


def _dft_ld(x, n_fft, inverse_of=None):
    k = np.arange(n_fft, dtype=LD)
    w = LD(2.0) * np.arccos(LD(-1.0)) * np.outer(k, k) / LD(n_fft)
    c, s = np.cos(w), np.sin(w)
    if inverse_of is None:
        xp = np.zeros(n_fft, LD)
        xp[:len(x)] = np.asarray(x, np.float32).astype(LD)
        return c @ xp, -(s @ xp)                                  # re, im of the forward transform, all n_fft bins
    re, im = inverse_of
    return (c @ re - s @ im) / LD(n_fft)


@pytest.mark.parametrize("reg", (1e-10, 1e-6))
def test_float64_restatement_sits_far_inside_the_tolerance(reg):
    """Direct long-double DFTs at the sizes that allow them (n_fft 8 and 64): the float64 numpy.fft composition is within
    1e-3 of the tolerance of the long-double response, so it can stand for the true value at the larger sizes too (its
    error grows like log n_fft)."""
    done = 0
    for rec, sweep in R.e2e_files():
        n_fft = R.next_power_of_two(max(rec.shape[0], sweep.size))
        if n_fft > 128:
            continue
        xr, xi = _dft_ld(sweep, n_fft)
        _, raw = R.deconvolve_f64(rec, sweep, reg, mode="full_fft")
        for c in range(rec.shape[1]):
            yr, yi = _dft_ld(rec[:, c], n_fft)
            p = xr * xr + xi * xi
            den = p + LD(reg) * max(LD(1e-30), np.max(p))
            h = _dft_ld(None, n_fft, inverse_of=((yr * xr + yi * xi) / den, (yi * xr - yr * xi) / den))
            _close(raw[c], h.astype(np.float64), f"n_fft {n_fft} channel {c}", factor=1e-3)
            done += 1
    assert done == 3


# -------------------------------------------------------------------------------------------------------------- divide
def _div_model(Y, X, reg, pmax=None, conj_y=False):
    """The reference's float64 lines, with the mistakes a kernel could make as options.  (H, max p)."""
    with np.errstate(all="ignore"):
        p = np.abs(X) ** 2
        own = float(np.max(p))
        eps = reg * max(1e-30, own if pmax is None else pmax)
        P = np.conj(Y) * X if conj_y else Y * np.conj(X)
        return P.real / (p + eps) + 1j * (P.imag / (p + eps)), own


def _div_rejections(neighbour=False, conj_y=False):
    Ys, Xs, _ = R.divide_case()
    hits = 0
    for reg in R.DIV_REG:
        pm = [_div_model(Y, X, reg)[1] for Y, X in zip(Ys, Xs)]
        for e, (Y, X) in enumerate(zip(Ys, Xs)):
            got, own = _div_model(Y, X, reg, pmax=pm[(e + 1) % len(pm)] if neighbour else None, conj_y=conj_y)
            ref, pref = R.divide(Y, X, 2 * (len(X) - 1), reg)
            try:
                R.check_pmax(own, pref, f"entry {e}")
                R.check_divide(got, ref, f"entry {e} reg {reg}")
            except AssertionError:
                hits += 1
    return hits


def test_divide_table_accepts_the_right_kernel():
    assert _div_rejections() == 0


def test_divide_table_rejects_eps_from_the_neighbouring_entry():
    assert _div_rejections(neighbour=True) > 0


def test_divide_table_rejects_conj_on_the_wrong_factor():
    assert _div_rejections(conj_y=True) > 0


def test_divide_table_holds_what_it_says():
    Ys, Xs, share = R.divide_case()
    assert [2 * (len(X) - 1) for X in Xs] == [e[0] for e in R.DIV_ENTRIES] and Xs[4] is Xs[share[4]]
    assert int(np.argmax(np.abs(Xs[1]))) == 0 and int(np.argmax(np.abs(Xs[2]))) == 256
    assert int(np.argmax(np.abs(Xs[3]))) == 2048 and int(np.argmax(np.abs(Xs[5]))) == 2047
    H0, p0 = R.divide(Ys[6], Xs[6], 512, 0.0)
    H1, p1 = R.divide(Ys[6], Xs[6], 512, 1e-10)
    assert p0 == 0 and np.isnan(H0.real).all() and np.all(H1 == 0)
    H, p = R.divide(Ys[9], Xs[9], 8, 1e-6)
    assert np.isposinf(p) and np.all(H == 0) and np.isnan(R.divide(Ys[9], Xs[9], 8, 0.0)[0].real).all()
    H, p = R.divide(Ys[7], Xs[7], 8, 0.0)
    assert 0 < float(p) < 2.3e-308 and np.isfinite(H.real.astype(np.float64)).all()


# -------------------------------------------------------------------------------------------------------------- finish
def _fin_rejections(mutant):
    slots, n_out, group = R.finish_case()
    hits = 0
    for dc in (False, True):
        for norm in (False, True):
            for target in R.FIN_TARGET:
                ref, _ = R.finish(slots, n_out, group, dc, norm, target)
                got = mutant(slots, n_out, group, dc, norm, target)
                try:
                    for e in range(len(slots)):
                        R.check_finish(got[e], ref[e], n_out[e], f"entry {e}")
                except AssertionError:
                    hits += 1
    return hits


def _mean_over_the_slot(slots, n_out, group, dc, norm, target):
    return R.finish(slots, n_out, group, dc, norm, target, mean=[R.mean32(s, s.size) for s in slots])[0]


def _peak_per_channel(slots, n_out, group, dc, norm, target):
    return R.finish(slots, n_out, range(len(slots)), dc, norm, target)[0]


def _tail_overwritten(slots, n_out, group, dc, norm, target):
    means = [R.mean32(s, n) for s, n in zip(slots, n_out)]
    return R.finish(slots, [s.size for s in slots], group, dc, norm, target, mean=means)[0]


def test_finish_table_accepts_the_right_kernel():
    assert _fin_rejections(lambda *a: R.finish(*a)[0]) == 0


@pytest.mark.parametrize("mutant", [_mean_over_the_slot, _peak_per_channel, _tail_overwritten])
def test_finish_table_rejects(mutant):
    assert _fin_rejections(mutant) > 0


def test_finish_table_holds_what_it_says():
    slots, n_out, group = R.finish_case()
    assert [s.size - n for s, n in zip(slots, n_out)] == [5 + e for e in range(8)]
    peaks = [float(np.max(np.abs(s[:n]))) for s, n in zip(slots, n_out)]
    assert peaks[3] > max(peaks[0], peaks[5]) and peaks[2] == 0.0
    out, means = R.finish(slots, n_out, group, True, True, 0.95)
    assert not out[2][:n_out[2]].any() and means[2] == 0
    for g in (0, 2, 3):
        assert abs(max(float(np.max(np.abs(out[e][:n_out[e]]))) for e in range(8) if group[e] == g) - 0.95) < 1e-6
    for e in range(8):
        R.check_mean(means[e], slots[e], n_out[e])


@pytest.mark.parametrize("bad,dc,all_nan", [(np.nan, False, True), (np.nan, True, True), (np.inf, True, True),
                                            (np.inf, False, False)])
def test_a_non_finite_channel_poisons_its_file(bad, dc, all_nan):
    """A NaN sample makes the file's peak NaN and every sample of the file NaN.  An inf does the same when the DC is
    removed (mean inf, inf - inf = NaN); without that the peak is inf, the scale 0, and the file is zeros and one NaN, as
    NumPy gives for the reference's lines."""
    slots, n_out, group = R.finish_nonfinite_case(bad)
    out, _ = R.finish(slots, n_out, group, dc, True, 0.95)
    for e in range(4):
        if all_nan:
            assert np.isnan(out[e][:n_out[e]]).all()
        else:
            assert np.isnan(out[e][:n_out[e]]).sum() == (1 if e in (1, 2) else 0) and not np.nan_to_num(out[e][:n_out[e]]).any()
    assert np.isfinite(out[4][:n_out[4]]).all() and abs(float(np.max(np.abs(out[4][:n_out[4]]))) - 0.95) < 1e-6
    # the reference's own lines on the same file (its _peak_normalise leaves a file alone only for peak <= 0)
    ir = np.stack([out_e[:700] for out_e in R.finish(slots[:2], n_out[:2], group[:2], dc, False, 0.95)[0]], axis=1)
    with np.errstate(all="ignore"):
        peak = float(np.max(np.abs(ir)))
        want = ir if peak <= 0.0 else (ir * (0.95 / peak)).astype(np.float32)
    assert np.array_equal(want, np.stack([out[0][:700], out[1][:700]], axis=1), equal_nan=True)


def test_the_oracle_scales_a_file_with_a_nan_by_nan():
    rec, sweep = R.e2e_files()[2]
    rec = rec.copy()
    rec[40, 1] = np.nan
    with np.errstate(all="ignore"):
        assert np.isnan(O.deconvolve(rec, sweep)).all()
        raw = O.deconvolve(rec, sweep, normalise_peak=False)
    assert np.isnan(raw[:, 1]).all() and np.isfinite(raw[:, 0]).all()
