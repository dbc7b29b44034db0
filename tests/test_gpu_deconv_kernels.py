"""ira_deconv_divide and ira_deconv_finish (ira_deconv.hip) called through the C-ABI, on buffers this file owns (their
scratch arrays included), against the restatements of tests/deconv_ref.py (whose case tables tests/test_deconv_ref_cpu.py
shows to reject the subtly wrong kernels).

Every buffer a launch writes is a guarded flat buffer (tests/guard_buffers.py); every guard and gap must come back
untouched, and so must the tail of each response past n_out.  Every
entry of a ragged divide launch, and every file of a finish launch, is also launched alone, in buffers of its own, and
must give the same bytes.

ira_deconv_divide: max |X|^2 within 2 float64 ulp, H within 8 * 2^-53 |H| normwise of the long-double restatement, NaN
and inf patterns equal.  ira_deconv_finish: the float32 mean within ulp32 / 2 + n 2^-53 mean|h| of the long-double mean,
and, given that mean, the restatement's bits.  test_zz_report prints the largest multiple of 2^-53 seen.  Measured on an MI355X: |dH| <= 5.08 * 2^-53 |H| (8 allowed);
every mean inside its bound, every finish output bit-equal to the restatement.

What these tests found (fixed with them): the file peak was taken with fmaxf, which drops a NaN, and a non-positive OR
NaN peak left the file unscaled -- so the finite channel of a stereo file whose other channel holds a NaN (or, with the
DC removed, an inf) came back scaled by its own peak, where the reference's numpy.max makes every sample of the file NaN.
"""
import numpy as np
import pytest

import deconv_ref as R
from guard_buffers import Flat, sentinel as _sentinel, to_device as _dev, untouched, words as _words

pytestmark = pytest.mark.gpu
IRA_OK, IRA_E_SIZE = 0, -2
STATS = {}


@pytest.fixture(scope="module")
def eng():
    R.need_longdouble()
    from audio_analysis_amd.engine import get_engine
    return get_engine()


# -------------------------------------------------------------------------------------------------------------- divide
def divide(eng, Ys, Xs, share, reg, phase=0, max_nfft=None):
    """One launch: (H per entry complex128, max |X|^2 per entry).  Entry e reads the X of entry share[e] where that is set."""
    nb = len(Ys)
    n_fft = np.array([2 * (len(y) - 1) for y in Ys], np.int32)
    own = [e for e in range(nb) if share[e] is None]
    ly, lx, lp = Flat([len(y) for y in Ys], np.complex128, phase), Flat([len(Xs[e]) for e in own], np.complex128, phase + 4), \
        Flat([nb], np.float64)
    xoff = {e: lx.off[i] for i, e in enumerate(own)}
    xoffs = np.array([xoff[e if share[e] is None else share[e]] for e in range(nb)], np.int64)
    x_host = lx.filled([Xs[e] for e in own])
    y, x, pmax = _dev(eng, ly.filled(Ys)), _dev(eng, x_host), _dev(eng, lp.filled())
    yoff, xo, nf = _dev(eng, np.array(ly.off, np.int64)), _dev(eng, xoffs), _dev(eng, n_fft)
    rc = eng.lib.ira_deconv_divide(y.data_ptr(), yoff.data_ptr(), x.data_ptr(), xo.data_ptr(), nf.data_ptr(), nb,
                                   int(n_fft.max()) if max_nfft is None else max_nfft, float(reg),
                                   pmax.data_ptr() + 8 * lp.off[0], eng.stream)
    assert rc == IRA_OK
    H = ly.split(y.cpu().numpy(), "ira_deconv_divide H")
    pm = lp.split(pmax.cpu().numpy(), "ira_deconv_divide pmax")[0]
    assert np.array_equal(_words(x.cpu().numpy()), _words(x_host)), "ira_deconv_divide wrote to X"
    return H, pm


@pytest.mark.parametrize("reg", R.DIV_REG)
def test_deconv_divide_against_long_double(eng, reg):
    Ys, Xs, share = R.divide_case()
    H, pm = divide(eng, Ys, Xs, share, reg)
    for e, (Y, X) in enumerate(zip(Ys, Xs)):
        what = f"reg {reg} entry {e} ({R.DIV_ENTRIES[e][1]}, n_fft {R.DIV_ENTRIES[e][0]})"
        ref, pref = R.divide(Y, X, R.DIV_ENTRIES[e][0], reg)
        R.check_pmax(pm[e], pref, what)
        STATS["divide"] = max(STATS.get("divide", 0.0), R.check_divide(H[e], ref, what))
        Ha, pa = divide(eng, [Y], [X], [None], reg, phase=e + 1)
        assert np.array_equal(_words(Ha[0]), _words(H[e])) and _words(pa)[0] == _words(pm[e:e + 1])[0], \
            f"{what}: alone and in the batch differ"


def test_deconv_divide_refusals(eng):
    Ys, Xs, _ = R.divide_case()
    ly, lp = Flat([len(Ys[1])], np.complex128), Flat([1], np.float64)
    y, x, pmax = _dev(eng, ly.filled([Ys[1]])), _dev(eng, Xs[1]), _dev(eng, lp.filled())
    yoff, xoff, nf = _dev(eng, np.array(ly.off, np.int64)), _dev(eng, np.zeros(1, np.int64)), _dev(eng, np.array([8], np.int32))

    def call(nb, max_nfft):
        return eng.lib.ira_deconv_divide(y.data_ptr(), yoff.data_ptr(), x.data_ptr(), xoff.data_ptr(), nf.data_ptr(), nb,
                                         max_nfft, 1e-10, pmax.data_ptr() + 8 * lp.off[0], eng.stream)

    assert call(0, 8) == IRA_OK and call(-1, 8) == IRA_E_SIZE and call(1, 1) == IRA_E_SIZE
    assert np.array_equal(_words(y.cpu().numpy()), _words(ly.filled([Ys[1]])))
    assert untouched(pmax.cpu().numpy())


# -------------------------------------------------------------------------------------------------------------- finish
def finish(eng, slots, n_out, group, remove_dc, normalise_peak, target, phase=0):
    """One launch: (the slots as they came back, the device's means)."""
    nb, ngroups = len(slots), max(group) + 1
    lh, lm, lp = Flat([s.size for s in slots], np.float32, phase), Flat([nb], np.float32), Flat([ngroups], np.uint32)
    h, mean, peak = _dev(eng, lh.filled(slots)), _dev(eng, lm.filled()), _dev(eng, lp.filled())
    hoff, no, gr = _dev(eng, np.array(lh.off, np.int64)), _dev(eng, np.array(n_out, np.int32)), _dev(eng, np.array(group, np.int32))
    rc = eng.lib.ira_deconv_finish(h.data_ptr(), hoff.data_ptr(), no.data_ptr(), gr.data_ptr(), nb, ngroups, int(max(n_out)),
                                   int(remove_dc), int(normalise_peak), float(target), mean.data_ptr() + 4 * lm.off[0],
                                   peak.data_ptr() + 4 * lp.off[0], eng.stream)
    assert rc == IRA_OK
    back = lh.split(h.cpu().numpy(), "ira_deconv_finish h")
    means = lm.split(mean.cpu().numpy(), "ira_deconv_finish mean")[0]
    lp.split(peak.cpu().numpy().view(np.uint32), "ira_deconv_finish peak")
    return back, means


def _files_alone(eng, slots, n_out, group, back, means, dc, norm, target, what):
    for g in sorted(set(group)):
        mem = [e for e in range(len(slots)) if group[e] == g]
        b, m = finish(eng, [slots[e] for e in mem], [n_out[e] for e in mem], [0] * len(mem), dc, norm, target, phase=g + 1)
        for i, e in enumerate(mem):
            assert np.array_equal(_words(b[i]), _words(back[e])), f"{what}: file {g} alone and in the batch differ (entry {e})"
            assert not dc or _words(m[i:i + 1])[0] == _words(means[e:e + 1])[0], f"{what}: mean of entry {e}"


@pytest.mark.parametrize("normalise_peak", [False, True], ids=["raw_peak", "normalise_peak"])
@pytest.mark.parametrize("remove_dc", [False, True], ids=["keep_dc", "remove_dc"])
def test_deconv_finish_bits(eng, remove_dc, normalise_peak):
    slots, n_out, group = R.finish_case()
    for target in R.FIN_TARGET:
        what = f"remove_dc {remove_dc} normalise_peak {normalise_peak} target {target}"
        back, means = finish(eng, slots, n_out, group, remove_dc, normalise_peak, target)
        if remove_dc:
            for e in range(len(slots)):
                R.check_mean(means[e], slots[e], n_out[e], f"{what} entry {e}")
        ref, _ = R.finish(slots, n_out, group, remove_dc, normalise_peak, target, mean=means if remove_dc else None)
        for e in range(len(slots)):
            R.check_finish(back[e], ref[e], n_out[e], f"{what} entry {e} (n_out {n_out[e]})")
        assert not back[2][:n_out[2]].any(), f"{what}: the all-zero file did not stay all zero"
        if not (remove_dc or normalise_peak):
            assert all(np.array_equal(_words(b), _words(s)) for b, s in zip(back, slots))
        _files_alone(eng, slots, n_out, group, back, means, remove_dc, normalise_peak, target, what)


@pytest.mark.parametrize("bad,remove_dc,all_nan", [(np.nan, False, True), (np.nan, True, True), (np.inf, True, True),
                                                   (np.inf, False, False)],
                         ids=["nan-keep_dc", "nan-remove_dc", "inf-remove_dc", "inf-keep_dc"])
def test_deconv_finish_non_finite_channel_poisons_its_file(eng, bad, remove_dc, all_nan):
    """A NaN sample in one channel makes every sample of both channels of its file NaN (numpy.max keeps it, the scale is
    NaN); an inf does the same once the DC is removed (mean inf, inf - inf = NaN); without that the peak is inf, the
    scale 0, and the file is zeros and one NaN, as NumPy gives for the reference's lines.  The finite file of the launch
    keeps the bytes it has alone."""
    slots, n_out, group = R.finish_nonfinite_case(bad)
    what = f"bad {bad} remove_dc {remove_dc}"
    back, means = finish(eng, slots, n_out, group, remove_dc, True, 0.95)
    if remove_dc:
        for e in range(len(slots)):
            if np.isfinite(slots[e][:n_out[e]]).all():
                R.check_mean(means[e], slots[e], n_out[e], f"{what} entry {e}")
            else:
                assert (np.isnan(means[e]) if np.isnan(bad) else means[e] == bad), (what, e, means[e])
    ref, _ = R.finish(slots, n_out, group, remove_dc, True, 0.95, mean=means if remove_dc else None)
    for e in range(len(slots)):
        R.check_finish(back[e], ref[e], n_out[e], f"{what} entry {e}")
    for e in range(4):
        if all_nan:
            assert np.isnan(back[e][:n_out[e]]).all(), f"{what}: entry {e} of a poisoned file holds a number"
    assert np.isfinite(back[4][:n_out[4]]).all()
    _files_alone(eng, slots, n_out, group, back, means, remove_dc, True, 0.95, what)


def test_deconv_finish_refusals(eng):
    slots, n_out, group = R.finish_case()
    lh = Flat([slots[1].size], np.float32)
    h, sc = _dev(eng, lh.filled([slots[1]])), _dev(eng, _sentinel(4, np.float32))
    hoff, no, gr = _dev(eng, np.array(lh.off, np.int64)), _dev(eng, np.array([63], np.int32)), _dev(eng, np.zeros(1, np.int32))

    def call(nb, ngroups, max_len, dc, norm):
        return eng.lib.ira_deconv_finish(h.data_ptr(), hoff.data_ptr(), no.data_ptr(), gr.data_ptr(), nb, ngroups, max_len,
                                         dc, norm, 0.95, sc.data_ptr(), sc.data_ptr() + 8, eng.stream)

    assert call(0, 1, 63, 1, 1) == IRA_OK and call(1, 1, 63, 0, 0) == IRA_OK
    assert call(-1, 1, 63, 1, 1) == IRA_E_SIZE and call(1, -1, 63, 1, 1) == IRA_E_SIZE and call(1, 1, -1, 1, 1) == IRA_E_SIZE
    assert np.array_equal(_words(h.cpu().numpy()), _words(lh.filled([slots[1]])))
    assert untouched(sc.cpu().numpy())


def test_zz_report():
    for name, worst in sorted(STATS.items()):
        print(f"ira_deconv_{name}: largest |dH| = {worst:.3f} * 2^-53 |H| (8 allowed)")
