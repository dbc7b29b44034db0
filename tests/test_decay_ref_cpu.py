"""tests/decay_ref.py (the reference and the comparison functions of test_gpu_decay_dispatch.py) pinned without a GPU.

Measured here, on the end-to-end input set (decay_ref.end_to_end_inputs: ten decays of 4097 .. 8 384 512 samples, RT60
0.03 .. 40 s, ranges (0,-10), (-5,-25), (-5,-35), (-5,-65)): numpy.linalg.lstsq differs from the long-double closed-form
line by at most 2.3e-15 relative in the slope, 2.6e-14 in the intercept and 1.2e-16 in r2 -- far inside comparison B's
1e-9 / 1e-10, so lstsq (the oracle's own fit) is the reference for every case, the 8.38 M-sample segment included.  The
float32 curves of the oracle's float64 path and of the long-double path are bit-identical on all 12 585 114 samples of
that set, and so are their records.  (A 2.88 M-sample decay with RT60 200 s was replaced: 1 to 3 of its float32 samples
differed between the two accumulations.)
"""
import numpy as np
import pytest

import decay_ref as R
from oracle import ira_oracle as O

SR = 48000


@pytest.fixture(autouse=True)
def _longdouble():
    R.need_longdouble()


@pytest.mark.parametrize("tag", ["xa", "xb", "xb16", "xc", "xa_smooth"])
def test_reference_reproduces_the_goldens(golden, tag):
    g, c, _ = golden
    case = c[f"{tag}/decay"]
    x = g[f"in/{tag.split('_')[0]}"]
    seg = x[case["start"]:]
    assert case["start"] == int(np.argmax(np.abs(x)))
    _, db = R.edc_curve(seg, 1e-20, -120.0, window=case["kw"].get("edc_smoothing_window_samples", 0))
    np.testing.assert_allclose(db, g[f"{tag}/decay/edc_db"], rtol=3e-7, atol=1e-6)
    names = {"EDT": (0.0, -10.0), "T20": (-5.0, -25.0), "T30": (-5.0, -35.0)}
    order = [k for k in names if k != "EDT" or case["kw"].get("compute_edt")]
    rec, cr = R.curve_records(db, [names[k] for k in order], R.PRODUCT_CROSS, 8, t_div=SR)
    assert {k for k, r in zip(order, rec) if r[0] == 1.0} == set(case["fits"])
    for k, r in zip(order, rec):
        gold = case["fits"].get(k)
        if gold is None:
            continue
        assert abs(r[6] / gold[7] - 1) < 1e-6 and abs(r[3] / gold[4] - 1) < 1e-6 and abs(r[5] - gold[6]) < 1e-9
        assert abs(r[1] - gold[2]) < 1e-7 and abs(r[2] - gold[3]) < 1e-7
    if case["early"] is not None:
        assert abs((cr[1] - cr[0]) / case["early"] - 1) < 1e-6


@pytest.mark.parametrize("n", [4, 5, 300])
def test_box_smoothing_is_numpy_convolve_same(n):
    rng = np.random.default_rng(n)
    a = -np.cumsum(rng.random(n)) * 0.7
    for w in (1, 2, 3, 8, 255, n):
        if w > n:
            continue
        ref = np.convolve(a, np.ones(w, dtype=np.float64) / float(w), mode="same")
        got = R.box_smooth(a, w).astype(np.float64)
        assert ref.shape == got.shape and np.max(np.abs(got - ref)) <= 1e-12, (n, w)


def test_reference_agrees_with_itself_on_the_end_to_end_inputs():
    """The oracle's float64 path and the long-double curve: every float32 sample, npts, valid and the times equal, rt60
    to 1e-12; and numpy.linalg.lstsq within 1e-10 of the long-double line (see the module docstring for the figures)."""
    worst = dict(slope=0.0, icpt=0.0, r2=0.0)
    total = 0
    for name, x in R.end_to_end_inputs():
        _, d32 = R.edc_curve(x, 1e-20, -120.0)
        _, db, _ = O.schroeder_edc_db(x, SR, trim_to_peak=False)
        assert np.array_equal(db.view(np.uint32), d32.view(np.uint32)), name
        total += x.size
        a, ca = R.end_to_end_records(x, R.FOUR_RANGES, R.PRODUCT_CROSS, 8)
        b, cb = R.curve_records(d32, R.FOUR_RANGES, R.PRODUCT_CROSS, 8)
        assert np.all(a[:, 0] == 1.0), name
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(ca, cb)
        ld, _ = R.curve_records(d32, R.FOUR_RANGES, (), 8, line="ld")
        worst["slope"] = max(worst["slope"], float(np.max(np.abs(ld[:, 3] / b[:, 3] - 1))))
        worst["icpt"] = max(worst["icpt"], float(np.max(np.abs(ld[:, 4] - b[:, 4]) / np.maximum(1.0, np.abs(b[:, 4])))))
        worst["r2"] = max(worst["r2"], float(np.max(np.abs(ld[:, 5] - b[:, 5]))))
    print(f"lstsq against the long-double line on {total} samples: {worst}")
    assert worst["slope"] < 1e-10 and worst["icpt"] < 1e-10 and worst["r2"] < 1e-10, worst


def test_records_keep_what_the_kernel_documents():
    t = R.time_axis(100)
    y = (-np.arange(100, dtype=np.float32)).astype(np.float32)
    r = R.fit_record(t, y, -5.0, -25.0, 8)
    assert r[0] == 1.0 and r[7] == 21 and abs(r[3] + SR) < 1e-6 * SR
    r = R.fit_record(t, y, -5.0, -25.0, 22)                    # too few points: times and npts kept
    assert r[0] == 0.0 and r[7] == 21 and not np.isnan(r[1]) and np.all(np.isnan(r[3:7]))
    r = R.fit_record(t, y, -5.0, -200.0, 8)                    # lower level never reached
    assert r[0] == 0.0 and np.isnan(r[2]) and np.isnan(r[7]) and not np.isnan(r[1])
    flat = np.concatenate([np.full(50, -3.0), [-12.0, -30.0]]).astype(np.float32)
    r = R.fit_record(R.time_axis(52), flat, -1.0, -10.0, 8)     # a mask of equal values: slope exactly 0, refused
    assert list(r[[0, 3, 4, 5, 6, 7]]) == [0.0, 0.0, -3.0, 0.0, -np.inf, 50.0] and r[1] == 0.0
    yr, ok = R.rel_to_peak(y + np.float32(3.0), -120.0, 100.0)
    assert ok and yr[0] == 0.0
    assert not R.rel_to_peak(y - np.float32(30.0), -120.0, 100.0)[1]
    y2 = y.copy(); y2[50] = np.inf
    assert not R.rel_to_peak(y2, -120.0, 0.0)[1]


# ------------------------------------------------------------------------------------------------- negative controls
def _ir():
    return R.ir(5, 20000, 1.0)                                  # ends at about -25 dB: the floor hides nothing


def test_negative_control_sum_without_the_last_sample():
    x = _ir()
    e = x.astype(np.float64) ** 2
    edc = np.cumsum(e[::-1])[::-1] - e[-1]                      # the last sample left out of every suffix sum
    edc = np.maximum(edc, 1e-20)
    db = 10.0 * np.log10(edc / edc[0])
    with pytest.raises(AssertionError):
        R.compare_edc(x, 1e-20, -120.0, got64=db)
    with pytest.raises(AssertionError):
        R.compare_edc(x, 1e-20, -120.0, got32=np.maximum(db, -120.0).astype(np.float32))


def test_negative_control_normaliser_one_sample_late():
    x = _ir()
    e = x.astype(np.float64) ** 2
    edc = np.maximum(np.cumsum(e[::-1])[::-1], 1e-20)
    good = 10.0 * np.log10(edc / edc[0])
    R.compare_edc(x, 1e-20, -120.0, got64=good, got32=np.maximum(good, -120.0).astype(np.float32))   # the plain float64 path passes
    db = 10.0 * np.log10(edc / edc[1])
    with pytest.raises(AssertionError):
        R.compare_edc(x, 1e-20, -120.0, got64=db)
    with pytest.raises(AssertionError):
        R.compare_edc(x, 1e-20, -120.0, got32=np.maximum(db, -120.0).astype(np.float32))


def test_negative_control_crossing_index_one_too_high():
    x = _ir()
    _, y = R.edc_curve(x, 1e-20, -120.0)
    t = R.time_axis(y.size)
    ref, cref = R.curve_records(y, R.PRODUCT_RANGES, (-10.0,), 8)
    i = int(np.argmax(y <= np.float32(-10.0))) + 1              # one too high
    t0, t1, y0, y1 = float(t[i - 1]), float(t[i]), float(y[i - 1]), float(y[i])
    wrong = t0 + float(np.clip((-10.0 - y0) / (y1 - y0), 0.0, 1.0)) * (t1 - t0)
    R.compare_times(cref, cref)
    with pytest.raises(AssertionError):
        R.compare_times([wrong], cref)
    bad = ref.copy(); bad[0, 2] = wrong
    with pytest.raises(AssertionError):
        R.compare_records(bad, ref)
    with pytest.raises(AssertionError):
        R.compare_end_to_end(bad, ref)


def test_negative_control_open_mask():
    x = _ir()
    _, y = R.edc_curve(x, 1e-20, -120.0)
    t = R.time_axis(y.size)
    ref = R.fit_record(t, y, 0.0, -10.0, 8)                     # starts at t[0] exactly: t > ts loses that sample
    assert ref[0] == 1.0 and ref[1] == 0.0
    m = (t > ref[1]) & (t <= ref[2])
    assert int(m.sum()) == ref[7] - 1
    tt, yy = t[m].astype(np.float64), y[m].astype(np.float64)
    slope, icpt, r2 = R.ld_line(tt, yy)
    bad = np.array([1.0, ref[1], ref[2], slope, icpt, r2, -60.0 / slope, m.sum()])
    R.compare_records(ref, ref)
    with pytest.raises(AssertionError):
        R.compare_records(bad, ref)
    bad[7] = ref[7]                                            # even with the count patched the line gives it away
    with pytest.raises(AssertionError):
        R.compare_records(bad, ref)


def test_negative_control_last_of_two_tied_maxima():
    x = np.zeros(40000, np.float32)
    x[[16383, 16384]] = [-0.5, 0.5]
    R.compare_peak(x, 16383, 0.5)
    with pytest.raises(AssertionError):
        R.compare_peak(x, 16384, 0.5)
    x[[100, 200]] = np.array([0x7fc00001, 0x7fffffff], np.uint32).view(np.float32)    # two NaNs: the first wins
    R.compare_peak(x, 100, np.float32(np.nan))
    with pytest.raises(AssertionError):
        R.compare_peak(x, 200, np.float32(np.nan))
