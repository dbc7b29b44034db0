"""GPU: the fused half-length forward transform (ira_rfft_smooth, mirror-pair tiles of ira_fftsmooth.hip) at every tile shape
its second pass has: quad tiles {p, p + 1, n1 - p - 1, n1 - p} only (an even number of mirror pairs), quad tiles and a last
two-row tile (an odd number), the split-pass fall-back of an odd n1, the smallest half length, and a length whose rotation
W_2n^k takes a step (n2 > 128).  Each element against the long-double restatement tests/longfft_ref.py under the bounds of
test_gpu_longfft_edges.py (2-norm and every bin, Im X[0] = Im X[L/2] = 0 exactly); the C entry point itself on guarded
spectrum and work buffers; one file through rt60_bands_device against the curve path."""
import numpy as np
import pytest

import guard_buffers as G
import longfft_ref as R
from test_gpu_longfft_edges import Elements, _eng, check_element, reference, run_forward

pytestmark = pytest.mark.gpu

# L: (n1, n2) of the half-length transform, mirror pairs n1/2 - 1, quad tiles, two-row tiles behind them
CASES = {
    128: ((8, 8), 3, 1, 1),              # the smallest half length the direct transform accepts
    200: ((10, 10), 4, 2, 0),            # an even number of pairs: quads only
    2400: ((30, 40), 14, 7, 0),
    4800: ((48, 50), 23, 11, 1),         # an odd number: a single pair is left over
    96000: ((200, 240), 99, 49, 1),      # n2 > 128: every lane's rotation takes a step
    450: ((15, 15), None, None, None),   # n1 odd: no row n1/2, the separate split pass
}


def _inputs(L):
    return R.make_inputs(L, n2=R.smooth_split_py(L)[1] if R.is_direct(L) else None, run=2 * R.smooth_split_py(L // 2)[1],
                         families=("impulse", "noise"))


def test_the_lengths_reach_every_tile_shape():
    """What the planner and the split do with the lengths above (no GPU work: the cases are what the module claims)."""
    eng = _eng()
    for L, (split, pairs, quads, left) in CASES.items():
        assert R.smooth_split_py(L // 2) == split == tuple(eng.smooth_split(L // 2)), L
        n1 = split[0]
        if pairs is None:
            assert n1 % 2 == 1 and R.predict_path(L) == ("smooth", "half_split", L // 2)
            continue
        assert R.predict_path(L) == ("smooth", "half_fused", L // 2)
        assert (n1 // 2 - 1, (n1 // 2 - 1) // 2, (n1 // 2 - 1) % 2) == (pairs, quads, left), L
    assert min(L // 2 for L in CASES) == 64 and R.smooth_split_py(63) is None and R.smooth_split_py(62) is None


@pytest.mark.parametrize("hann", [False, True])
@pytest.mark.parametrize("L", sorted(CASES))
def test_half_length_forward_against_the_restatement(L, hann):
    """Impulses (closed forms; at the ends, the middle and the column edges) and noise, all in one call at sample offsets of
    every parity, bin by bin."""
    eng = _eng()
    names, x = _inputs(L)
    el = Elements()
    el.add(names, x, L)
    got = run_forward(eng, el, hann)
    assert len(got) >= 2
    re, im, vn, xn = reference("pair tiles", list(x), L, L, L, hann)
    for j, nm in enumerate(names):
        path = check_element(got[j], re[j], im[j], vn[j], xn[j], L, hann, L, L, "pair tiles", nm, planned=el.planned[j])
        assert path[1] == ("half_split" if CASES[L][1] is None else "half_fused")
        assert got[j][0].imag == 0.0 and got[j][-1].imag == 0.0


@pytest.mark.parametrize("L", [128, 200, 4800, 96000])
def test_entry_point_writes_nothing_outside_spectrum_and_work(L):
    """ira_rfft_smooth (interleave, no split scratch) on buffers of its own: two signals at an even and an odd sample offset,
    spectra at offsets of both parities with gaps between them, the work array of 2 n complex values between guards.  Every
    guard word comes back untouched, every bin and every work element was written, and the spectra are the bytes rfft_any
    gives for the same samples."""
    eng = _eng()
    t = eng.torch
    n = L // 2
    rng = np.random.default_rng(L)
    rows = [(rng.standard_normal(L) * np.exp(-np.arange(L) / (0.3 * L))).astype(np.float32) for _ in range(2)]
    fx = G.Flat([L, L], np.float32, phase=2)
    assert fx.off[0] % 2 != fx.off[1] % 2
    x = G.to_device(eng, fx.filled(rows))
    fs = G.Flat([n + 1, n + 1], np.complex128, phase=1)
    assert fs.off[0] % 2 != fs.off[1] % 2
    spec = G.to_device(eng, fs.filled())
    fw = G.Flat([2 * n], np.complex128)
    work = G.to_device(eng, fw.filled())
    xo = t.from_numpy(np.array(fx.off, np.int64)).to(eng.device)
    so = t.from_numpy(np.array(fs.off, np.int64)).to(eng.device)
    t1, t2, tf = eng.smooth_tables(n)
    from audio_analysis_amd._lib import ptr as p
    for hann in (0, 1):
        rc = eng.lib.ira_rfft_smooth(p(x), p(xo), n, 2, hann, p(t1), p(t2), p(tf), p(work) + 16 * fw.off[0], p(spec), p(so),
                                     None, None, None, None, None, None, None, None, 1, eng.stream)
        assert rc == 0, rc
        got = fs.split(spec.cpu().numpy().view(np.complex128), f"spectrum L={L}")
        wk = fw.split(work.cpu().numpy().view(np.complex128), f"work array L={L}")[0]
        ref, ro = eng.rfft_any(x, np.array(fx.off, np.int64), np.array([L, L], np.int32), bool(hann))
        h = ref.cpu().numpy().view(np.complex128)
        for e in range(2):
            assert got[e].tobytes() == h[ro[e] : ro[e] + n + 1].tobytes(), (L, hann, e)
            assert got[e][0].imag == 0.0 and got[e][-1].imag == 0.0
        sent = np.uint64(G.SENT64)
        assert not np.any(np.all(G.words(wk).reshape(-1, 2) == sent, axis=1)), "a work element was never written"
        fx.split(x.cpu().numpy(), f"input L={L}")
        spec.copy_(G.to_device(eng, fs.filled()))
        work.copy_(G.to_device(eng, fw.filled()))


def test_band_t30_through_the_bank_equals_the_curve_path():
    """rt60_bands_device on two short files (4800 and 9600 samples: quad tiles and an odd pair in the forward transform):
    every band's T30, T20 and EDT as the fused fits give them equal what ira_edc_db + ira_curve_fits give on the same band
    signals -- the same fits found, the values to 1e-9 relative."""
    from audio_analysis_amd.analyse import rt60bands as rb
    from audio_analysis_amd.synth import synth_ir
    eng = _eng()
    SR = 48000
    st = rb.Rt60BandsAnalysisSettings(band_mode="octave", include_t20=True, include_edt=True)
    dec = st.decay_settings
    chans = [synth_ir(60, 0, 4800, rt60_seconds=0.03), synth_ir(61, 0, 9600, rt60_seconds=0.05)]
    b = eng.upload(chans)
    bands, vals, have = rb.rt60_bands_device(eng, b, SR, st)
    nb = len(bands)
    assert nb >= 2 and have.all()
    _, y, y_off = rb.band_signals_device(eng, b, SR, st)
    start = eng.peaks(b).astype(np.int64) if dec.trim_to_peak else np.zeros(b.count, np.int64)
    if dec.ignore_leading_seconds > 0.0:
        start = start + int(round(dec.ignore_leading_seconds * SR))
    start = np.minimum(b.length.astype(np.int64), start)
    seg_c = np.repeat(np.arange(b.count), nb)
    seg_b = np.tile(np.arange(nb), b.count)
    seg_off = (y_off[seg_c, seg_b] + start[seg_c]).astype(np.int64)
    seg_len = (b.length.astype(np.int64) - start)[seg_c]
    ranges = [(float(r[0]), max(float(r[1]), float(dec.fit_lower_limit_db)))
              for r in (dec.t30_range_db, dec.t20_range_db, dec.edt_range_db)]
    edc, e_off = eng.edc_db(y, seg_off, seg_len, dec.edc_epsilon, dec.edc_floor_db)
    fit, _ = eng.curve_fits(edc, e_off, seg_len, 1.0, float(SR), ranges, 8)
    fit = fit.cpu().numpy()
    found = 0
    for s, (c, k) in enumerate(zip(seg_c, seg_b)):
        for j in range(3):
            ok = fit[s, j, 0] == 1.0
            assert ok == (not np.isnan(vals[c, k, j])), (c, bands[k].name, j, fit[s, j], vals[c, k])
            if ok:
                found += j == 0
                assert abs(vals[c, k, j] - fit[s, j, 6]) <= 1e-9 * abs(fit[s, j, 6]), (c, bands[k].name, j)
    assert found >= 2                                           # T30 itself was found and compared
