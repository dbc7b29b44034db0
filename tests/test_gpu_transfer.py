"""
The dual-channel spectral sums on the device (ira_xspec_accumulate, ira_xspec_finish, audio_analysis_amd.analyse.transfer)
against the float64 NumPy restatement of tests/transfer_ref.py.

Sums are held to transfer_ref.tolerance, a bound derived from the normwise error g * nf of one packed float64 transform
(g = 16 log2(n_fft) 2^-53, nf the JOINT norm of the two windowed channels of a frame) and the roundings of the K-term
sums; derived values to that bound propagated (h1_bound, coherence_bound); the finish stage, on its own, to a few ulp of
the restatement applied to the device's own sums.  Every test prints the largest observed error beside its bound.
"""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import transfer_ref as R

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
SR = 48000
C = R.FRAMES_PER_CHUNK
DELAYS = (0, 5, -7)
FIR = (0.6, 0.3)


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def run(eng, rows, pairs, n_fft, hop, window):
    """Engine level: rows -> one device buffer; pairs = [(x row, y row, delay)] -> one accumulate and one finish launch.
    Returns the device's (npairs, 11, nbins) float64."""
    b = eng.upload([np.asarray(r, dtype=np.float32) for r in rows])
    xo, yo, n = [], [], []
    for xi, yi, d in pairs:
        xs, ys, nn = R.geometry(int(b.length[xi]), int(b.length[yi]), d)
        xo.append(int(b.off[xi]) + xs)
        yo.append(int(b.off[yi]) + ys)
        n.append(nn)
    out = eng.cross_spectra(b.x, np.array(xo, np.int64), np.array(yo, np.int64), np.array(n, np.int64), n_fft, hop,
                            window == "hann")
    return out.cpu().numpy()


def noise_pair(rng, length, gain=1.0):
    """A float32 reference row and a measurement row: the reference through a two-tap filter plus independent noise."""
    x = (gain * rng.standard_normal(length)).astype(np.float32)
    y = (np.convolve(x.astype(np.float64), FIR)[:length] + 0.2 * gain * rng.standard_normal(length)).astype(np.float32)
    return x, y


def sums_errors(dev, ref):
    """(observed error / bound, per sum, the largest over the bins) of one pair; a bin with a zero bound must be exact."""
    bxx, byy, bxy = ref["bounds"]
    exx, eyy = np.abs(dev[0] - ref["sxx"]), np.abs(dev[1] - ref["syy"])
    exy = np.abs((dev[2] + 1j * dev[3]) - ref["sxy"])
    out = []
    for e, b in ((exx, bxx), (eyy, byy), (exy, bxy)):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(b > 0.0, e / b, np.where(e == 0.0, 0.0, np.inf))
        out.append(float(np.max(r)) if r.size else 0.0)
    return out


@pytest.mark.parametrize("n_fft", [256, 512, 1024, 2048, 4096, 8192])
def test_sums_within_the_derived_bound_and_identical_alone(n_fft):
    """K = 1, C, C + 1, 2C + 1 frames (C frames per chunk) x delays 0, +5, -7 as ONE ragged batch per (hop, window), hop =
    n_fft, n_fft / 2 and 37, Hann and rectangular; then every pair alone, in a buffer of its own: the same bytes.  Every
    transform length from 256 to 8192: the three instantiations of the accumulate kernel (up to 2048, 4096 -- the length the
    settings and the command line default to -- and 8192) and every remainder of the transform's radix schedule."""
    eng = _eng()
    rng = np.random.default_rng(n_fft)
    worst = 0.0
    for hop in (n_fft, n_fft // 2, 37):
        rows, pairs, ks = [], [], []
        for k in (1, C, C + 1, 2 * C + 1):
            x, y = noise_pair(rng, n_fft + (k - 1) * hop + 7)           # 7 spare samples: every delay keeps K = k
            rows += [x, y]
            for d in DELAYS:
                pairs.append((len(rows) - 2, len(rows) - 1, d))
                ks.append(k)
        for window in ("hann", "rect"):
            dev = run(eng, rows, pairs, n_fft, hop, window)
            assert dev.shape == (len(pairs), 11, n_fft // 2 + 1)
            for p, (xi, yi, d) in enumerate(pairs):
                ref = R.pair_reference(rows[xi], rows[yi], d, n_fft, hop, window)
                assert ref["K"] == ks[p]
                rxx, ryy, rxy = sums_errors(dev[p], ref)
                worst = max(worst, rxx, ryy, rxy)
                assert max(rxx, ryy, rxy) <= 1.0, (n_fft, hop, window, ks[p], d, rxx, ryy, rxy)
                alone = run(eng, [rows[xi], rows[yi]], [(0, 1, d)], n_fft, hop, window)
                assert alone[0].tobytes() == dev[p].tobytes(), (n_fft, hop, window, ks[p], d)
            print(f"n_fft {n_fft} hop {hop} {window}: {len(pairs)} pairs, largest error / bound so far {worst:.3e} (bound 1)")
    assert worst > 0.0                                                  # the device did not merely echo the reference


@pytest.mark.parametrize("n_fft", [512, 4096])
def test_reads_stay_inside_the_rows(n_fft):
    """Rows of EXACTLY n_fft + (K - 1) hop samples, K = 1 and 17, no spare sample, in a hand-built buffer with 1 to 7 NaN
    samples in front of and behind every row (Engine.upload packs rows back to back, where a read past a row would land in
    finite neighbour data): one sample read outside a row makes a sum NaN.  Between the others a pair of n_fft - 1 samples:
    no frame, zero sums and the NaN pattern of a pair without frames."""
    eng = _eng()
    rng = np.random.default_rng(100 + n_fft)
    worst = 0.0
    for hop in (1, n_fft // 2, n_fft):
        lens = [n_fft, n_fft - 1, n_fft + 16 * hop]
        rows = [r for n in lens for r in noise_pair(rng, n)]
        off, pos = [], 0
        for i, r in enumerate(rows):
            pos += 1 + (3 * i + hop) % 7                                # the gap in front of row i
            off.append(pos)
            pos += r.size
        flat = np.full(pos + 7, np.nan, np.float32)
        for o, r in zip(off, rows):
            flat[o : o + r.size] = r
        assert np.count_nonzero(np.isnan(flat)) == flat.size - sum(r.size for r in rows)
        x_dev = eng.to_dev(flat)
        for window in ("hann", "rect"):
            dev = eng.cross_spectra(x_dev, np.array(off[0::2], np.int64), np.array(off[1::2], np.int64),
                                    np.array(lens, np.int64), n_fft, hop, window == "hann").cpu().numpy()
            for p, k in ((0, 1), (2, 17)):
                ref = R.pair_reference(rows[2 * p], rows[2 * p + 1], 0, n_fft, hop, window)
                assert ref["K"] == k
                assert np.all(np.isfinite(dev[p, :4])), (n_fft, hop, window, k)
                errs = sums_errors(dev[p], ref)
                worst = max(worst, *errs)
                assert max(errs) <= 1.0, (n_fft, hop, window, k, errs)
            assert R.pair_reference(rows[2], rows[3], 0, n_fft, hop, window)["K"] == 0
            assert np.all(dev[1, :4] == 0.0) and np.all(np.isnan(dev[1, 4:10])) and np.all(dev[1, 10] == 0.0)
            assert np.array_equal(np.isnan(R.derived(dev[1, 0], dev[1, 1], dev[1, 2], dev[1, 3])), np.isnan(dev[1]))
    print(f"n_fft {n_fft}: rows between NaN, largest error / bound {worst:.3e} (bound 1)")
    assert worst > 0.0


@pytest.mark.parametrize("window", ["rect", "hann"])
def test_a_channel_silent_in_some_frames_only(window):
    """The measurement is zero for its first 3 hops, then noise: its first two frames are all zeros (their spectrum is taken
    as 0 exactly), the later frames of the SAME chunk are not.  The sums stay within the bound, and Syy is the Syy of the
    pair with the two silent frames cut off the front -- against the reference's, within its bound, not bit for bit: the
    frames fall into the chunks differently."""
    eng = _eng()
    n_fft, hop = 4096, 2048
    rng = np.random.default_rng(12)
    x, y = noise_pair(rng, n_fft + 19 * hop)
    y[: 3 * hop] = 0.0
    assert not np.any(y[: hop + n_fft]) and np.any(y[2 * hop : 2 * hop + n_fft])
    cut_x, cut_y = x[2 * hop :], y[2 * hop :]
    dev = run(eng, [x, y, cut_x, cut_y], [(0, 1, 0), (2, 3, 0)], n_fft, hop, window)
    ref = R.pair_reference(x, y, 0, n_fft, hop, window)
    ref_cut = R.pair_reference(cut_x, cut_y, 0, n_fft, hop, window)
    assert ref["K"] == 20 and ref_cut["K"] == 18 and C == 16
    errs, errs_cut = sums_errors(dev[0], ref), sums_errors(dev[1], ref_cut)
    with np.errstate(divide="ignore", invalid="ignore"):
        r_syy = np.abs(dev[0, 1] - ref_cut["syy"]) / ref_cut["bounds"][1]
    print(f"{window}: error / bound {max(errs):.3e} (whole), {max(errs_cut):.3e} (cut); Syy of the whole against the cut "
          f"pair's reference {float(np.max(r_syy)):.3e} (bound 1)")
    assert max(errs) <= 1.0 and max(errs_cut) <= 1.0
    assert np.all(ref_cut["bounds"][1] > 0.0) and np.all(r_syy <= 1.0)


def test_finish_stage_alone_to_a_few_ulp():
    """The eleven rows against the restatement applied to the DEVICE's own four sums: 4 ulp for the quotients (H1, H2,
    coherence), 8 ulp for log10 and atan2; the NaN pattern of zero denominators included."""
    eng = _eng()
    rng = np.random.default_rng(5)
    n_fft, hop = 1024, 37
    x, y = noise_pair(rng, n_fft + 40 * hop)
    z = np.zeros_like(x)
    tone = np.cos(2.0 * np.pi * 64.0 / n_fft * np.arange(x.size)).astype(np.float32)
    rows = [x, y, z, tone, (1e-6 * x).astype(np.float32)]
    pairs = [(0, 1, 0), (0, 0, 0), (1, 0, 3), (2, 1, 0), (0, 2, 0), (2, 2, 0), (3, 1, 0), (0, 4, 0), (0, 1, x.size - 100)]
    for window in ("hann", "rect"):
        dev = run(eng, rows, pairs, n_fft, hop, window)
        worst_q = worst_t = 0.0
        for p in range(len(pairs)):
            want = R.derived(dev[p, 0], dev[p, 1], dev[p, 2], dev[p, 3])
            assert np.array_equal(np.isnan(want), np.isnan(dev[p])), (window, p)
            assert np.array_equal(dev[p, :4], want[:4])
            q = float(np.max(R.ulps(dev[p, 4:9], want[4:9])))
            t = float(np.max(R.ulps(dev[p, 9:11], want[9:11])))
            worst_q, worst_t = max(worst_q, q), max(worst_t, t)
            assert q <= 4.0 and t <= 8.0, (window, p, q, t)
        # zero reference: H1 and coherence NaN; zero measurement: H2 and coherence NaN, H1 = 0; no frames: zero sums
        assert np.all(np.isnan(dev[3, 4:6])) and np.all(np.isnan(dev[3, 8])) and np.all(dev[3, 0] == 0.0)
        assert np.all(dev[4, 4:6] == 0.0) and np.all(np.isnan(dev[4, 6:9])) and np.all(dev[4, 9] == -np.inf)
        assert np.all(np.isnan(dev[5, 4:10])) and np.all(dev[5, 10] == 0.0)
        assert np.all(dev[8, :4] == 0.0) and np.all(np.isnan(dev[8, 4:10]))
        assert np.all(dev[1, 8] <= 1.0)
        print(f"{window}: quotients within {worst_q:.2f} ulp (bound 4), log10 / atan2 within {worst_t:.2f} ulp (bound 8)")


def test_properties_identity_scaled_delay_and_a_quiet_channel():
    eng = _eng()
    rng = np.random.default_rng(6)
    n_fft, hop, window = 1024, 512, "hann"
    n = n_fft + 19 * hop
    x = rng.standard_normal(n + 9).astype(np.float32)
    y_scaled = np.concatenate([np.zeros(9, np.float32), (0.25 * x[:n]).astype(np.float32)])     # y[n] = 0.25 x[n - 9], exact
    y_quiet = (1e-6 * x).astype(np.float32)
    rows = [x, y_scaled, y_quiet]
    pairs = [(0, 0, 0), (0, 1, 9), (0, 2, 0)]
    dev = run(eng, rows, pairs, n_fft, hop, window)
    refs = [R.pair_reference(rows[a], rows[b], d, n_fft, hop, window) for a, b, d in pairs]
    for p, ref in enumerate(refs):
        assert ref["K"] >= 20 and max(sums_errors(dev[p], ref)) <= 1.0, (p, sums_errors(dev[p], ref))
    # y = x: H1 = 1, coherence 1 (clamped), within the propagated bound
    for p, gain in ((0, 1.0), (1, 0.25)):
        ref = refs[p]
        bxx, byy, bxy = ref["bounds"]
        bh = R.h1_bound(ref["sxx"], ref["sxy"], bxx, bxy)
        bc = R.coherence_bound(ref["sxx"], ref["syy"], ref["sxy"], bxx, byy, bxy)
        eh = np.abs((dev[p, 4] + 1j * dev[p, 5]) - gain)
        ec = 1.0 - dev[p, 8]
        bp = 1.01 * bxy / np.abs(ref["sxy"]) + 4.0 * R.U                  # |d phase| <= asin(|dSxy| / |Sxy|)
        ep = np.abs(dev[p, 10])
        print(f"gain {gain}: |H1 - gain| {eh.max():.3e} (bound {bh[np.argmax(eh / bh)]:.3e}, ratio {np.max(eh / bh):.3e});  "
              f"1 - coherence {ec.max():.3e} (ratio {np.max(ec / bc):.3e});  |phase| {ep.max():.3e} (ratio {np.max(ep / bp):.3e})")
        assert np.all(eh <= bh) and np.all(ec >= 0.0) and np.all(ec <= bc) and np.all(ep <= bp)
        assert np.all(np.abs(dev[p, 9] - 20.0 * math.log10(gain)) <= 20.0 / math.log(10.0) * 1.01 * bh / gain + 1e-14)
    # 120 dB down: the sums stay within the JOINT-norm bound (the quiet channel carries the loud one's rounding error)
    ref = refs[2]
    rxx, ryy, rxy = sums_errors(dev[2], ref)
    rel = np.abs(dev[2, 1] - ref["syy"]) / ref["syy"]
    print(f"y 120 dB below x: error / bound Sxx {rxx:.3e}, Syy {ryy:.3e}, Sxy {rxy:.3e};  largest relative Syy error "
          f"{rel.max():.3e} (bound {np.max(ref['bounds'][1] / ref['syy']):.3e}, 2^-53 = {R.U:.3e})")
    assert max(rxx, ryy, rxy) <= 1.0
    eh = np.abs((dev[2, 4] + 1j * dev[2, 5]) - (ref["rows"][4] + 1j * ref["rows"][5]))
    assert np.all(eh <= R.h1_bound(ref["sxx"], ref["sxy"], ref["bounds"][0], ref["bounds"][2]))
    assert np.all(np.abs(np.abs(dev[2, 4] + 1j * dev[2, 5]) - 1e-6) < 1e-9)          # float32 rounding of 1e-6 x


def test_degenerate_pairs_get_their_status_and_leave_the_others_alone():
    from audio_analysis_amd.analyse import transfer as T
    eng = _eng()
    rng = np.random.default_rng(7)
    n_fft = 256
    st = T.TransferSettings(n_fft=n_fft, overlap=0.5, delay=0, band_hz=(1000.0, 20000.0))
    x, y = noise_pair(rng, 5000)
    x2, y2 = noise_pair(rng, 3001)
    short = rng.standard_normal(n_fft - 1).astype(np.float32)
    bad = y.copy()
    bad[1234] = np.nan
    chans = [x, y, short, np.zeros(4000, np.float32), bad, x2, y2]
    pairs = [(0, 1), (0, 2), (3, 1), (0, 4), (5, 6), (2, 2)]
    batch = eng.upload(chans)
    res = T.transfer_device(eng, batch, [a for a, _ in pairs], [b for _, b in pairs], SR, st)
    out = T.transfer_results(res, SR, [f"p{i}" for i in range(len(pairs))], st)
    assert [r.status for r in out] == [0, T.STATUS_TOO_SHORT, T.STATUS_SILENT_REFERENCE, T.STATUS_NON_FINITE, 0, T.STATUS_TOO_SHORT]
    assert list(res.frames) == [38, 0, 30, 38, 22, 0] and list(res.samples) == [5000, 255, 4000, 5000, 3001, 255]
    for r in out:
        if r.status:
            assert all(np.all(np.isnan(r.arrays[k])) for k in T.ARRAYS) and math.isnan(r.mean_coherence)
            assert all(math.isnan(b.mag_db) for b in r.rows) and "NA" in T.summarise_transfer_text([r])
    assert np.all(res.out[1, :4] == 0.0) and np.all(res.out[2, 0] == 0.0) and np.all(np.isnan(res.out[3, :4]))
    # the good pairs: within the bound, and the same bytes as in batches of their own
    for p, (a, b) in ((0, (0, 1)), (4, (5, 6))):
        ref = R.pair_reference(chans[a], chans[b], 0, n_fft, st.hop, "hann")
        errs = sums_errors(res.out[p], ref)
        print(f"pair {p} beside the degenerate ones: error / bound {max(errs):.3e}")
        assert max(errs) <= 1.0 and ref["status"] == 0
        alone = T.transfer_device(eng, eng.upload([chans[a], chans[b]]), [0], [1], SR, st)
        assert alone.out[0].tobytes() == res.out[p].tobytes()
        assert 0.0 < out[p].mean_coherence < 1.0 and 0.0 <= out[p].coherent_fraction <= 1.0
    for p, (a, b) in enumerate(pairs):
        assert R.pair_reference(chans[a], chans[b], 0, n_fft, st.hop, "hann")["status"] == out[p].status
    # an empty batch: no launch, empty results
    empty = T.transfer_device(eng, batch, [], [], SR, st)
    assert empty.out.shape == (0, 11, n_fft // 2 + 1) and T.transfer_results(empty, SR, [], st) == []
    e = eng.cross_spectra(batch.x, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), n_fft, 128, True)
    assert tuple(e.shape) == (0, 11, n_fft // 2 + 1)
    assert T.analyse_transfer_batch(chans, [], SR, [], st) == []


def _delayed(x, taps, d):
    """taps * x, delayed by d samples (d < 0: advanced), the length of x, float32."""
    y = np.convolve(x.astype(np.float64), taps)[: x.size]
    out = np.zeros_like(y)
    if d >= 0:
        out[d:] = y[: y.size - d]
    else:
        out[:d] = y[-d:]
    return out.astype(np.float32)


def test_auto_delay_and_the_file_entry_point(tmp_path):
    from scipy.io import wavfile
    from audio_analysis_amd.analyse import transfer as T
    eng = _eng()
    rng = np.random.default_rng(8)
    x = (0.1 * rng.standard_normal(30000)).astype(np.float32)
    taps = (1.0, 0.3, -0.2)
    late, early = _delayed(x, taps, 300), _delayed(x, taps, -300)
    batch = eng.upload([x, late, early])
    d = T.find_delay_device(eng, batch, [0, 0], [1, 2], SR)
    print(f"delays found: {list(d)} (set: [300, -300])")
    assert list(d) == [300, -300]
    # module level, from files: the reference file stereo (mixed down), the measured file mono
    wavfile.write(str(tmp_path / "ref.wav"), SR, np.stack([x, x], axis=1))
    wavfile.write(str(tmp_path / "late.wav"), SR, late)
    st = T.TransferSettings(n_fft=1024, overlap=0.5)
    (r,) = T.analyse_transfer_files([tmp_path / "late.wav"], tmp_path / "ref.wav", st, SR)
    assert (r.pair_name, r.delay_samples, r.status, r.n_fft, r.hop) == ("late.wav:mono", 300, 0, 1024, 512)
    ref = R.pair_reference(x, late, 300, 1024, 512, "hann")
    assert r.frames == ref["K"] and r.samples == 29700
    dev = np.stack([r.arrays[k] for k in T.ARRAYS])
    errs = sums_errors(dev, ref)
    bxx, byy, bxy = ref["bounds"]
    eh = np.abs((dev[4] + 1j * dev[5]) - (ref["rows"][4] + 1j * ref["rows"][5]))
    bh = R.h1_bound(ref["sxx"], ref["sxy"], bxx, bxy)
    print(f"files: sums error / bound {max(errs):.3e}; |H1 - ref| / bound {np.max(eh / bh):.3e}")
    assert max(errs) <= 1.0 and np.all(eh <= bh)
    freq = r.frequency_hz
    band = (freq >= 20.0) & (freq <= 20000.0)
    assert r.mean_coherence == pytest.approx(float(np.mean(ref["rows"][8][band])), abs=1e-9) and r.mean_coherence > 0.99
    # the three taps: |H1| at DC is their sum
    assert abs(math.hypot(dev[4][0], dev[5][0]) - 1.1) < 0.02


def test_cli_writes_a_json_document_that_round_trips(tmp_path):
    from scipy.io import wavfile
    from audio_analysis_amd.analyse import transfer as T
    rng = np.random.default_rng(9)
    x = (0.1 * rng.standard_normal(12000)).astype(np.float32)
    y = _delayed(x, (0.5, 0.25), 40)
    wavfile.write(str(tmp_path / "st.wav"), SR, np.stack([x, y], axis=1))
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.transfer", "--input", str(tmp_path / "st.wav"), "--reference-channel",
                        "left", "--n-fft", "512", "--json", str(tmp_path / "o.json")], capture_output=True, text=True,
                       cwd=str(REPO), env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.startswith("[st.wav:right]\nDelay: 40 samples (0.833 ms)  Frames: 45 of 512 (hann, hop 256)")
    doc = json.loads((tmp_path / "o.json").read_text())
    (row,) = doc["transfer"]
    assert row["delay_samples"] == 40 and row["status"] == 0 and len(row["arrays"]["coherence"]) == 257
    back = T.transfer_results_from_json(doc)
    assert T.transfer_results_to_json(back) == doc and T.summarise_transfer_text(back) == r.stdout
