"""MLS measurement through the public functions of analyse/mls.py on the GPU, against tests/mls_ref.py: a known response
recovered bit for bit from recordings on the PCM16 grid, the period signal-to-noise ratio, silence and a NaN channel, the
epilogue's rules, independence of the batching, the command line's round trip, and the measurement orders 14 .. 21: a sparse
response on the 2^-9 grid recovered exactly (a closed form), Gaussian recordings bit for bit against the restatement and, at
sampled positions, within mls_ref.bound of correctly rounded sums."""
import json

import numpy as np
import pytest

import mls_ref as R

pytestmark = pytest.mark.gpu
FS = 48000


@pytest.fixture(scope="module")
def eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def _burst(seed, n=300):
    """A decaying noise burst: the response to recover."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) * np.exp(-np.arange(n) / 60.0) * 0.05


def _circular(h, order, amplitude=0.5):
    """One steady-state period of the system's answer to the repeated stimulus, float64."""
    p = (1 << order) - 1
    s = amplitude * R.sequence(order).astype(np.float64)
    hp = np.zeros(p)
    hp[: h.size] = h
    return np.real(np.fft.ifft(np.fft.fft(hp) * np.fft.fft(s)))


def _on_grid(y):
    k = np.rint(y * 32768.0)
    assert np.abs(k).max() < 32768, "the test signal would clip"
    return (k / 32768.0).astype(np.float32)


RAW = dict(normalise_peak=False, remove_dc=False)


@pytest.mark.parametrize("order,periods_played", [(10, 4), (13, 4)])
def test_grid_input_equals_the_int64_restatement(eng, order, periods_played):
    from audio_analysis_amd.analyse import mls as D
    p = (1 << order) - 1
    h = _burst(order)
    rec = np.tile(_on_grid(_circular(h, order)), periods_played)
    hs, res = D.mls_impulse_responses([rec], FS, D.MlsSettings(order=order, **RAW), eng=eng)
    assert res[0].periods == periods_played - 1 == 3 and res[0].begin_samples == p and res[0].period_samples == p
    ref64, ref32 = R.grid_int64(rec, p, order, 3)
    assert hs[0].dtype == np.float32 and np.array_equal(R.bits_of(hs[0]), R.bits_of(ref32))
    # against h itself: the stimulus has the level 0.5, so the measured response is 0.5 h.  A sample of the recording is off
    # by at most 2^-16 (half a step of the grid), so c[k] and sum Y by at most R P 2^-16 each and h[k] by less than 2^-15;
    # the float32 result adds 2^-24 |h|.  The restatement shows the same error to the bit.
    true = np.zeros(p)
    true[: h.size] = 0.5 * h
    err = np.abs(hs[0].astype(np.float64) - true)
    allowed = 2.0 ** -15 + 2.0 ** -24 * np.abs(true)
    print(f"order {order}: worst error {err.max():.3e} ({float((err / allowed).max()):.3f} of the quantisation bound)")
    assert np.all(err <= allowed)
    assert np.array_equal(err, np.abs(ref32.astype(np.float64) - true))
    assert res[0].peak_samples == int(np.argmax(np.abs(ref32))) and res[0].peak_value == float(np.abs(ref32).max())
    assert res[0].period_snr_db == np.inf                    # identical periods: D = 0


def test_period_snr_with_known_noise(eng):
    from audio_analysis_amd.analyse import mls as D
    order, periods = 10, 8
    p = (1 << order) - 1
    rng = np.random.default_rng(3)
    clean = np.tile(_circular(_burst(1), order), periods + 1)
    rec = (clean + 0.01 * rng.standard_normal(clean.size)).astype(np.float32)
    _, res = D.mls_impulse_responses([rec], FS, D.MlsSettings(order=order), eng=eng)
    e, d, _, _ = R.sums_ld(rec, p, p, periods)
    ref = float(10.0 * np.log10((e / periods) / d))
    # what to expect: E / R ~ R P sigma_y^2, D ~ (R - 1) P sigma_n^2
    rough = 10.0 * np.log10(periods * np.var(clean[:p]) / ((periods - 1) * 1e-4))
    print(f"period_snr_db {res[0].period_snr_db:.4f}, long double {ref:.4f}, from the levels {rough:.2f}")
    assert res[0].periods == periods and abs(res[0].period_snr_db - ref) <= 0.5
    assert abs(ref - rough) <= 1.0


def test_silence_and_a_nan_channel(eng):
    from audio_analysis_amd.analyse import mls as D
    order = 9
    p = (1 << order) - 1
    good = np.tile(_on_grid(_circular(_burst(2), order)), 3)
    st = D.MlsSettings(order=order)
    hs, res = D.mls_impulse_responses([np.zeros(3 * p, np.float32)], FS, st, eng=eng)
    assert np.array_equal(R.bits_of(hs[0]), np.zeros(p, np.uint32)) and res[0].peak_value == 0.0
    bad = good.copy() * np.float32(3.0)                       # it would own the file's peak
    bad[p + 17] = np.nan
    alone, _ = D.mls_impulse_responses([good], FS, st, eng=eng)
    pair, res = D.mls_impulse_responses([good, bad], FS, st, eng=eng, file_of_channel=[0, 0])
    assert np.isnan(pair[1]).all() and np.isnan(res[1].peak_value) and np.isnan(res[1].period_snr_db)
    assert np.array_equal(R.bits_of(pair[0]), R.bits_of(alone[0])), "a NaN channel moved the other channel of its file"
    assert np.isfinite(pair[0]).all() and abs(float(np.abs(pair[0]).max()) - 0.95) <= 1e-6


def test_epilogue_follows_deconv_finish(eng):
    from audio_analysis_amd.analyse import mls as D
    order = 10
    left = np.tile(_on_grid(_circular(_burst(4), order) + 0.01), 3)
    right = np.tile(_on_grid(0.3 * _circular(_burst(5), order) - 0.02), 3)
    raw, _ = D.mls_impulse_responses([left, right], FS, D.MlsSettings(order=order, **RAW), eng=eng)
    got, _ = D.mls_impulse_responses([left, right], FS, D.MlsSettings(order=order), eng=eng, file_of_channel=[0, 0])
    split, _ = D.mls_impulse_responses([left, right], FS, D.MlsSettings(order=order), eng=eng, file_of_channel=[0, 1])
    # deconvolve.py's rules: the mean leaves each channel (float64 mean rounded to float32, float32 subtraction), then one
    # float32 scale target / peak per file.  The mean's float64 sum may differ from NumPy's in its last bit: 2 ulp of 0.95.
    centred = [v - np.float32(v.astype(np.float64).mean()) for v in raw]
    peak = max(float(np.abs(v).max()) for v in centred)
    for c in range(2):
        want = centred[c] * np.float32(0.95 / peak)
        assert np.abs(got[c] - want).max() <= 2.0 ** -22
        own = centred[c] * np.float32(0.95 / float(np.abs(centred[c]).max()))
        assert np.abs(split[c] - own).max() <= 2.0 ** -22
    assert abs(max(float(np.abs(v).max()) for v in got) - 0.95) <= 2.0 ** -22
    assert float(np.abs(got[1]).max()) < 0.5                 # the quiet channel keeps its level relative to the loud one


def _batching(eng, monkeypatch, order):
    from audio_analysis_amd import engine as E
    from audio_analysis_amd.analyse import mls as D
    p = (1 << order) - 1
    rng = np.random.default_rng(order)
    # different lengths: R = 2, 4, 2, 3, 4 -- the chains are grouped by R
    chans = [rng.standard_normal((r + 1) * p + k).astype(np.float32) for k, r in enumerate((2, 4, 2, 3, 4))]
    st = D.MlsSettings(order=order)
    files = list(range(5))
    whole, res = D.mls_impulse_responses(chans, FS, st, eng=eng, file_of_channel=files)
    assert [r.periods for r in res] == [2, 4, 2, 3, 4]
    monkeypatch.setattr(E, "MLS_SCRATCH_BYTES", E.mls_scratch_bytes(1, order))       # one channel a chain
    cut, res_cut = D.mls_impulse_responses(chans, FS, st, eng=eng, file_of_channel=files)
    for c in range(5):
        one, res_one = D.mls_impulse_responses([chans[c]], FS, st, eng=eng)
        assert np.array_equal(R.bits_of(whole[c]), R.bits_of(one[0])) and np.array_equal(R.bits_of(cut[c]), R.bits_of(one[0]))
        assert res[c].period_snr_db == res_one[0].period_snr_db == res_cut[c].period_snr_db
        assert res[c].peak_samples == res_one[0].peak_samples


def test_results_do_not_depend_on_the_batching(eng, monkeypatch):
    _batching(eng, monkeypatch, 8)


def test_results_do_not_depend_on_the_batching_at_order_16(eng, monkeypatch):
    """Two passes of the transform and two samples a thread in the fold and the finish."""
    _batching(eng, monkeypatch, 16)


# ------------------------------------------------------------------------------------------- the measurement orders
MEASUREMENT_ORDERS = tuple(range(14, 22))           # 0.3 s to 44 s of sequence at 48 kHz


def _sequence(order):
    from audio_analysis_amd.engine import mls_bits       # tests/test_mls_cpu.py holds it to the plain recurrence up here
    return 1 - 2 * mls_bits(order).astype(np.int64)


@pytest.mark.parametrize("order", MEASUREMENT_ORDERS)
def test_a_sparse_response_comes_back_exactly(eng, order):
    """Two channels, each R periods (3; 2 at order 21) of the amplitude-0.5 sequence circularly convolved with twelve taps
    k / 256, indices 0 and P - 1 among them.  Every intermediate of the chain is an integer multiple of 2^-9 far below 2^53
    (|Y| < 2^5, |W| < 2^(m + 5)), so nothing rounds and the response is 0.5 h exactly, zeros included.  The reference is the
    closed form: it owes nothing to mls_ref.fwht."""
    from audio_analysis_amd.analyse import mls as D
    p, periods = (1 << order) - 1, 2 if order == 21 else 3
    s = _sequence(order)
    hs_true = [R.sparse_response(order, 10 * order + c) for c in range(2)]
    recs = []
    for h in hs_true:
        y = R.sparse_period(h, s)
        assert np.count_nonzero(h) == 12 and h[0] != 0.0 and h[p - 1] != 0.0
        assert np.array_equal(np.rint(y * 512.0), y * 512.0) and np.abs(y).max() <= 6.0
        recs.append(np.tile(y.astype(np.float32), periods + 1))
    hs, res = D.mls_impulse_responses(recs, FS, D.MlsSettings(order=order, **RAW), eng=eng)
    for c in range(2):
        assert res[c].periods == periods and res[c].begin_samples == p
        want = (0.5 * hs_true[c]).astype(np.float32)
        differ = R.bits_of(hs[c]) != R.bits_of(want)
        assert not differ.any(), f"order {order} channel {c}: {int(differ.sum())} samples differ, first at {int(np.argmax(differ))}"
        assert res[c].period_snr_db == np.inf                # identical periods: D = 0


@pytest.mark.parametrize("order", MEASUREMENT_ORDERS)
def test_gaussian_recordings_at_the_measurement_orders(eng, order):
    """Off the grid, R = 2, two channels: the response equals the restatement's to the bit, and at k = 0, 1, P - 1 and seeded
    positions the restatement's float64 value lies within mls_ref.bound of correctly rounded sums (mls_ref.sampled_ld).
    The device's float32 is that float64 rounded once more: half an ulp, 2^-24 |h|, on top.
    Measured on an MI355X: equal to the bit at every order; the worst sampled error over the bound was 0 at orders 14, 15 and
    16 (signed sums of that few float32 values still fit a float64 exactly at the sampled positions), 1.8e-4, 1.7e-4, 1.7e-4, 7.9e-5 and 1.1e-4 at
    orders 17 .. 21."""
    from audio_analysis_amd.analyse import mls as D
    from audio_analysis_amd.engine import mls_tables
    if np.finfo(np.longdouble).eps >= 2.0 ** -60:
        pytest.skip("numpy.longdouble is no wider than float64 here")
    p, periods = (1 << order) - 1, 2
    rng = np.random.default_rng(2000 + order)
    recs = [rng.standard_normal((periods + 1) * p).astype(np.float32) for _ in range(2)]
    hs, res = D.mls_impulse_responses(recs, FS, D.MlsSettings(order=order, **RAW), eng=eng)
    s = _sequence(order)
    worst = 0.0
    for c in range(2):
        assert res[c].periods == periods
        ch = R.fast_chain(recs[c], p, order, periods, tabs=mls_tables(order))
        differ = R.bits_of(hs[c]) != R.bits_of(ch["h"])
        assert not differ.any(), f"order {order} channel {c}: {int(differ.sum())} samples differ, first at {int(np.argmax(differ))}"
        ks = R.sample_positions(order, 100 * order + c, 8 if c == 0 else 4)
        ref = R.sampled_ld(ch["Y"], s, order, periods, ks)
        bound = R.bound(order, periods, ch["Y"])
        err = np.abs(ch["h64"][ks].astype(np.longdouble) - ref)
        worst = max(worst, float(err.max() / bound))
        assert np.all(err <= bound)
        assert np.all(np.abs(hs[c][ks].astype(np.longdouble) - ref) <= bound + 2.0 ** -24 * np.abs(ref))
    print(f"order {order} R {periods}: worst sampled error {worst:.3g} of the bound")


def test_generate_then_deconvolve_round_trips_a_room(eng, tmp_path, capsys):
    from scipy.io import wavfile
    from audio_analysis_amd.analyse import mls as D
    order = 10
    p = (1 << order) - 1
    stim = tmp_path / "stimulus.wav"
    D.main(["generate", "--order", str(order), "--periods", "4", "--output", str(stim)])
    fs, s = wavfile.read(str(stim))
    s = np.asarray(s, dtype=np.float64).reshape(-1)
    assert fs == FS and s.size == 4 * p and set(np.unique(s)) == {-0.5, 0.5}
    room = _burst(6)
    rec = np.convolve(s, room)[: 4 * p].astype(np.float32)
    wavfile.write(str(tmp_path / "hall.wav"), FS, rec)
    out_json = tmp_path / "hall.json"
    D.main(["deconvolve", "--recorded", str(tmp_path / "hall.wav"), "--order", str(order), "--no-normalise", "--keep-dc",
            "--output-dir", str(tmp_path / "out"), "--json", str(out_json)])
    text = capsys.readouterr().out
    assert "[hall.wav:mono]" in text and "hall_ir.wav" in text
    fs, ir = wavfile.read(str(tmp_path / "out" / "hall_ir.wav"))
    ir = np.asarray(ir).reshape(-1)
    assert fs == FS and ir.dtype == np.float32 and ir.size == p
    true = np.zeros(p)
    true[: room.size] = 0.5 * room                           # relative to a +-1 sequence: the stimulus' level stays in
    # float32 samples of the recording: 2^-24 relative each, averaged over three periods
    assert np.abs(ir - true).max() <= 1e-6
    doc = json.loads(out_json.read_text())
    assert doc["mls"][0]["periods"] == 3 and doc["mls"][0]["peak_samples"] == int(np.argmax(np.abs(true)))
