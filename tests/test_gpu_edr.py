"""
The energy decay relief end to end on the GPU (audio_analysis_amd/analyse/edr.py): the closed-form input of edr_ref (four
decaying sines, one per octave row) through analyse_edr_batch, the fit records against decay_ref.curve_records on the
device's own float32 curves (comparison B of decay_ref), a stereo WAV through the command line with and without the noise
subtraction and the relief, and a batch whose shortest channel has no frame.
"""
import functools
import json

import numpy as np
import pytest

import decay_ref as DR
import edr_ref as R

pytestmark = pytest.mark.gpu

FS = 48000


def _edr():
    from audio_analysis_amd.analyse import edr as D
    return D


def _octaves(D, **kw):
    return D.EdrSettings(f_min_hz=R.OCTAVE_EDGES[0], f_max_hz=R.OCTAVE_EDGES[1], points_per_octave=1, **kw)


@functools.lru_cache(maxsize=None)
def tones():
    x = R.closed_form_input()
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("n_fft,hop", [(2048, 256), (4096, 512)])
def test_closed_form_input_gives_the_nominal_times(n_fft, hop):
    D = _edr()
    st = _octaves(D, n_fft=n_fft, hop_length=hop)
    r = D.analyse_edr_batch([tones()], FS, ["tones"], st)[0]
    assert r.centre_hz.size == 7 and np.allclose(r.centre_hz[list(R.OCCUPIED)], R.TONES_HZ, rtol=1e-6)
    assert r.frames == 1 + (r.analysis_length_samples - n_fft) // hop and r.relief_db.shape == (7, r.frames)
    worst = 0.0
    for j, t60 in zip(R.OCCUPIED, R.TONES_T60):
        assert r.status[j] == 0 and r.edt_valid[j] and r.t20_valid[j] and r.t30_valid[j]
        rel = np.abs(np.array([r.edt_seconds[j], r.t20_seconds[j], r.t30_seconds[j]]) - t60) / t60
        worst = max(worst, float(rel.max()))
        assert np.all(rel <= 1e-3), (j, rel)
    print(f"({n_fft}, {hop}): worst relative deviation from the nominal times {worst:.3g}")
    # the longest decay is the 1.6 s tone's: in its own row, or in the next one, which holds nothing but its leakage
    assert r.longest_t30_hz == r.centre_hz[int(np.nanargmax(r.t30_seconds))] and r.longest_t30_hz in r.centre_hz[:2]
    assert r.median_t30_seconds == np.median(r.t30_seconds[r.t30_valid]) and r.initial_level_db.max() == 0.0
    assert np.all(r.relief_db[:, 0] == 0.0)                                 # L(0, j) is exactly 0 dB


def test_fit_records_equal_the_oracle_on_the_devices_own_curves():
    from audio_analysis_amd.engine import get_engine
    D = _edr()
    eng = get_engine()
    st = _octaves(D, n_fft=2048, hop_length=256)
    x = tones()
    batch = eng.upload([x, x[: FS]])
    dev = D.edr_device(eng, batch, FS, st)
    curves, fits = dev.curves.cpu().numpy(), dev.fits.cpu().numpy().reshape(2, 7, 3, 8)
    stats = {}
    for ch in range(2):
        T = int(dev.frames[ch])
        c = curves[int(dev.curve_off[ch]) :][: 7 * T].reshape(7, T)
        for j in range(7):
            ref, _ = DR.curve_records(c[j], R.RANGES, (), st.min_fit_points, t_mul=float(st.hop_length), t_div=float(FS))
            DR.compare_records(fits[ch, j], ref, stats)
    print("records against the oracle on the device's curves:", stats)


def _write_wav(path, left, right):
    from scipy.io import wavfile
    wavfile.write(str(path), FS, np.stack([left, right], axis=1).astype(np.float32))


def test_stereo_wav_through_the_command_line(tmp_path, capsys):
    D = _edr()
    x = tones().astype(np.float64)
    rng = np.random.default_rng(11)
    noisy = x + rng.standard_normal(x.size) * (np.sqrt(np.mean(x[: FS // 10] ** 2)) * 10.0 ** (-50.0 / 20.0))
    wav = tmp_path / "tones.wav"
    _write_wav(wav, x.astype(np.float32), noisy.astype(np.float32))
    base = ["--input", str(wav), "--f-min", repr(R.OCTAVE_EDGES[0]), "--f-max", repr(R.OCTAVE_EDGES[1]), "--points-per-octave", "1"]

    def run(extra, name):
        out = tmp_path / name
        D.main(base + extra + ["--json", str(out)])
        doc = json.loads(out.read_text())
        res = D.edr_results_from_json(doc)
        assert D.edr_results_to_json(res) == doc                            # the round trip
        return doc, res

    doc0, plain = run([], "plain.json")
    text = capsys.readouterr().out
    assert [r.channel_name for r in plain] == ["tones.wav:left", "tones.wav:right"] and text.count("[tones.wav:") == 2
    assert text == D.summarise_edr_text(plain)
    doc1, sub = run(["--noise-tail-fraction", "0.1"], "sub.json")
    row = 2                                                                 # the 500 Hz octave
    clean, before, after = plain[0].t30_seconds[row], plain[1].t30_seconds[row], sub[1].t30_seconds[row]
    print(f"T30 at 500 Hz: clean {clean:.4f} s, noisy {before:.4f} s, noisy with the subtraction {after:.4f} s")
    assert abs(clean - 1.0) <= 1e-3 and abs(after - clean) < abs(before - clean)
    assert np.all(sub[1].noise_power > 0.0) and np.all(plain[1].noise_power == 0.0) and sub[1].noise_frames == sub[1].frames // 10
    doc2, bare = run(["--no-relief"], "bare.json")
    assert all(r.relief_db is None for r in bare) and all(r.relief_db is not None for r in plain)
    for a, b in zip(doc0["energy_decay_relief"], doc2["energy_decay_relief"]):
        assert "relief_db" in a and "relief_db" not in b and {k: v for k, v in a.items() if k != "relief_db"} == b


def test_mixed_batch_refuses_a_channel_without_a_frame():
    D = _edr()
    rng = np.random.default_rng(3)
    chans = [rng.standard_normal(n).astype(np.float32) for n in (9000, 5000, 1500)]
    with pytest.raises(ValueError, match="Not enough samples after trimming/selection for energy decay relief"):
        D.analyse_edr_batch(chans, FS, ["a", "b", "c"], D.EdrSettings(trim_to_peak=False))
    res = D.analyse_edr_batch(chans[:2], FS, ["a", "b"], D.EdrSettings(trim_to_peak=False))
    assert [r.frames for r in res] == [1 + (9000 - 2048) // 256, 1 + (5000 - 2048) // 256]
    assert np.array_equal(res[0].status != 0, res[0].bin_count == 0) and np.any(res[0].status == D.STATUS_EMPTY)
