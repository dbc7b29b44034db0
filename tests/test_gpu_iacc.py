"""
ISO 3382-1 inter-channel cross-correlation on the device (ira_onset_index + ira_xcorr_windows,
audio_analysis_amd.analyse.iacc) against a long-double NumPy restatement of the definitions in the module's docstring
(xcorr_ref.py); a closed form that does not use the restatement; band signals against the oracle's float64 filter bank.

Tolerance of the raw sums (the energy tests' tolerance): |C_dev - C_ref| <= 1e-12 sqrt(El_ref Er_ref) per partition and lag,
El and Er to 1e-12 relative.  NumPy float64 sums of a 100 003-sample pair sit 7.6e-18 from the long-double values on that
scale and a deliberately sequential float64 sum 3e-16, so the margin is about four orders of magnitude whatever the
kernel's summation order.
"""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import ira_oracle as O
from xcorr_ref import narrow, ref_coefficient, ref_onset, ref_sums

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
SR = 48000
CH = 4096                # XC_CHUNK of audio_analysis_amd/csrc/ira_xcorr.hip: rows (counted from the onset) per workgroup
LD = np.longdouble


# ------------------------------------------------------------------------------------------------ the restatement: xcorr_ref.py
def assert_sums(dev, ref, what):
    ref64 = ref.astype(np.float64)
    nlag = ref.shape[1] - 2
    for j in range(ref.shape[0]):
        el, er = ref64[j, nlag], ref64[j, nlag + 1]
        err = float(np.max(np.abs((dev[j, :nlag].astype(LD) - ref[j, :nlag]).astype(np.float64))))
        assert err <= 1e-12 * math.sqrt(el * er), (what, j, err, el, er)
        assert abs(dev[j, nlag] - el) <= 1e-12 * el and abs(dev[j, nlag + 1] - er) <= 1e-12 * er, (what, j)


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def device_sums(eng, pairs, limits, tmax, lead=()):
    """Engine level: the onsets of every channel and the raw sums of every (l, r) pair, one batch, one launch.  `lead`:
    channels uploaded in front of the pairs (they shift everything behind them)."""
    chans = [np.asarray(c, np.float32) for c in lead] + [np.asarray(c, np.float32) for p in pairs for c in p]
    b = eng.upload(chans)
    on, _, _ = eng.onset_index(b, 0.01)
    k = len(lead)
    li = np.arange(k, k + 2 * len(pairs), 2)
    out = eng.xcorr_windows(b.x, b.off[li], b.off[li + 1], b.length[li], li.astype(np.int32), (li + 1).astype(np.int32), on,
                            np.asarray(limits, dtype=np.int64).reshape(len(pairs), -1), tmax)
    return on.cpu().numpy()[k:].reshape(-1, 2), out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ raw sums
T0 = 48
# (length, pre-delay of l, pre-delay of r): every length at which the chunking changes, onset 0, an onset in the last
# chunk, different onsets in the two channels, a pair shorter than the lag range
_SPEC = [(CH - 1, 0, 0), (CH, 0, 7), (CH + 1, 5, 0), (CH + T0, 0, 0), (2 * CH + T0 + 1, 2 * CH + 9, 2 * CH + 9),
         (100003, 555, 540), (30, 3, 3), (2 * CH + T0 + 1, 100, 131), (CH + 2, 0, 0)]
_LIM4 = [CH - 1, CH, CH + 1, 3 * CH]                       # a limit on a chunk boundary and one sample either side of it
_cache = {}


def _pairs():
    from audio_analysis_amd.synth import synth_ir
    if "pairs" not in _cache:
        _cache["pairs"] = [(synth_ir(i, 0, n, SR, rt60_seconds=0.2 + 0.3 * i, pre_delay=dl),
                            synth_ir(i, 1, n, SR, rt60_seconds=0.25 + 0.3 * i, pre_delay=dr))
                           for i, (n, dl, dr) in enumerate(_SPEC)]
    return _cache["pairs"]


def _one_limit(pair_index):
    """One limit per pair; the last pair (onset 0) gets L = N_K + 1."""
    n, dl, dr = _SPEC[pair_index]
    return [n - 1] if pair_index == len(_SPEC) - 1 else [3840]


_TREF = {4: 128, 1: 48}       # the largest T each limit set is run at


def _reference(nlim):
    """Long-double sums of every pair at the largest T of the limit set, computed once; smaller T are cut out of them."""
    if nlim not in _cache:
        pairs = _pairs()
        lims = [_LIM4 if nlim == 4 else _one_limit(i) for i in range(len(pairs))]
        _cache[nlim] = [ref_sums(l, r, min(ref_onset(l), ref_onset(r)), lim, _TREF[nlim]) for (l, r), lim in zip(pairs, lims)]
    return _cache[nlim]


@pytest.mark.parametrize("tmax,nlim", [(48, 4), (48, 1), (1, 1), (128, 4)])
def test_raw_sums_ragged_batch_vs_restatement(tmax, nlim):
    eng = _eng()
    pairs = _pairs()
    lims = [_LIM4 if nlim == 4 else _one_limit(i) for i in range(len(pairs))]
    on, out = device_sums(eng, pairs, lims, tmax)
    assert out.shape == (len(pairs), nlim + 1, 2 * tmax + 3)
    ref = _reference(nlim)
    for i, (l, r) in enumerate(pairs):
        assert (on[i, 0], on[i, 1]) == (ref_onset(l), ref_onset(r)) == (_SPEC[i][1], _SPEC[i][2]), i
        assert_sums(out[i], narrow(ref[i], _TREF[nlim], tmax), (tmax, nlim, i))
    if nlim == 1:                                            # L = N_K + 1: the late partition is the last sample alone
        l, r = pairs[-1]
        assert out[-1, 1, 2 * tmax + 1] == float(l[-1]) ** 2 and out[-1, 1, tmax] == float(l[-1]) * float(r[-1])
    if nlim == 4:                                            # limits past the end of a pair: empty partitions are zeros
        assert np.all(out[0, 1:] == 0.0) and np.all(out[6, 1:] == 0.0)


def test_bit_identical_whatever_the_batch():
    eng = _eng()
    pairs = _pairs()
    k = 5                                                    # the 100 003-sample pair, in the middle of the ragged batch
    for tmax, lim in ((48, _LIM4), (128, [3840])):
        _, alone = device_sums(eng, [pairs[k]], [lim], tmax)
        _, many = device_sums(eng, pairs, [lim] * len(pairs), tmax)
        assert np.array_equal(many[k].view(np.uint64), alone[0].view(np.uint64))
        for shift in (1, 3):                                 # the pair starts 4 or 12 bytes past a 16-byte line
            _, mis = device_sums(eng, [pairs[k]], [lim], tmax, lead=[np.full(shift, 0.25, np.float32)])
            assert np.array_equal(mis[0].view(np.uint64), alone[0].view(np.uint64)), shift
        _, last = device_sums(eng, pairs[:k] + pairs[k + 1 :] + [pairs[k]], [lim] * len(pairs), tmax)
        assert np.array_equal(last[-1].view(np.uint64), alone[0].view(np.uint64))


# ------------------------------------------------------------------------------------------------ closed form
def test_delayed_copy_closed_form():
    """r[n] = 0.5 l[n - 17] with the last 64 samples of l zeroed: C(17) = 0.5 El and Er = 0.25 El exactly, so the
    whole-response IACC is 1 (the float64 value is 1 + 2.2e-16: sqrt and divide round) at tau = +17 samples, the right
    channel lagging; the pair's onset is the left channel's."""
    from audio_analysis_amd.analyse import iacc as I
    from audio_analysis_amd.synth import synth_ir
    l = synth_ir(60, 0, 20000, SR, rt60_seconds=0.5)
    l[-64:] = 0.0
    r = np.zeros_like(l)
    r[17:] = np.float32(0.5) * l[:-17]
    st = I.IaccSettings(bands=None)
    fwd, swapped, neg = I.analyse_iacc_pairs_batch([l, r, l], [r, l, -r], SR, ["fwd", "swapped", "neg"], st)
    ulp = np.finfo(np.float64).eps
    for res, tau in ((fwd, 17), (swapped, -17), (neg, 17)):
        print(f"closed form {res.pair_name}: IACC_A - 1 = {res.broadband.whole - 1.0:.3e}, tau = {res.broadband.tau_whole_seconds * SR:g}")
        assert res.status == 0 and res.onset_samples == ref_onset(l) and res.max_lag_samples == 48
        assert abs(res.broadband.whole - 1.0) <= 4 * ulp, res.broadband.whole
        assert res.broadband.tau_whole_seconds == tau / SR
    assert neg.broadband == fwd.broadband


# ------------------------------------------------------------------------------------------------ bands
def _oracle_band_signals(x, sr, mode):
    n = x.size
    f = np.fft.rfftfreq(n, d=1.0 / float(sr)).astype(np.float32)
    spec = np.fft.rfft(x.astype(np.float64))
    out = []
    for b in O.band_definitions(sr, band_mode=mode):
        m = O.band_mask(f, b, 1.0 / 6.0, 0.5 * float(sr))
        out.append((b["name"], np.fft.irfft(spec * m.astype(np.float64), n=n).astype(np.float32)))
    return out


@pytest.mark.parametrize("mode,n", [("octave", 48000), ("three", 20000)])
def test_band_path_vs_oracle_filter_bank(mode, n):
    """Full band path (filter bank on the device + lag sums) against the restatement on the oracle's float64 band signals
    rounded to float32: IACC within 1e-6, tau equal wherever the runner-up lag is more than 1e-6 below the maximum."""
    from audio_analysis_amd.analyse import iacc as I
    from audio_analysis_amd.analyse.rt60bands import Rt60BandsAnalysisSettings
    from audio_analysis_amd.synth import synth_ir
    l = synth_ir(70, 0, n, SR, rt60_seconds=0.6)
    r = (0.6 * synth_ir(70, 1, n, SR, rt60_seconds=0.7) + 0.4 * np.roll(l, 9)).astype(np.float32)   # partly correlated
    st = I.IaccSettings(bands=Rt60BandsAnalysisSettings(band_mode=mode), early_limits_ms=(50.0, 80.0))
    res = I.analyse_iacc_pairs_batch([l], [r], SR, ["p"], st)[0]
    o = min(ref_onset(l), ref_onset(r))
    lim = [2400, 3840]
    assert res.status == 0 and res.onset_samples == o
    bl, br = _oracle_band_signals(l, SR, mode), _oracle_band_signals(r, SR, mode)
    assert [b.name for b in res.band_definitions] == [nm for nm, _ in bl]
    rows = [("Broadband", l, r, res.broadband)] + [(nm, yl, yr, res.band_values_by_name[nm]) for (nm, yl), (_, yr) in zip(bl, br)]
    for name, yl, yr, got in rows:
        p = ref_sums(yl, yr, o, lim, 48)
        cells = [(p[0], got.early[0], got.tau_early_seconds[0]), (p[1] + p[2], got.late[0], got.tau_late_seconds[0]),
                 (p[0] + p[1], got.early[1], got.tau_early_seconds[1]), (p[2], got.late[1], got.tau_late_seconds[1]),
                 ((p[0] + p[1]) + p[2], got.whole, got.tau_whole_seconds)]
        for c, (rec, iacc, tau_s) in enumerate(cells):
            want, tau, iacf = ref_coefficient(rec)
            print(f"bands {mode} {name} cell {c}: IACC {iacc:.9f}, off by {iacc - want:.3e}")
            assert abs(iacc - want) <= 1e-6, (mode, name, c, iacc, want)
            if np.sort(iacf)[-2] < want - 1e-6:
                assert tau_s == tau / SR, (mode, name, c, tau_s * SR, tau)
    if mode == "octave":
        assert res.iacc_e3 == sum(res.band_values_by_name[nm].early[0] for nm in ("500Hz", "1000Hz", "2000Hz")) / 3.0
    else:
        assert math.isnan(res.iacc_e3)


# ------------------------------------------------------------------------------------------------ status
def test_status_flags_keep_the_rest_of_the_batch(tmp_path):
    from scipy.io import wavfile
    from audio_analysis_amd.analyse import iacc as I
    from audio_analysis_amd.synth import synth_ir
    gl, gr = synth_ir(80, 0, 30000, SR, rt60_seconds=0.4), synth_ir(80, 1, 30000, SR, rt60_seconds=0.45)
    silent = np.zeros(30000, np.float32)
    sl, sr_ = gl[:3840 + 240 + 80].copy(), gr[:3840 + 240 + 80].copy()   # onset 320: L = 3840 = N_K, too short
    nan = gr.copy()
    nan[5000] = np.nan
    lefts = [gl, silent, gl, sl, gl, gl]
    rights = [gr, gr, silent, sr_, nan, gr]
    st = I.IaccSettings(bands=None)
    res = I.analyse_iacc_pairs_batch(lefts, rights, SR, [str(i) for i in range(6)], st)
    alone = I.analyse_iacc_pairs_batch([gl], [gr], SR, ["g"], st)[0]
    assert ref_onset(sl) == ref_onset(sr_) == 320
    assert [r.status for r in res[:4]] == [0, I.STATUS_SILENT, I.STATUS_SILENT, I.STATUS_TOO_SHORT]
    assert res[4].status & I.STATUS_NON_FINITE and res[5].status == 0
    for i in (0, 5):
        assert res[i].broadband == alone.broadband and res[i].onset_samples == alone.onset_samples
    assert 0.0 < alone.broadband.whole < 1.0 and all(math.isfinite(v) for v in alone.broadband.early + alone.broadband.late)
    for i in (1, 2, 3, 4):
        v = res[i].broadband
        assert math.isnan(v.whole) and math.isnan(v.early[0]) and math.isnan(v.late[0]) and math.isnan(v.tau_whole_seconds)
    # with bands: a bad pair's bands are NaN too, the good ones are untouched
    resb = I.analyse_iacc_pairs_batch([gl, silent, gl], [gr, gr, gr], SR, ["a", "b", "c"], I.IaccSettings())
    assert resb[0].band_values_by_name == resb[2].band_values_by_name and resb[0].iacc_e3 == resb[2].iacc_e3
    assert all(math.isnan(p.whole) for p in resb[1].band_values_by_name.values()) and math.isnan(resb[1].iacc_e3)
    assert math.isfinite(resb[0].iacc_e3) and len(resb[0].band_values_by_name) == 9
    # a mono file in a file list: status 8, its neighbours as if it were not there
    q = lambda x: np.round(x * 32767.0).astype(np.int16)                  # noqa: E731
    wavfile.write(str(tmp_path / "a.wav"), SR, np.stack([q(gl), q(gr)], axis=1))
    wavfile.write(str(tmp_path / "m.wav"), SR, q(gl))
    wavfile.write(str(tmp_path / "b.wav"), SR, np.stack([q(gr), q(gl)], axis=1))
    files = I.analyse_iacc_files([tmp_path / "a.wav", tmp_path / "m.wav", tmp_path / "b.wav"], st)
    assert [r.pair_name for r in files] == ["a.wav", "m.wav", "b.wav"]
    assert [r.status for r in files] == [0, I.STATUS_NOT_STEREO, 0]
    assert math.isnan(files[1].broadband.whole) and math.isnan(files[1].iacc_e3)
    one = I.analyse_iacc_from_wav_file(tmp_path / "a.wav", st)
    assert len(one) == 1 and one[0].pair_name == "a.wav" and one[0].broadband == files[0].broadband
    assert 0.0 < files[2].broadband.whole < 1.0 and files[2].onset_samples == files[0].onset_samples


# ------------------------------------------------------------------------------------------------ command line
def test_cli_on_the_golden_bundle(tmp_path):
    from audio_analysis_amd.analyse import iacc as I
    env = dict(os.environ, PYTHONPATH=str(REPO))
    out_json = tmp_path / "iacc.json"
    r = subprocess.run([sys.executable, "-m", "analyse.iacc", "--bundle", "tests/golden/bundle", "--json", str(out_json)],
                       capture_output=True, text=True, cwd=str(REPO), env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    api = I.analyse_iacc_bundle(REPO / "tests" / "golden" / "bundle")
    assert r.stdout == I.summarise_iacc_text(api)
    assert [a.pair_name for a in api] == ["early", "late_hot"] and all(a.status == 0 for a in api)
    assert "IACC_E80" in r.stdout and "1000Hz" in r.stdout and "IACC_E3: " in r.stdout and "NA" not in r.stdout
    back = I.iacc_results_from_json(json.loads(out_json.read_text()))
    assert I.summarise_iacc_text(back) == r.stdout
    assert back[0].broadband == api[0].broadband and back[1].band_values_by_name == api[1].band_values_by_name
    assert I.iacc_results_to_json(back) == I.iacc_results_to_json(api)
