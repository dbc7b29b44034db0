"""
Modulation transfer sums (ira_mtf_sums) and the speech transmission index (audio_analysis_amd.analyse.sti) on the device
against the long-double restatement in sti_ref.py, closed forms, the oracle's float64 filter bank and Schroeder's
prediction for an exponential decay.

Bounds.  E: 1e-12 relative (a float64 sum of non-negative terms).  m: 1e-10 absolute, derived, not measured: at
w n <= 546 turns (12.5 Hz at 48 kHz, 2^21 samples) an unreduced float64 phase would be off by 2 pi 2^-53 546 = 4e-13 and
the sums add ~1e-15; the kernel reduces the phase exactly, so it has to stay far inside.  Every test prints its measured
maximum before it asserts.
"""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import sti_ref as R
from oracle import ira_oracle as O

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
SR = 48000
C = 16384                     # IRA_MTF_CHUNK (test_sti_cpu.py checks it against the header and the module)
TOL_E, TOL_M = 1e-12, 1e-10


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def _noise_row(seed, n):
    g = np.random.default_rng(seed).standard_normal(n)
    return (g * np.exp(-3.0 * np.arange(n) / max(n, 1))).astype(np.float32)


def device_sums(eng, rows, w_rows, odd=True, lead=1):
    """Engine level: every row at its own offset of one flat buffer (odd offsets unless told otherwise), one launch."""
    off, pos = [], lead
    for r in rows:
        if odd and pos % 2 == 0:
            pos += 1
        off.append(pos)
        pos += r.size
    flat = np.full(pos + 8, 0.5, np.float32)             # the gaps are not zero: a read outside a row would show
    for o, r in zip(off, rows):
        flat[o : o + r.size] = r
    out = eng.mtf_sums(eng.to_dev(flat), np.array(off, np.int64), np.array([r.size for r in rows], np.int64),
                       np.asarray(w_rows, np.float64))
    return out.cpu().numpy()


def check_rows(got, rows, w_rows, what):
    worst_e = worst_m = 0.0
    for i, (x, w) in enumerate(zip(rows, w_rows)):
        want = R.sums(x, w)
        worst_e = max(worst_e, abs(float((R.LD(got[i, 0]) - want[0]) / want[0])))
        worst_m = max(worst_m, float(np.max(np.abs(R.m_of(got[i].astype(R.LD)) - R.m_of(want)))))
    print(f"{what}: max relative error of E {worst_e:.3e}, max absolute error of m {worst_m:.3e}")
    assert worst_e <= TOL_E and worst_m <= TOL_M, (what, worst_e, worst_m)
    return worst_e, worst_m


def _same(a, b):
    """Two results from the same samples through two separate runs of the filter bank.  Should the float32 band signals
    differ at all, they differ by a few float32 roundings d <= 4 * 2^-24 per sample, and m moves by at most
    2 sum |e' - e| / E <= 2 * 2 d = 9.5e-7 (the bound of test_module_vs_oracle_filter_bank); TI's slope is below 4.9."""
    return float(np.max(np.abs(np.array(a.mtf) - np.array(b.mtf)))) <= 1e-6 and abs(a.sti - b.sti) <= 5e-6


# ------------------------------------------------------------------------------------------------ the kernel
# A thread holds quads u < 16 of four samples, 1024 samples apart (ira_mtf.hip): lengths either side of the stride at which
# a thread's next quad becomes empty, and last quads of 1, 2, 3 and 4 samples (cnt % 4) on both sides of it and of a chunk
_EDGE_LENS = [2, 4, 5, 6, 1022, 1023, 1024, 1025, 2050, C - 2, C + 2]


@pytest.mark.parametrize("nf", [1, 14, 16])
def test_ragged_launch_vs_restatement(nf):
    eng = _eng()
    lens = [1, 3, C - 1, C, C + 1, 2 * C + 5, 100003] + _EDGE_LENS
    rows = [_noise_row(10 + i, n) for i, n in enumerate(lens)]
    freqs = {1: (12.5,), 14: R.FREQS, 16: R.FREQS + (16.0, 20.0)}[nf]
    w_rows = [R.turns(freqs, (44100, 48000)[i % 2]) for i in range(len(rows))]
    got = device_sums(eng, rows, w_rows)
    assert got.shape == (len(rows), 2 * nf + 1)
    check_rows(got, rows, w_rows, f"ragged launch, nf = {nf}")


def test_every_frequency_count_on_short_rows():
    """nf = 1 .. 16, each a launch of its own (the record, the LDS table and the fold's stride are sized by nf)."""
    eng = _eng()
    lens = [1, 6, 1023, 1026, 2050, C + 2]
    rows = [_noise_row(40 + i, n) for i, n in enumerate(lens)]
    freqs = R.FREQS + (16.0, 20.0)
    worst = (0.0, 0.0)
    for nf in range(1, 17):
        w_rows = [R.turns(freqs[:nf], (44100, 48000)[i % 2]) for i in range(len(rows))]
        got = device_sums(eng, rows, w_rows)
        assert got.shape == (len(rows), 2 * nf + 1)
        worst = tuple(map(max, worst, check_rows(got, rows, w_rows, f"short rows, nf = {nf}")))
    print(f"short rows, nf = 1 .. 16: max relative error of E {worst[0]:.3e}, max absolute error of m {worst[1]:.3e}")


def test_integer_rows_exact_energy_and_quarter_turn_sums():
    """Integer-valued samples (|x| <= 127): every square and every partial sum is an integer far below 2^53, so E is exact
    in any order, bit for bit.  At w = 0, 0.25 and 0.5 turns per sample the phase w n reduces exactly to a multiple of a
    quarter turn, where sincospi returns exactly 0 and +-1, so the three phasor factors, their products and the sums are
    exact too: A = E and B = 0 at w = 0, the sums over n % 4 with signs (+, 0, -, 0) and (0, +, 0, -) at 0.25, the
    alternating sum and 0 at 0.5.  Asserted as equalities (a zero may carry either sign)."""
    eng = _eng()
    lens = [1, 3] + _EDGE_LENS + [C - 1, C, C + 1, 2 * C + 5]
    rng = np.random.default_rng(2025)
    rows = [rng.integers(-127, 128, n).astype(np.float32) for n in lens]
    got = device_sums(eng, rows, [[0.0, 0.25, 0.5]] * len(rows))
    exact = True
    for i, x in enumerate(rows):
        e = x.astype(np.int64) ** 2
        e4 = np.concatenate([e, np.zeros(-e.size % 4, np.int64)]).reshape(-1, 4).sum(axis=0)
        want = [e.sum(), e.sum(), 0, e4[0] - e4[2], e4[1] - e4[3], e4[0] - e4[1] + e4[2] - e4[3], 0]
        assert got[i, 0].view(np.uint64) == np.float64(want[0]).view(np.uint64), (lens[i], got[i, 0], want[0])
        if not np.array_equal(got[i], np.array(want, np.float64)):
            exact = False
            print(f"length {lens[i]}: got {got[i].tolist()}, want {want}")
    print(f"integer rows at w = 0, 0.25, 0.5: A and B exact at every length: {exact}")
    assert exact


def test_long_row_of_2_21_samples():
    """The case a drifting recurrence or an unreduced phase fails: w n reaches 546 turns."""
    eng = _eng()
    n = 1 << 21
    g = np.random.default_rng(77).standard_normal(n)
    x = (g * np.exp(-2.0 * np.arange(n) / n)).astype(np.float32)       # the end of the row still carries weight
    w = R.turns(R.FREQS, SR)
    got = device_sums(eng, [x], [w])
    check_rows(got, [x], [w], "row of 2^21 samples, nf = 14")
    tail = np.zeros(n, np.float32)
    tail[-3] = 0.9                                                       # all of the energy at the far end
    got = device_sums(eng, [tail], [w])
    m = R.m_of(got[0].astype(R.LD))
    print(f"impulse at sample 2^21 - 3: max |m - 1| {np.max(np.abs(m - 1.0)):.3e}")
    assert np.max(np.abs(m - 1.0)) <= 1e-15 and got[0, 0] == np.float64(np.float32(0.9)) ** 2


def test_bit_identical_whatever_the_batch_and_alignment():
    eng = _eng()
    x = _noise_row(5, 250001)
    w = R.turns(R.FREQS, SR)
    alone = device_sums(eng, [x], [w], odd=False, lead=0)
    rng = np.random.default_rng(3)
    others = [_noise_row(100 + k, int(rng.integers(1, 60000))) for k in range(40)]
    rows = others[:23] + [x] + others[23:]
    w44 = R.turns(R.FREQS, 44100)
    many = device_sums(eng, rows, [w44] * 23 + [w] + [w44] * 17)
    assert np.array_equal(many[23].view(np.uint64), alone[0].view(np.uint64))
    for lead in (1, 2, 3):                                               # 4, 8, 12 bytes past a 16-byte line
        mis = device_sums(eng, [x], [w], odd=False, lead=lead)
        assert np.array_equal(mis[0].view(np.uint64), alone[0].view(np.uint64)), lead
    again = device_sums(eng, [x], [w], odd=False, lead=0)
    assert np.array_equal(again.view(np.uint64), alone.view(np.uint64))


def _sums_raw(eng, flat_dev, off, length, w, max_len):
    """ira_mtf_sums through the bound library with the caller's max_len and a scratch of exactly
    ira_mtf_scratch_doubles(nseg, max_len, nf) doubles carved from the front of a larger NaN-filled buffer
    (Engine.mtf_sums always passes the true maximum length).  Returns (records, the buffer past the scratch)."""
    from audio_analysis_amd.engine import _ptr, check
    t = eng.torch
    nseg, nf = len(off), len(w)
    nsc = int(eng.lib.ira_mtf_scratch_doubles(nseg, max_len, nf))
    assert nsc == nseg * (-(-max_len // C)) * (2 * nf + 1)
    big = t.full((nsc + 64,), float("nan"), dtype=t.float64, device=eng.device)
    out = t.full((nseg * (2 * nf + 1),), float("nan"), dtype=t.float64, device=eng.device)
    d_off, d_len = eng.to_dev(np.asarray(off, np.int64)), eng.to_dev(np.asarray(length, np.int64))
    d_w = eng.to_dev(np.tile(np.asarray(w, np.float64), nseg))
    check(eng.lib.ira_mtf_sums(_ptr(flat_dev), _ptr(d_off), _ptr(d_len), _ptr(d_w), nseg, max_len, nf, _ptr(big), _ptr(out),
                               eng.stream), "ira_mtf_sums")
    return out.cpu().numpy().reshape(nseg, 2 * nf + 1), big[nsc:].cpu().numpy()


def test_fold_reads_only_the_records_max_len_paid_for():
    """A row longer than the max_len the caller stated comes out as if cut at max_len (the fold stops at the records the
    scratch holds for it), its neighbour is untouched and nothing past the scratch is read or written."""
    eng = _eng()
    rows = [_noise_row(61, 3 * C), _noise_row(62, C)]
    off = [1, 1 + 3 * C + 2]
    flat = np.full(off[1] + C + 8, 0.5, np.float32)
    for o, r in zip(off, rows):
        flat[o : o + r.size] = r
    x = eng.to_dev(flat)
    w = R.turns(R.FREQS, SR)
    both, past = _sums_raw(eng, x, off, [3 * C, C], w, 2 * C)
    cut, _ = _sums_raw(eng, x, off[:1], [2 * C], w, 2 * C)
    solo, _ = _sums_raw(eng, x, off[1:], [C], w, C)
    assert np.all(np.isfinite(both[0])) and np.array_equal(both[0].view(np.uint64), cut[0].view(np.uint64))
    assert np.array_equal(both[1].view(np.uint64), solo[0].view(np.uint64))
    assert np.all(np.isnan(past))


def test_closed_forms_on_the_device():
    eng = _eng()
    w = R.turns(R.FREQS, SR)
    rows = []
    for n, pos in ((1, 0), (5000, 4999), (C, C - 1), (C + 1, C), (100003, 77777), (3 * C, 2 * C + 1021)):
        x = np.zeros(n, np.float32)
        x[pos] = -0.3
        rows.append(x)
    got = device_sums(eng, rows, [w] * len(rows))
    worst = 0.0
    for i, x in enumerate(rows):
        assert got[i, 0] == float(np.max(np.abs(x)).astype(np.float64) ** 2)
        worst = max(worst, float(np.max(np.abs(R.m_of(got[i].astype(R.LD)) - 1.0))))
    print(f"unit impulses: max |m - 1| {worst:.3e}")
    assert worst <= 1e-15
    from audio_analysis_amd.analyse.sti import mtf_from_sums, sti_from_mtf
    sti, _ = sti_from_mtf(np.stack([mtf_from_sums(got[4])] * 7))
    assert abs(sti - 1.0) <= 1e-12
    # geometric rows: e = 0.25^j exactly, on every sample and on strides that cross chunks
    worst = 0.0
    for stride, count, fs in ((1, 100, 48000), (997, 100, 48000), (16385, 40, 44100)):
        x, a = R.geometric_row(stride, count)
        wg = R.turns(R.FREQS, fs)
        g = device_sums(eng, [x], [wg])
        worst = max(worst, float(np.max(np.abs(R.m_of(g[0].astype(R.LD)) - R.geometric_m(a, stride, count, wg)))))
        assert abs(g[0, 0] - (1.0 - a ** count) / (1.0 - a)) <= TOL_E * g[0, 0]
    print(f"geometric rows: max |m - closed form| {worst:.3e}")
    assert worst <= TOL_M


# ------------------------------------------------------------------------------------------------ the module
_LENS = [20000, 5000, C + 1, 37123, 8191, 48000, 2 * C + 5, 12345]


def _irs():
    from audio_analysis_amd.synth import synth_ir
    return [synth_ir(60 + i, i % 2, n, SR, rt60_seconds=0.3 + 0.25 * i) for i, n in enumerate(_LENS)]


@pytest.fixture(scope="module")
def module_run():
    """One 8-channel ragged batch through the module, with the device's own band signals brought back."""
    from audio_analysis_amd.analyse import energy as E
    from audio_analysis_amd.analyse import sti as S
    eng = _eng()
    chans = _irs()
    st = S.StiSettings()
    batch = eng.upload(chans)
    sig = E.band_signals_device(eng, batch, SR, st.bands)
    res = S.sti_results(S.sti_device(eng, batch, SR, st, band_signals=sig), SR, [f"c{i}" for i in range(len(chans))], st)
    direct = S.analyse_sti_batch(chans, SR, [f"c{i}" for i in range(len(chans))], st)
    return chans, res, direct, sig[1].cpu().numpy(), np.asarray(sig[2])


def test_module_vs_restatement_on_the_devices_band_signals(module_run):
    from audio_analysis_amd.analyse import sti as S
    chans, res, direct, yh, y_off = module_run
    w = R.turns(R.FREQS, SR)
    worst = worst_sti = 0.0
    for i, x in enumerate(chans):
        assert res[i].status == S.STATUS_SHORT and res[i].band_names == S.BAND_NAMES
        m = np.array([R.mtf(yh[y_off[i, k] : y_off[i, k] + x.size], w) for k in range(7)])
        got = np.array(res[i].mtf)
        assert got.shape == (7, 14)
        worst = max(worst, float(np.max(np.abs(got - m))))
        s, mti = R.sti(m)
        worst_sti = max(worst_sti, abs(res[i].sti - s), float(np.max(np.abs(np.array(res[i].mti) - np.array(mti)))))
        assert res[i].rating == S.rating_word(res[i].sti)
        # the batch entry point builds its own band signals from its own upload of the same samples
        assert direct[i].status == res[i].status and _same(direct[i], res[i])
    print(f"module, 8 channels x 7 bands x 14: max |m - restatement| {worst:.3e}, max |STI, MTI - restatement| {worst_sti:.3e}")
    assert worst <= TOL_M
    # TI has slope 10 / (30 ln 10) / (m (1 - m)) <= 4.9 inside the clip range (0.0307 <= m <= 0.9693) and 0 outside: 1e-10
    # of m is 5e-10 of MTI; the square roots of STI steepen that where an MTI is small, for which a factor 100 is left
    assert worst_sti <= 5e-8


def test_module_vs_oracle_filter_bank(module_run):
    """The same batch against the restatement applied to the oracle's float64 bank rounded to float32.  The bound follows
    from the band signals' actual difference: with S = sum e cis, |S| and E each move by at most D = sum |e_dev - e_ref|,
    so m = |S| / E moves by at most (1 + m) D / E <= 2 D / E (E the smaller of the two), plus the kernel's own 1e-10."""
    chans, res, _, yh, y_off = module_run
    w = R.turns(R.FREQS, SR)
    worst = worst_bound = 0.0
    for i, x in enumerate(chans):
        ob = R.oracle_band_signals(x, SR)
        assert tuple(n for n, _ in ob) == res[i].band_names
        for k, (name, yref) in enumerate(ob):
            ydev = yh[y_off[i, k] : y_off[i, k] + x.size]
            e_dev, e_ref = ydev.astype(np.float64) ** 2, yref.astype(np.float64) ** 2
            bound = 2.0 * float(np.sum(np.abs(e_dev - e_ref))) / min(float(e_dev.sum()), float(e_ref.sum())) + TOL_M
            err = float(np.max(np.abs(np.array(res[i].mtf[k]) - R.mtf(yref, w))))
            assert err <= bound, (i, name, err, bound)
            worst, worst_bound = max(worst, err), max(worst_bound, bound)
    print(f"module vs oracle bank: max |m - restatement on the oracle's bands| {worst:.3e} (largest bound {worst_bound:.3e})")
    assert worst_bound < 1e-3                                             # the bound itself is not vacuous


# The restatement alone (oracle bank + sti_ref on a CPU, seed 2024) is off Schroeder's prediction by 0.006848 (T = 1.0 s)
# and 0.006207 (T = 2.5 s): the carrier's own fluctuation in the narrow low bands.  The test allows twice that.
@pytest.mark.parametrize("t_seconds,seconds,cpu_deviation", [(1.0, 3.0, 0.006848), (2.5, 4.0, 0.006207)])
def test_schroeder_prediction_for_decaying_noise(t_seconds, seconds, cpu_deviation):
    from audio_analysis_amd.analyse import sti as S
    x = R.decaying_noise(2024, t_seconds, seconds, SR)
    res = S.analyse_sti_batch([x], SR, ["noise"])[0]
    want = R.schroeder_sti(t_seconds)
    print(f"T = {t_seconds} s: STI {res.sti:.6f}, Schroeder {want:.6f}, deviation {abs(res.sti - want):.6f}")
    assert res.status == 0
    assert abs(res.sti - want) <= 2.0 * cpu_deviation
    assert res.rating == ("fair" if t_seconds == 1.0 else "poor")


def test_status_rows_leave_the_rest_of_the_batch_intact():
    from audio_analysis_amd.analyse import sti as S
    from audio_analysis_amd.synth import synth_ir
    n = 80000                                                             # > fs / 0.63 = 76190.5 samples
    good = synth_ir(3, 0, n, SR, rt60_seconds=0.9)
    silent = np.zeros(n, np.float32)
    nan = good.copy()
    nan[5000] = np.nan
    inf = good.copy()
    inf[7000] = np.inf
    short = synth_ir(4, 0, 76190, SR, rt60_seconds=0.5)
    enough = synth_ir(4, 0, 76191, SR, rt60_seconds=0.5)
    chans = [good, silent, nan, short, inf, enough, good, np.zeros(9000, np.float32)]
    res = S.analyse_sti_batch(chans, SR, [str(i) for i in range(len(chans))])
    assert [r.status for r in res] == [0, 1, 2, 4, 2, 0, 0, 5]
    alone = S.analyse_sti_batch([good], SR, ["g"])[0]
    assert res[0].mtf == res[6].mtf and res[0].sti == res[6].sti
    assert _same(res[0], alone)
    for i in (1, 2, 4, 7):
        assert math.isnan(res[i].sti) and res[i].rating == "NA"
        assert all(math.isnan(v) for v in res[i].mti) and all(math.isnan(v) for row in res[i].mtf for v in row)
    for i in (0, 3, 5):
        assert 0.0 < res[i].sti < 1.0 and all(0.0 <= v <= 1.0 for row in res[i].mtf for v in row)
    # noise and levels reach the result: each lowers every m by its factor
    st = S.StiSettings(snr_db=6.0, band_levels_db=(70.0, 68.0, 66.0, 64.0, 62.0, 60.0, 58.0))
    adj = S.analyse_sti_batch([good], SR, ["g"], st)[0]
    want = R.adjust(np.array(alone.mtf), [6.0] * 7, list(st.band_levels_db))
    assert np.max(np.abs(np.array(adj.mtf) - want)) <= 1e-12 and adj.sti < alone.sti
    assert abs(adj.sti - R.sti(want)[0]) <= 1e-12


# ------------------------------------------------------------------------------------------------ entry points, command line
def _run_cli(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.sti", *map(str, args)], capture_output=True, text=True,
                       cwd=str(REPO), env=env, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_wav_bundle_entry_points_and_cli(tmp_path):
    from audio_analysis_amd.analyse import sti as S
    from audio_analysis_amd.synth import synth_ir
    n = 2 * SR
    taps, stereo = {}, {}
    for k, name in enumerate(["hall", "plate"]):
        st = np.stack([synth_ir(50 + k, 0, n, SR, rt60_seconds=0.8), synth_ir(50 + k, 1, n, SR, rt60_seconds=1.4)], axis=1)
        taps[name] = O.recorder_wav_bytes(st.reshape(-1), SR)
        stereo[name] = st
    wav = tmp_path / "hall.wav"
    wav.write_bytes(taps["hall"])
    one = S.analyse_sti_from_wav_file(wav)
    assert [r.channel_name for r in one] == ["left", "right"] and all(r.status == 0 for r in one)
    assert one[0].sti > one[1].sti                                        # the longer tail transmits less
    mono = S.analyse_sti_from_wav_file(wav, S.StiSettings(use_mono_downmix_for_stereo=True))
    assert [r.channel_name for r in mono] == ["mono"]
    pcm = O.wav_pcm16_payload(taps["hall"])[1].astype(np.float32) / 32768.0
    down = S.analyse_sti_batch([0.5 * (pcm[:, 0] + pcm[:, 1])], SR, ["m"])[0]
    assert np.max(np.abs(np.array(mono[0].mtf) - np.array(down.mtf))) <= 1e-6
    out = _run_cli(["--input", wav, "--snr-db", "12", "--json", tmp_path / "w.json"])
    api = S.analyse_sti_files([wav], S.StiSettings(snr_db=12.0))
    assert out == S.summarise_sti_text(api)
    assert [r.channel_name for r in api] == ["hall.wav:left", "hall.wav:right"]
    assert "STI: " in out and "8000Hz" in out and "12.5Hz" in out
    assert all(a.sti < b.sti for a, b in zip(api, one))                   # the noise lowers the index
    back = S.sti_results_from_json(json.loads((tmp_path / "w.json").read_text()))
    assert back == api and S.summarise_sti_text(back) == out
    # bundle: meta.json + taps/<name>.wav, read through the native ingest
    root = tmp_path / "bundle"
    (root / "taps").mkdir(parents=True)
    for name, blob in taps.items():
        (root / "taps" / f"{name}.wav").write_bytes(blob)
    (root / "meta.json").write_text(O.recorder_meta_json(SR, n, list(taps)))
    levels = ["70", "68", "66", "64", "62", "60", "58"]
    out = _run_cli(["--bundle", root, "--mono", "--levels-db", *levels])
    st_b = S.StiSettings(band_levels_db=tuple(float(v) for v in levels), use_mono_downmix_for_stereo=True)
    api = S.analyse_sti_bundle(root, st_b)
    assert out == S.summarise_sti_text(api)
    assert [r.channel_name for r in api] == ["hall:mono", "plate:mono"]
    wav2 = tmp_path / "plate.wav"
    wav2.write_bytes(taps["plate"])
    ref = S.analyse_sti_files([wav, wav2], st_b)
    for a, b in zip(api, ref):                                            # the native ingest's downmix is the channel policy's
        assert a.status == b.status == 0 and _same(a, b)
