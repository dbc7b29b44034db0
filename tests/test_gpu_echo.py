"""
The Dietsch-Kraak echo criterion on the device (ira_echo_criterion, audio_analysis_amd.analyse.echo) against the float64
NumPy restatement of tests/echo_ref.py; band signals against the oracle's float64 filter bank.

Every comparison uses, per segment, tol = (8 M + 100) 2^-53 max(ts) / (D / fs) (echo_ref.tolerance): the worst-case rounding
of two sums of M non-negative terms on each side, through the ratio and the lagged difference, plus 16 ulp for pow --
about 1e-9 on these inputs against an observed 1e-13 between a float64 and a long-double restatement: a bound, not a fit.
"""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import echo_ref as R
from oracle import ira_oracle as O

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
SR = 48000
CHUNK = 4096                      # engine.ECHO_CHUNK: samples per workgroup, counted from the onset
BIG = float(1 << 31)
N_SPEECH, N_MUSIC = 2.0 / 3.0, 1.0


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def prm(n, d, fs=SR, guard=0, mmax=BIG, step=48, t10=0.9, t50=1.0):
    return [n, float(d), float(guard), float(mmax), float(step), t10, t50, float(fs)]


def run(eng, chans, params, seg_chan, seg_param, onset_db=-20.0):
    """Engine level: one batch, one launch; segment j reads channel seg_chan[j] itself with parameter set seg_param[j]."""
    b = eng.upload([np.asarray(c, dtype=np.float32) for c in chans])
    on, _, _ = eng.onset_index(b, 10.0 ** (onset_db / 10.0))
    seg_chan = np.asarray(seg_chan, dtype=np.int32)
    rec, curve = eng.echo_criterion(b.x, b.off[seg_chan], b.length[seg_chan], seg_chan, on,
                                    np.asarray(params, dtype=np.float64), np.asarray(seg_param, dtype=np.int32))
    return on.cpu().numpy(), rec.cpu().numpy(), curve.cpu().numpy()


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32))).astype(np.float64)


def check_segment(y, o, p, rec, curve_row, what=""):
    """The issue's conditions for one segment: signal y (float32), onset o, parameter set p, the device's record and curve
    row.  Returns the reference EK (None for a segment without samples)."""
    n, d, guard, cap, step, t10, t50, fs = p[0], int(p[1]), int(p[2]), int(p[3]), int(p[4]), p[5], p[6], p[7]
    m = min(len(y) - o - guard, cap)
    assert rec[6] == m, (what, rec[6], m)
    if m <= 0:
        assert np.isnan(rec[0]) and rec[1] == -1 and rec[5] == 0.0
        assert np.all(np.isnan(curve_row))
        return None
    ek, ts, w, v = R.ek_curve(y, o, n, d, fs, m)
    tol = R.tolerance(m, ts, d, fs)
    print(f"{what}: M {m} D {d} n {n:.3f} tol {tol:.3e} |ek_max - ref| {abs(rec[0] - ek.max()):.3e} "
          f"|ts_end - ref| {abs(rec[4] - ts[-1]):.3e} (bound {tol * d / fs:.3e})")
    assert abs(rec[0] - ek.max()) <= tol, (what, rec[0], ek.max(), tol)
    assert abs(rec[4] - ts[-1]) <= tol * d / fs, (what, rec[4], ts[-1])
    i = int(rec[1])
    assert rec[1] == i and 0 <= i < m and ek[i] >= ek.max() - 2.0 * tol, (what, i, int(np.argmax(ek)))
    for r, thr in ((rec[2], t10), (rec[3], t50)):
        i = int(r)
        assert r == i and -1 <= i < m, (what, r)
        if i >= 0:
            assert ek[i] >= thr - tol, (what, i, ek[i], thr)
        assert np.all(ek[: i if i >= 0 else m] < thr + tol), (what, i, thr, R.first_at_or_above(ek, thr))
    # the sums themselves: M terms, one rounding each, and pow
    assert abs(rec[5] - w[-1]) <= (2.0 * m + 32.0) * 2.0 ** -53 * w[-1], (what, rec[5], w[-1])
    assert abs(rec[7] - v[-1]) <= (2.0 * m + 32.0) * 2.0 ** -53 * v[-1], (what, rec[7], v[-1])
    if step > 0:
        want = R.step_max(ek, step)
        got = curve_row[: want.size]
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        assert np.all(err <= tol + ulp32(want)), (what, int(np.argmax(err)), float(err.max()))
        assert np.all(np.isnan(curve_row[want.size:])), what
    else:
        assert np.all(np.isnan(curve_row)), what
    return ek


# ------------------------------------------------------------------------------------------------ closed forms
def test_closed_forms_on_the_device():
    """Constant magnitude: EK[m] = m / (2 D) for m < D and 0.5 after, for any n.  A unit impulse at 0 and g at sample k:
    EK = k g^n / ((1 + g^n) D) for k <= m < k + D, 0 elsewhere -- there ts is constant, so the plateau is exact and the
    first index of the maximum is k itself.  k = 4000 puts the plateau across a chunk boundary (the halo)."""
    eng = _eng()
    rng = np.random.default_rng(2)
    const = (0.37 * rng.choice([-1.0, 1.0], 9000)).astype(np.float32)
    k = 4000
    imp = [np.zeros(10000, np.float32) for _ in range(2)]
    for y, g in zip(imp, (0.5, 1.0)):
        y[0], y[k] = 1.0, g
    params = [prm(N_SPEECH, 432, t10=0.25, t50=0.4), prm(N_MUSIC, 672, t10=0.25, t50=0.4), prm(2.0, 432, t10=0.25, t50=0.4),
              prm(0.5, 100, t10=0.25, t50=0.4)]
    chans = [const] + imp
    seg_chan = [0, 0, 0, 0, 1, 1, 2, 2]
    seg_param = [0, 1, 2, 3, 0, 1, 0, 1]
    on, rec, curve = run(eng, chans, params, seg_chan, seg_param)
    assert list(on) == [0, 0, 0]
    for j, (c, p) in enumerate(zip(seg_chan, seg_param)):
        ek = check_segment(chans[c], 0, params[p], rec[j], curve[j], f"closed form {j}")
        n, d = params[p][0], int(params[p][1])
        tol = (8.0 * ek.size + 100.0) * 2.0 ** -53 * (ek.size / (2.0 * SR)) / (d / SR)
        if c == 0:
            m = np.arange(ek.size)
            want = np.where(m < d, m / (2.0 * d), 0.5)
            assert abs(rec[j][0] - 0.5) <= tol
            assert rec[j][2] in (math.ceil(0.25 * 2 * d) - 1, math.ceil(0.25 * 2 * d), math.ceil(0.25 * 2 * d) + 1)
        else:
            gn = float(chans[c][k]) ** n
            plateau = k * gn / ((1.0 + gn) * d)
            want = np.zeros(ek.size)
            want[k : k + d] = plateau
            assert abs(rec[j][0] - plateau) <= tol and rec[j][1] == k
            assert rec[j][2] == (k if plateau >= 0.25 else -1) and rec[j][3] == (k if plateau >= 0.4 else -1)
        sm = R.step_max(want, 48)
        assert np.all(np.abs(curve[j][: sm.size].astype(np.float64) - sm) <= tol + ulp32(sm))


# ------------------------------------------------------------------------------------------------ broadband, ragged
def _with_copy(x, delay, gain=1.5):
    y = x.astype(np.float64).copy()
    y[delay:] += gain * x[: x.size - delay].astype(np.float64)
    return y.astype(np.float32)


def _place_maximum(target, n, d, guard):
    """A response plus a delayed copy of itself at gain 1.5 whose reference EK has its maximum exactly at sample `target`
    after the onset: the delay is moved by the miss until it hits (host arithmetic only; a few seeds in case one oscillates)."""
    from audio_analysis_amd.synth import synth_ir
    for seed in range(60, 70):
        x = synth_ir(seed, 0, 16000, SR, rt60_seconds=0.25, pre_delay=37 + seed % 3)
        delay = target - 500
        for _ in range(12):
            y = _with_copy(x, delay)
            o = R.onset(y)
            ek = R.ek_curve(y, o, n, d, SR, y.size - o - guard)[0]
            a = int(np.argmax(ek))
            if a == target:
                top = np.sort(ek)[-2:]
                if top[1] - top[0] > 1e-7:                   # far more than tol: the device must name this very index
                    return y, o
                break
            delay += target - a
    raise AssertionError(f"no input with its maximum at {target}")


def test_broadband_ragged_batch_vs_restatement():
    """Criteria without bands through the public device function.  Onsets that are no multiples of 4 samples; M equal to a
    chunk multiple and +-1; M = D + 1 (analysed) and M = D (status 2); the EK maximum at the last sample of a chunk, the
    first sample of a chunk and within D of a chunk start."""
    from audio_analysis_amd.analyse import echo as E
    from audio_analysis_amd.synth import synth_ir
    eng = _eng()
    speech = E.EchoCriterion("speech", N_SPEECH, 9.0, None, 0.9, 1.0)
    music = E.EchoCriterion("music", N_MUSIC, 14.0, None, 1.5, 1.8)
    guard = 2400

    def cut(x, m):                                           # the channel cut so that L - G = m
        return x[: R.onset(x) + guard + m].copy()

    long_ = [synth_ir(40 + i, 0, 30000, SR, rt60_seconds=0.3 + 0.1 * i, pre_delay=[37, 101, 258, 3][i]) for i in range(4)]
    chans = [cut(long_[0], 2 * CHUNK), cut(long_[1], 2 * CHUNK - 1), cut(long_[2], 2 * CHUNK + 1), long_[3]]
    for target in (CHUNK - 1, CHUNK, CHUNK + 100, 2 * CHUNK - 1):
        y, _ = _place_maximum(target, N_SPEECH, 432, guard)
        chans.append(y)
    st = E.EchoCriterionSettings(criteria=(speech, music), max_tau_ms=None)
    b = eng.upload(chans)
    res = E.echo_criterion_device(eng, b, SR, st)
    out = E.echo_criterion_results(res, SR, [str(i) for i in range(len(chans))])
    onsets = [R.onset(x) for x in chans]
    assert any(o % 4 for o in onsets) and list(res.onset) == onsets
    assert [int(v) for v in res.records[:3, 0, 6]] == [2 * CHUNK, 2 * CHUNK - 1, 2 * CHUNK + 1]
    for i, x in enumerate(chans):
        assert out[i].status == 0
        for k, c in enumerate(st.criteria):
            p = E.criterion_params(c, SR, st)
            ek = check_segment(x, onsets[i], p, res.records[i, k], res.curve[i, k], f"ragged {i} {c.name}")
            v = out[i].values_by_name[c.name]
            assert v.ek_max == res.records[i, k, 0] and v.tau_max_seconds == res.records[i, k, 1] / SR
            assert v.rating == R.rating(v.ek_max, c.threshold_10, c.threshold_50) and v.build_up_seconds == res.records[i, k, 4]
            assert len(v.curve) == -(-ek.size // 48)
    for i, target in zip(range(4, 8), (CHUNK - 1, CHUNK, CHUNK + 100, 2 * CHUNK - 1)):
        assert res.records[i, 0, 1] == target, (i, res.records[i, 0, 1], target)
    # M = D + 1 is analysed, M = D is too short (one criterion per run: the two have different D)
    for c, d in ((speech, 432), (music, 672)):
        st1 = E.EchoCriterionSettings(criteria=(c,), max_tau_ms=None)
        pair = [cut(long_[0], d + 1), cut(long_[0], d), long_[3]]
        r1 = E.echo_criterion_device(eng, eng.upload(pair), SR, st1)
        o1 = E.echo_criterion_results(r1, SR, ["plus1", "exact", "good"])
        assert [r.status for r in o1] == [0, E.STATUS_TOO_SHORT, 0] and list(r1.records[:2, 0, 6]) == [d + 1, d]
        check_segment(pair[0], R.onset(pair[0]), E.criterion_params(c, SR, st1), r1.records[0, 0], r1.curve[0, 0], f"M = D + 1 {c.name}")
        assert o1[1].values_by_name[c.name].rating == "NA" and math.isnan(o1[1].values_by_name[c.name].ek_max)
        assert o1[2].values_by_name[c.name].ek_max == out[3].values_by_name[c.name].ek_max      # bit for bit, another batch


def test_long_channel_more_chunks_than_a_wave_has_lanes():
    """480 000 samples with max_tau_ms = None: 117 chunks, so the carry scan and the fold run more than one round of 64."""
    from audio_analysis_amd.analyse import echo as E
    from audio_analysis_amd.synth import synth_ir
    eng = _eng()
    x = _with_copy(synth_ir(45, 0, 480000, SR, rt60_seconds=1.4, pre_delay=1001), 300007, gain=0.9)
    short = synth_ir(46, 0, 9000, SR, rt60_seconds=0.2)
    st = E.EchoCriterionSettings(criteria=(E.EchoCriterion("speech", N_SPEECH, 9.0, None, 0.9, 1.0),
                                           E.EchoCriterion("music", N_MUSIC, 14.0, None, 1.5, 1.8)), max_tau_ms=None)
    res = E.echo_criterion_device(eng, eng.upload([x, short]), SR, st)
    assert res.records[0, 0, 6] > 64 * CHUNK
    for i, y in enumerate((x, short)):
        for k, c in enumerate(st.criteria):
            check_segment(y, R.onset(y), E.criterion_params(c, SR, st), res.records[i, k], res.curve[i, k], f"long {i} {c.name}")
    assert res.records[0, 0, 1] > 64 * CHUNK                  # the late copy holds the maximum: found past the first round


# ------------------------------------------------------------------------------------------------ bands
EDGES = ((700.0, 1400.0), (700.0, 2800.0))


def _oracle_bands(x, sr, edges=EDGES):
    n = x.size
    f = np.fft.rfftfreq(n, d=1.0 / float(sr)).astype(np.float32)
    spec = np.fft.rfft(x.astype(np.float64))
    out = []
    for lo, hi in edges:
        m = O.band_mask(f, dict(kind="bandpass", low_edge_hz=lo, high_edge_hz=hi), 1.0 / 6.0, 0.5 * float(sr))
        out.append(np.fft.irfft(spec * m.astype(np.float64), n=n))
    return out


def test_kernel_alone_on_uploaded_oracle_band_signals():
    """The oracle's float64 band signals (700-1400 Hz, 700-2800 Hz), rounded to float32 and uploaded as they are; both
    criteria in one launch, every band segment starting at the broadband channel's onset."""
    from audio_analysis_amd.analyse import echo as E
    from audio_analysis_amd.synth import synth_ir
    eng = _eng()
    x = _with_copy(synth_ir(11, 0, 72000, SR, rt60_seconds=0.9), 7200)
    ys = [y.astype(np.float32) for y in _oracle_bands(x, SR)]
    b = eng.upload([x] + ys)
    on, _, _ = eng.onset_index(b, 0.01)
    st = E.EchoCriterionSettings()
    params = [E.criterion_params(c, SR, st) for c in st.criteria]
    rec, curve = eng.echo_criterion(b.x, b.off[1:], b.length[1:], np.zeros(2, np.int32), on, np.asarray(params),
                                    np.arange(2, dtype=np.int32))
    rec, curve = rec.cpu().numpy(), curve.cpu().numpy()
    o = R.onset(x)
    assert int(on.cpu().numpy()[0]) == o
    for k in range(2):
        check_segment(ys[k], o, params[k], rec[k], curve[k], f"oracle band {EDGES[k]}")


def _band_inputs():
    from audio_analysis_amd.synth import synth_ir
    return [synth_ir(70, 0, 48000, SR, rt60_seconds=0.4), synth_ir(71, 0, 37123, SR, rt60_seconds=0.6),
            synth_ir(72, 0, 48000, SR, rt60_seconds=0.35)]


def test_band_path_vs_oracle_filter_bank():
    """Full band path (filter bank on the device + the kernel) on synthetic responses plus a copy of themselves 150 ms later at
    gain 1.5, max_tau_ms = 400.  The device's band signals differ from the oracle's float64 ones by delta <= 1e-6 of the peak
    (the existing band tolerance, asserted); delta is propagated by interval arithmetic (echo_ref.ek_interval) and every
    device EK_max and curve point must lie inside the interval widened by tol.  The interval's half-width must stay <= 0.02,
    so that the test cannot pass vacuously.  The speech criterion must rate "audible" on all three; the music criterion's
    reference EK_max for rt60 = 0.6 s lies between its two thresholds (1.5 / 1.8), so its rating is compared with the
    reference's whenever the interval does not straddle a threshold."""
    from audio_analysis_amd.analyse import echo as E
    from audio_analysis_amd.analyse.rt60bands import Rt60BandsAnalysisSettings, band_signals_device
    eng = _eng()
    chans = [_with_copy(x, 7200) for x in _band_inputs()]
    st = E.EchoCriterionSettings(max_tau_ms=400.0)
    names = ["a", "b", "c"]
    res = E.analyse_echo_criterion_batch(chans, SR, names, st)
    batch = eng.upload(chans)
    bands, rows = E.criterion_bands(st.criteria)
    assert rows == [1, 2]
    _, y, y_off = band_signals_device(eng, batch, SR, Rt60BandsAnalysisSettings(transition_width_octaves=1.0 / 6.0), bands=bands)
    yh = y.cpu().numpy()
    rec = E.echo_criterion_device(eng, batch, SR, st)
    for i, x in enumerate(chans):
        o = R.onset(x)
        assert res[i].status == 0 and res[i].onset_samples == o
        for k, (c, yref) in enumerate(zip(st.criteria, _oracle_bands(x, SR))):
            ydev = yh[y_off[i, k] : y_off[i, k] + x.size]
            delta = float(np.max(np.abs(ydev.astype(np.float64) - yref)))
            peak = float(np.max(np.abs(x)))
            assert delta <= 1e-6 * peak, (c.name, delta)
            p = E.criterion_params(c, SR, st)
            d, m = int(p[1]), int(rec.records[i, k, 6])
            assert m == min(x.size - o - int(p[2]), int(p[3]))
            ek, ts, _, _ = R.ek_curve(yref.astype(np.float32), o, c.exponent, d, SR, m)
            tol = R.tolerance(m, ts, d, SR)
            lo, hi = R.ek_interval(yref, delta, o, c.exponent, d, SR, m)
            slo, shi = R.step_max(lo, 48).astype(np.float64), R.step_max(hi, 48).astype(np.float64)
            half = max(float(np.max(shi - slo)), float(hi.max() - lo.max())) / 2.0
            v = res[i].values_by_name[c.name]
            print(f"band path {i} {c.name}: delta {delta / peak:.2e} of the peak, half-width {half:.2e}, tol {tol:.2e}, "
                  f"EK_max {v.ek_max:.4f} (reference {ek.max():.4f}) at {1000.0 * v.tau_max_seconds:.1f} ms, {v.rating}")
            assert half <= 0.02, (c.name, half)
            assert lo.max() - tol <= v.ek_max <= hi.max() + tol, (c.name, v.ek_max, lo.max(), hi.max())
            cur = np.asarray(v.curve, dtype=np.float64)
            assert cur.size == slo.size
            assert np.all(cur >= slo - tol - ulp32(slo)) and np.all(cur <= shi + tol + ulp32(shi)), c.name
            assert 0.150 <= v.tau_max_seconds <= 0.175
            straddles = any(lo.max() - tol < t <= hi.max() + tol for t in (c.threshold_10, c.threshold_50))
            if not straddles:
                assert v.rating == R.rating(float(ek.max()), c.threshold_10, c.threshold_50)
        assert res[i].values_by_name["speech"].rating == "audible"
    assert res[0].values_by_name["music"].rating == "audible" and res[2].values_by_name["music"].rating == "audible"
    # the same responses without the copy: no echo
    plain = E.analyse_echo_criterion_batch(_band_inputs(), SR, names, st)
    for r in plain:
        assert r.status == 0 and [v.rating for v in r.values_by_name.values()] == ["inaudible", "inaudible"]
        assert all(0.4 <= v.ek_max <= 0.7 for v in r.values_by_name.values())


def test_end_guard_keeps_the_wrapped_pre_ringing_out():
    """A 2 s response with rt60 = 0.3 s and max_tau_ms = None: with end_guard_ms = 50 the speech rating is "inaudible" (the
    band filter's pre-ringing of the direct sound wraps to the end of the file and is left out), and everything in front of
    M matches a run with an explicit smaller max_tau_ms bit for bit: the sums are causal."""
    from audio_analysis_amd.analyse import echo as E
    from audio_analysis_amd.synth import synth_ir
    x = synth_ir(80, 0, 96000, SR, rt60_seconds=0.3)
    whole = E.analyse_echo_criterion_batch([x], SR, ["x"], E.EchoCriterionSettings(max_tau_ms=None))[0]
    part = E.analyse_echo_criterion_batch([x], SR, ["x"], E.EchoCriterionSettings(max_tau_ms=1000.0))[0]
    assert whole.status == 0 and whole.values_by_name["speech"].rating == "inaudible"
    for name in ("speech", "music"):
        w, p = whole.values_by_name[name], part.values_by_name[name]
        full = 48001 // 48                                   # steps that end in front of the shorter run's M
        assert len(w.curve) == -(-(96000 - whole.onset_samples - 2400) // 48) and len(p.curve) == full + 1
        assert np.array_equal(np.asarray(w.curve[:full], np.float32).view(np.uint32), np.asarray(p.curve[:full], np.float32).view(np.uint32))
        if w.tau_max_seconds * SR < 48001:
            assert (w.ek_max, w.tau_max_seconds) == (p.ek_max, p.tau_max_seconds)


# ------------------------------------------------------------------------------------------------ determinism, rates
def test_bit_identical_whatever_the_batch():
    from audio_analysis_amd.engine import Engine
    from audio_analysis_amd.synth import synth_ir
    eng = _eng()
    x = _with_copy(synth_ir(7, 0, 250001, SR, rt60_seconds=1.1, pre_delay=333), 100003, gain=4.0)
    params = [prm(N_SPEECH, 432, guard=2400), prm(N_MUSIC, 672, guard=2400, t10=1.5, t50=1.8)]
    _, alone, alone_c = run(eng, [x], params, [0, 0], [0, 1])
    assert alone[0, 6] == 250001 - R.onset(x) - 2400 and np.isfinite(alone[:, :6]).all()
    bits = lambda a, c: (a.view(np.uint64), c[:, : alone_c.shape[1]].view(np.uint32))    # noqa: E731
    rng = np.random.default_rng(3)
    others = [synth_ir(100 + k, 0, int(rng.integers(4000, 60000)), SR) for k in range(299)]
    chans = others[:200] + [x] + others[200:]
    seg_chan = np.repeat(np.arange(300), 2)
    _, many, many_c = run(eng, chans, params, seg_chan, np.tile([0, 1], 300))
    assert all(np.array_equal(g, w) for g, w in zip(bits(many[400:402], many_c[400:402]), bits(alone, alone_c)))
    for shift in (1, 2, 3):                                  # the channel starts 4, 8, 12 bytes past a 16-byte line
        _, mis, mis_c = run(eng, [np.zeros(shift, np.float32) + 0.25, x], params, [1, 1], [0, 1])
        assert all(np.array_equal(g, w) for g, w in zip(bits(mis, mis_c), bits(alone, alone_c))), shift
    # the float64 stash of the first pass read back by the second: the same results to the bit
    eng.echo_stash = True
    try:
        _, st, st_c = run(eng, [x], params, [0, 0], [0, 1])
    finally:
        eng.echo_stash = Engine.echo_stash
    assert all(np.array_equal(g, w) for g, w in zip(bits(st, st_c), bits(alone, alone_c)))


def test_mixed_sample_rates_in_one_launch():
    from audio_analysis_amd.synth import synth_ir
    eng = _eng()
    rates = [44100, 48000, 44100, 48000]
    chans = [_with_copy(synth_ir(30 + i, 0, 30000 + 999 * i, fs, rt60_seconds=0.3 + 0.1 * i), 6000 + 100 * i)
             for i, fs in enumerate(rates)]
    params, seg_chan, seg_param = [], [], []
    for fs in (44100, 48000):
        params.append(prm(N_SPEECH, R.lag(9.0, fs), fs, R.guard(50.0, fs), R.mmax(500.0, fs), max(1, round(fs / 1000.0))))
        params.append(prm(N_MUSIC, R.lag(14.0, fs), fs, R.guard(50.0, fs), R.mmax(500.0, fs), max(1, round(fs / 1000.0)), 1.5, 1.8))
    assert [p[1] for p in params] == [397.0, 617.0, 432.0, 672.0] and [p[4] for p in params] == [44.0, 44.0, 48.0, 48.0]
    for i, fs in enumerate(rates):
        seg_chan += [i, i]
        seg_param += [0, 1] if fs == 44100 else [2, 3]
    on, rec, curve = run(eng, chans, params, seg_chan, seg_param)
    for j, (c, p) in enumerate(zip(seg_chan, seg_param)):
        o = R.onset(chans[c])
        assert on[c] == o
        check_segment(chans[c], o, params[p], rec[j], curve[j], f"mixed rates {j}")


# ------------------------------------------------------------------------------------------------ degenerate channels
def test_degenerate_channels_keep_the_rest_of_the_batch():
    from audio_analysis_amd.analyse import echo as E
    from audio_analysis_amd.synth import synth_ir
    good = _with_copy(synth_ir(3, 0, 30000, SR, rt60_seconds=0.4), 7200)
    silent = np.zeros(9000, np.float32)
    nan = good.copy()
    nan[5000] = np.nan
    short = good[:2500].copy()                               # L - G < D
    chans = [good, silent, nan, short, good]
    names = [str(i) for i in range(len(chans))]
    wide = (E.EchoCriterion("speech", N_SPEECH, 9.0, None, 0.9, 1.0), E.EchoCriterion("music", N_MUSIC, 14.0, None, 1.5, 1.8))
    for crit in (wide, (E.SPEECH, E.MUSIC)):
        st = E.EchoCriterionSettings(criteria=crit)
        res = E.analyse_echo_criterion_batch(chans, SR, names, st)
        alone = E.analyse_echo_criterion_batch([good], SR, ["g"], st)[0]
        assert [r.status for r in res] == [0, E.STATUS_SILENT, E.STATUS_NON_FINITE, E.STATUS_TOO_SHORT, 0]
        for i in (0, 4):
            for name, v in res[i].values_by_name.items():
                a = alone.values_by_name[name]
                assert v.rating in E.RATINGS and math.isfinite(v.ek_max) and all(math.isfinite(c) for c in v.curve)
                assert (v.ek_max, v.tau_max_seconds, v.build_up_seconds, v.rating) == (a.ek_max, a.tau_max_seconds, a.build_up_seconds, a.rating)
                assert np.array_equal(np.asarray(v.curve, np.float32).view(np.uint32), np.asarray(a.curve, np.float32).view(np.uint32))
        for i in (1, 2, 3):
            for v in res[i].values_by_name.values():
                assert v.rating == "NA" and all(math.isnan(t) for t in (v.ek_max, v.tau_max_seconds, v.first_tau_10_seconds,
                                                                      v.first_tau_50_seconds, v.build_up_seconds))
                assert all(math.isnan(c) for c in v.curve)
        text = E.summarise_echo_criterion_text(res)
        assert "Status: 1 (silent)" in text and "Status: 4 (non-finite)" in text and "Status: 2 (too short)" in text


# ------------------------------------------------------------------------------------------------ command line
def _run_cli(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.echo", *map(str, args)], capture_output=True, text=True,
                       cwd=str(REPO), env=env, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_cli_on_wav_and_bundle(tmp_path):
    from audio_analysis_amd.analyse import echo as E
    from audio_analysis_amd.synth import synth_ir
    n = SR
    st = np.stack([_with_copy(synth_ir(50, 0, n, SR, rt60_seconds=0.4), 7200), synth_ir(50, 1, n, SR, rt60_seconds=0.5)], axis=1)
    wav = tmp_path / "hall.wav"
    wav.write_bytes(O.recorder_wav_bytes(st.reshape(-1), SR))
    out = _run_cli(["--input", wav, "--max-tau-ms", "400", "--json", tmp_path / "w.json"])
    settings = E.EchoCriterionSettings(max_tau_ms=400.0)
    api = E.analyse_echo_criterion_files([wav], settings)
    assert out == E.summarise_echo_criterion_text(api)
    assert [r.channel_name for r in api] == ["hall.wav:left", "hall.wav:right"]
    assert api[0].values_by_name["speech"].rating == "audible" and api[1].values_by_name["speech"].rating == "inaudible"
    assert "Criterion  EK_max  tau_max_ms" in out and "audible" in out
    doc = json.loads((tmp_path / "w.json").read_text())
    back = E.echo_results_from_json(doc)
    assert E.summarise_echo_criterion_text(back) == out and E.echo_results_to_json(back) == doc
    assert back[0].values_by_name["music"] == api[0].values_by_name["music"] and len(back[0].values_by_name["music"].curve) > 300
    # bundle: meta.json + taps/<name>.wav, read through the native ingest; no curve asked for, none in the JSON
    out = _run_cli(["--bundle", REPO / "tests" / "golden" / "bundle", "--mono", "--criteria", "music", "--curve-step-ms", "0",
                    "--json", tmp_path / "b.json"])
    st_b = E.EchoCriterionSettings(criteria=(E.MUSIC,), curve_step_ms=0.0, use_mono_downmix_for_stereo=True)
    api = E.analyse_echo_criterion_bundle(REPO / "tests" / "golden" / "bundle", st_b)
    assert out == E.summarise_echo_criterion_text(api)
    assert [r.channel_name for r in api] == ["early:mono", "late_hot:mono"] and all(r.status == 0 for r in api)
    doc = json.loads((tmp_path / "b.json").read_text())
    assert all("curve" not in c for row in doc["echo_criterion"] for c in row["criteria"])
    assert E.echo_results_to_json(E.echo_results_from_json(doc)) == doc
