"""
The minimum-phase chain on the device (ira_minphase_*, audio_analysis_amd.analyse.minphase) against the float64 restatement
of tests/minphase_ref.py, held to its derived bounds (its docstring has the derivation): rounding the cepstrum to float32
moves phi_min by at most 2^-23 sum |c[n]|, the float64 transforms and the logarithm add a second term, and the SUM of
both is asserted for every field of every record; the wrapped excess phase and the group delays follow from it.  Shapes:
D = 5, 64, 100, 257 and 4097 (and 16) at oversample 2, 4 and 16 (N = 32 .. 2^17: the Bluestein length 32, the full-length
direct transform at 64, half-length transforms above, an element of several workgroups and several unwrap tiles at 2^17), post_ms,
onset and peak centres, silence, non-finite channels between good ones, sub-batches, a floor that engages, and the
analytic cases of the restatement's module against the device.  Polarity: a channel and its negation, and channels whose
samples sum below zero on every path the first transform takes, held without a 2 pi exemption (the device's Im X_0 is
+0.0 on all of them; measured on an MI355X, the unwrapped excess phase at the first grid point lies within 0.13 of its
bound of the restatement's).  The minimum-phase response against the restatement's, per sample within Bounds.response
(worst 0.26 of the bound, at N = 32).  The kernels alone, bin by bin: tests/test_gpu_minphase_kernels.py.
"""
import functools
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import minphase_ref as R
from oracle import ira_oracle as O

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
FS = 48000
U = 2.0 ** -53


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def _mp():
    from audio_analysis_amd.analyse import minphase as D
    return D


@functools.lru_cache(maxsize=None)
def channel(length, seed, peak_at=3):
    """Decaying noise behind a direct sound that is the one largest sample."""
    rng = np.random.default_rng(1000 + seed)
    x = rng.standard_normal(length) * np.exp(-np.arange(length) / max(length / 6.0, 1.0))
    x[min(peak_at, length - 1)] = 5.0
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


_REFS = {}


def reference(x, p, d, n, floor_db=-120.0):
    """The restatement of one channel and its bounds, computed once per (samples, p, D, N, floor)."""
    key = (np.asarray(x, dtype=np.float32)[:d].tobytes(), int(p), int(d), int(n), float(floor_db))
    if key not in _REFS:
        ref = R.chain(x, p, d, n, floor_db)
        _REFS[key] = (ref, R.Bounds(ref) if ref["valid"] else None)
    return _REFS[key]


def hold(res, ch, x, what, worst, analytic_excess=None, alias=0.0):
    """Every field of every record of channel ch against the restatement; worst[field] = max error / bound.
    analytic_excess (wrapped, per bin of the transform): the excess phase is held to it as well, within first + second +
    alias."""
    D = _mp()
    p, d, n = int(res.centre[ch]), int(res.segment[ch]), int(res.n_fft[ch])
    floor_db = res.settings.floor_db
    ref, b = reference(x, p, d, n, floor_db)
    k = res.bins[ch]
    rec, want = res.records[ch], R.records(ref, k)
    assert ref["valid"] and np.isfinite(rec).all(), what
    put = lambda name, ratio: worst.__setitem__(name, max(worst.get(name, 0.0), float(np.max(ratio))))
    put("X", np.abs(rec[:, :2] - want[:, :2]) / (2.0 * b.e_x))
    put("P", abs(res.pmax[ch] - ref["P"]) / (2.0 * (2.0 * math.sqrt(ref["P"]) * b.e_x + b.e_x ** 2) + 4.0 * U * ref["P"]))
    bm = b.phi_min()
    put("phi_min", np.abs(2.0 * rec[:, 2:5] - 2.0 * want[:, 2:5]) / bm)
    # the unwrapped excess phase: the running sum of whole turns rounds once per turn taken, on either side
    turns = np.count_nonzero(np.abs(np.diff(ref["wrapped"])) > np.pi)
    unwrap = 2.0 * (turns + 64) * U * float(np.max(np.abs(ref["excess"])))
    be = [bm + b.phi_rel(k + dk) + unwrap for dk in (-1, 0, 1)]
    every = bm + b.phi_rel(np.arange(n // 2 + 1)) + unwrap
    step = np.abs(R.wrap(np.diff(ref["wrapped"])))
    ambiguous = int(np.count_nonzero(np.pi - step <= every[1:] + every[:-1]))
    for q in range(3):
        err = rec[:, 5 + q] - want[:, 5 + q]
        if ambiguous:                       # a step within the bound of pi may turn the other way: whole turns are no error
            err = R.wrap(err)
        put("excess", np.abs(err) / be[q])
    worst["ambiguous"] = worst.get("ambiguous", 0) + ambiguous
    if analytic_excess is not None:
        ba = alias + b.phi_min(analytic=True)
        for q, dk in enumerate((-1, 0, 1)):
            put("analytic", np.abs(R.wrap(rec[:, 5 + q] - analytic_excess[k + dk])) / (ba + b.phi_rel(k + dk, 1) + unwrap))
    # the curves: the module's own arithmetic on the device's records against the same arithmetic on the restatement's
    got = D.minphase_arithmetic(rec, k, n, p, res.pmax[ch], int(res.floored[ch]), FS, floor_db)
    exp = D.minphase_arithmetic(want, k, n, p, ref["P"], int(ref["floored"].sum()), FS, floor_db)
    derr = (rec[:, 7] - rec[:, 5]) - (want[:, 7] - want[:, 5])
    put("tau_e", np.abs(R.wrap(derr) if ambiguous else derr) / (4.0 * np.pi / n) / b.delay(be[0], be[2]))
    if not ambiguous:
        put("tau_e", np.abs(got["excess_group_delay_seconds"] - exp["excess_group_delay_seconds"]) * FS / b.delay(be[0], be[2]))
    put("tau_min", np.abs(got["minimum_group_delay_seconds"] - exp["minimum_group_delay_seconds"]) * FS / b.delay(bm, bm))
    # the floor: flags equal except where |X|^2 lies within the transform's error of P_floor
    near = np.abs(ref["power"] - ref["P_floor"]) <= 2.0 * (2.0 * b.mag * b.e_x + b.e_x ** 2) + 4.0 * b.e_x * math.sqrt(ref["P"]) * 10.0 ** (floor_db / 10.0)
    assert np.array_equal(got["floored"][~near[k]], ref["floored"][k][~near[k]]), what
    assert abs(int(res.floored[ch]) - int(ref["floored"].sum())) <= int(near.sum()), what
    clear = ~near[k] & ~ref["floored"][k]
    if clear.any():
        put("level_db", np.abs(got["level_db"] - exp["level_db"])[clear]
            / ((10.0 / math.log(10.0)) * (2.0 * 2.0 * b.e_x / b.mag[k][clear]) * 1.01 + 64.0 * U * np.abs(exp["level_db"][clear]) + 64.0 * U))
    assert np.array_equal(got["frequencies_hz"], k * FS / n) and np.array_equal(got["bin"], k)
    bad = {f: v for f, v in worst.items() if f != "ambiguous" and not v <= 1.0}
    assert not bad, (what, bad)
    return ref, b, near


def report(title, worst):
    print(f"{title}: worst error / bound " + ", ".join(f"{f} {v:.3g}" for f, v in worst.items() if f != "ambiguous")
          + f"; steps within the bound of pi: {worst.get('ambiguous', 0)}")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("oversample", [2, 4, 16])
def test_every_shape_against_the_restatement(oversample):
    """A mixed batch: D = 5, 64, 100, 257, 4097 (odd and even) and 16 (N = 64 at oversample 4), the peak as the centre."""
    D = _mp()
    eng = _eng()
    lens = (5, 64, 100, 257, 4097, 16)
    chans = [channel(n, i, peak_at=2 + i) for i, n in enumerate(lens)]
    st = D.MinPhaseSettings(oversample=oversample)
    res = D.minphase_device(eng, eng.upload(chans), FS, st)
    want_n = {2: [32, 128, 256, 1024, 16384, 32], 4: [32, 256, 512, 2048, 32768, 64],
              16: [128, 1024, 2048, 8192, 1 << 17, 256]}[oversample]
    assert list(res.n_fft) == want_n and list(res.segment) == list(lens) and list(res.centre) == [2, 3, 4, 5, 6, 7]
    assert res.records.shape == (6, 479, 8)
    worst = {}
    for ch, x in enumerate(chans):
        ref, b, near = hold(res, ch, x, f"oversample {oversample}, D = {lens[ch]}", worst)
        assert not ref["floored"].any() and res.floored[ch] == 0
    report(f"oversample {oversample}, N = {want_n}", worst)
    # the results through the module: per channel values and curves
    out = D.minphase_results(res, FS, [f"c{i}" for i in range(6)])
    for ch, r in enumerate(out):
        assert (r.centre, r.centre_samples, r.segment_samples, r.fft_size) == ("peak", 2 + ch, lens[ch], want_n[ch])
        assert r.floored_share == 0.0 and math.isfinite(r.excess_delay_seconds) and math.isfinite(r.excess_phase_span_deg)
        assert np.isfinite(r.level_db).all() and np.isfinite(r.excess_phase_deg).all() and len(r.frequencies_hz) == 479


def test_post_ms_cuts_the_segment_and_the_onset_is_the_device_onset():
    D = _mp()
    eng = _eng()
    chans = [channel(3000, 11, peak_at=40), channel(2001, 12, peak_at=1900), channel(130, 13, peak_at=7)]
    chans = [x.copy() for x in chans]
    for x, p in zip(chans, (40, 1900, 7)):                                  # quiet, then a rise in front of the peak: the onset lies before it
        x[: p - 2] *= np.float32(0.01)
        x[p - 2], x[p - 1] = 0.2, 1.5
    st = D.MinPhaseSettings(post_ms=2.5, centre="onset", onset_db=-20.0, oversample=2)
    res = D.minphase_device(eng, eng.upload(chans), FS, st)
    onset = eng.onset_index(eng.upload(chans), st.rel_energy)[0].cpu().numpy()
    want_onset = [int(np.nonzero(x.astype(np.float64) ** 2 >= float(x[p]) ** 2 * st.rel_energy)[0][0]) for x, p in zip(chans, (40, 1900, 7))]
    assert list(res.centre) == list(onset) == want_onset == [39, 1899, 6]
    assert list(res.segment) == [39 + 1 + 120, 2001, 127] and list(res.n_fft) == [512, 4096, 256]      # D below L, D = L, D below L
    worst = {}
    for ch, x in enumerate(chans):
        hold(res, ch, x, f"post_ms, channel {ch}", worst)
    report("post_ms 2.5, onset centres", worst)
    # the peak as the centre moves phi_rel alone: X and phi_min are the segment's
    peak = D.minphase_device(eng, eng.upload(chans), FS, D.MinPhaseSettings(post_ms=2.5 - 1000.0 / FS, oversample=2))
    assert list(peak.centre) == [40, 1900, 7] and list(peak.segment) == list(res.segment)
    assert np.array_equal(bits(peak.records[:, :, :5]), bits(res.records[:, :, :5]))
    assert not np.array_equal(peak.records[:, :, 5:], res.records[:, :, 5:])


def test_silence_and_non_finite_channels_touch_no_other_channel():
    D = _mp()
    eng = _eng()
    a, b = channel(100, 21), channel(100, 22, peak_at=9)
    nan_ch, inf_ch = channel(100, 23).copy(), channel(100, 24).copy()
    nan_ch[50], inf_ch[99] = np.nan, np.inf
    late = channel(100, 25).copy()
    late[80] = np.nan                                                       # behind the segment post_ms keeps: the channel has values
    assert eng.smooth_split(256) is not None                                # N = 512 rides a half-length transform of its own
    st = D.MinPhaseSettings()
    alone = D.minphase_device(eng, eng.upload([a, b]), FS, st)
    batch = [a, nan_ch, b, np.zeros(100, np.float32), inf_ch, np.zeros(0, np.float32)]
    mixed = D.minphase_device(eng, eng.upload(batch), FS, st, centre_samples=[3, 3, 9, 0, 3, 0])
    assert list(alone.centre) == [3, 9] and list(mixed.n_fft) == [512] * 5 + [32]
    assert np.array_equal(bits(mixed.records[[0, 2]]), bits(alone.records)) and np.isfinite(alone.records).all()
    assert np.array_equal(bits(mixed.pmax[[0, 2]]), bits(alone.pmax)) and list(mixed.floored) == [0] * 6
    assert np.isnan(mixed.records[[1, 3, 4, 5]]).all()
    assert math.isnan(mixed.pmax[1]) and mixed.pmax[3] == 0.0 and not math.isfinite(mixed.pmax[4]) and mixed.pmax[5] == 0.0
    for r in D.minphase_results(mixed, FS, list("abcdef"))[1::2] + D.minphase_results(mixed, FS, list("abcdef"))[4:5]:
        assert np.isnan(r.level_db).all() and np.isnan(r.excess_phase_deg).all() and np.isnan(r.minimum_group_delay_seconds).all()
        assert not r.floored.any() and math.isnan(r.floored_share) and math.isnan(r.excess_delay_seconds)
    cut = D.minphase_device(eng, eng.upload([late, a]), FS, D.MinPhaseSettings(post_ms=1.0), centre_samples=[3, 3])
    assert list(cut.segment) == [52, 52] and np.isfinite(cut.records).all()
    # the response: silence stays silence, a non-finite channel is NaN, the neighbours are untouched
    hs = D.minimum_phase_impulse_responses(batch, FS, st)
    good = D.minimum_phase_impulse_responses([a, b], FS, st)
    assert [h.size for h in hs] == [100, 100, 100, 100, 100, 0] and all(h.dtype == np.float32 for h in hs)
    assert np.array_equal(hs[0], good[0]) and np.array_equal(hs[2], good[1]) and np.isfinite(good[0]).all()
    assert np.isnan(hs[1]).all() and np.isnan(hs[4]).all() and not hs[3].any()


def test_no_result_depends_on_the_sub_batch_cut(monkeypatch):
    from audio_analysis_amd import engine
    D = _mp()
    eng = _eng()
    worst = {}
    for length, n_fft, exact in ((100, 512, True), (7, 32, False)):
        direct = eng.smooth_split(n_fft // 2) is not None and n_fft >= 128
        assert direct == exact and (exact or eng.smooth_split(n_fft) is None)      # 512: half-length direct; 32: Bluestein
        chans = [channel(length, 40 + i, peak_at=1 + i) for i in range(5)]
        per = int(engine.minphase_scratch_bytes([n_fft])[0])
        runs = []
        for budget, cuts in ((per, 5), (2 * per, 3), (4 << 30, 1)):
            monkeypatch.setattr(engine, "MINPHASE_SCRATCH_BYTES", budget)
            assert len(engine.minphase_cut([n_fft] * 5)) == cuts
            runs.append(D.minphase_device(eng, eng.upload(chans), FS, D.MinPhaseSettings()))
        for res in runs:
            assert list(res.n_fft) == [n_fft] * 5
            for ch, x in enumerate(chans):
                hold(res, ch, x, f"N = {n_fft}, channel {ch}", worst)
        if exact:
            for res in runs[1:]:
                assert np.array_equal(bits(res.records), bits(runs[0].records)) and np.array_equal(bits(res.pmax), bits(runs[0].pmax))
        else:                               # every run lies within the bound of the restatement: two runs within twice that
            for ch, x in enumerate(chans):
                ref, b = reference(x, 1 + ch, length, n_fft)
                for res in runs[1:]:
                    assert np.all(np.abs(2.0 * (res.records[ch, :, 2:5] - runs[0].records[ch, :, 2:5])) <= 2.0 * b.phi_min())
    report("sub-batches of 1, 2 and 5 channels", worst)


def test_a_floor_that_engages_on_a_comb():
    """x = [1, 0, .., 1], floor_db = -60: |X|^2 = 4 cos^2 falls below the floor at every notch.  The flags are the
    restatement's except at bins whose |X|^2 lies within the transform's error of P_floor: counted, at most 1 % of the bins."""
    D = _mp()
    eng = _eng()
    worst, combs = {}, []
    for d in (64, 257, 1000):
        x = np.zeros(d, dtype=np.float32)
        x[0] = x[-1] = 1.0
        combs.append(x)
    st = D.MinPhaseSettings(floor_db=-60.0, f_max_hz=24000.0)
    res = D.minphase_device(eng, eng.upload(combs), FS, st, centre_samples=[0, 0, 0])
    for ch, x in enumerate(combs):
        ref, b, near = hold(res, ch, x, f"comb of {x.size} samples", worst)
        excepted = int(np.count_nonzero(near))
        assert excepted <= 0.01 * near.size and abs(res.pmax[ch] - 4.0) <= 1e-12
        assert 0 < ref["floored"].sum() and abs(int(res.floored[ch]) - int(ref["floored"].sum())) <= excepted
        r = D.minphase_results(res, FS, ["a", "b", "c"])[ch]
        assert 0.0 < r.floored_share < 0.2 and r.floored_share ==res.floored[ch] / (ref["n"] // 2 + 1) and np.all(r.level_db >= 10.0 * np.log10(4.0) - 60.0 - 1e-9)
        print(f"comb of {x.size} samples, N = {ref['n']}: {int(ref['floored'].sum())} floored bins, {excepted} within the "
              f"transform's error of the floor, device count {int(res.floored[ch])}")
    report("comb, floor -60 dB", worst)


# ------------------------------------------------------------------------------------------------ polarity
def _excess_bounds(ref, b, k, n):
    """What hold() allows the unwrapped excess phase at k - 1, k, k + 1, and its count of ambiguous steps."""
    bm = b.phi_min()
    turns = np.count_nonzero(np.abs(np.diff(ref["wrapped"])) > np.pi)
    unwrap = 2.0 * (turns + 64) * U * float(np.max(np.abs(ref["excess"])))
    be = [bm + b.phi_rel(k + dk) + unwrap for dk in (-1, 0, 1)]
    every = bm + b.phi_rel(np.arange(n // 2 + 1)) + unwrap
    step = np.abs(R.wrap(np.diff(ref["wrapped"])))
    return bm, be, int(np.count_nonzero(np.pi - step <= every[1:] + every[:-1]))


def test_polarity_and_a_negative_sample_sum():
    """A channel, its negation, a channel whose samples sum below zero, and one more such channel for every path the
    first transform takes (N = 32 Bluestein, N = 64 the full-length direct transform, N = 32768 a half-length one of
    several workgroups).  X_0 < 0 there: angle(X_0) is +pi by the +0.0 that numpy.fft.rfft leaves in Im X_0, and the unwrap
    starts from that bin.  Every channel is held as it stands, and the unwrapped excess phase at the first grid point
    is compared with the restatement's as a number, not modulo 2 pi: a -0.0 in the device's Im X_0 would move the whole
    curve by 360 degrees."""
    D = _mp()
    eng = _eng()
    a = channel(100, 71)
    neg = (-a).astype(np.float32)
    c = channel(257, 72, peak_at=4).copy()
    c[4] = -5.0
    c[:3] -= np.float32(0.5)
    chans = [a, neg, c] + [(-channel(d, 73 + i)).astype(np.float32) for i, d in enumerate((5, 16, 4097))]
    res = D.minphase_device(eng, eng.upload(chans), FS, D.MinPhaseSettings())
    assert list(res.n_fft) == [512, 512, 2048, 32, 64, 32768] and list(res.centre) == [3, 3, 4, 3, 3, 3]
    sums = [float(np.sum(x[:d].astype(np.float64))) for x, d in zip(chans, res.segment)]
    assert sums[0] > 0.0 and all(v < 0.0 for v in sums[1:]), sums
    out = D.minphase_results(res, FS, list("abcdef"))
    held = []
    for ch, x in enumerate(chans):
        worst = {}
        ref, b, _ = hold(res, ch, x, f"polarity, channel {ch} (sample sum {sums[ch]:.3g})", worst)
        n, k = int(res.n_fft[ch]), res.bins[ch]
        _, be, ambiguous = _excess_bounds(ref, b, k, n)
        first = res.records[ch, 0, 6] - R.records(ref, k)[0, 6]
        print(f"channel {ch}: sample sum {sums[ch]:.4g}, X_0 {ref['X'][0].real:.4g}, X_N/2 {ref['X'][-1].real:.4g}; unwrapped excess at "
              f"the first grid point off by {first:.3g} rad ({abs(first) / be[1][0]:.3g} of its bound), ambiguous steps {ambiguous}")
        if not ambiguous:
            assert abs(first) <= be[1][0], (ch, first, be[1][0])
        report(f"polarity, channel {ch}", worst)
        held.append((ref, b, be, ambiguous))
    # the negation against its original
    assert bits(res.pmax[1:2])[0] == bits(res.pmax[0:1])[0] and res.floored[1] == res.floored[0]
    assert np.array_equal(bits(res.records[1, :, 2:5]), bits(res.records[0, :, 2:5]))
    assert np.array_equal(bits(res.records[1, :, :2]), bits(-res.records[0, :, :2]))
    (_, b0, be0, amb0), (_, b1, be1, amb1) = held[0], held[1]
    for q in range(3):
        odd = R.wrap(res.records[1, :, 5 + q] - res.records[0, :, 5 + q] - np.pi)
        assert np.all(np.abs(odd) <= 2.0 * np.maximum(be0[q], be1[q])), (q, float(np.max(np.abs(odd))))
    if not (amb0 or amb1):
        span_bound = 2.0 * np.degrees(2.0 * float(np.max(np.maximum(be0[1], be1[1]))))
        assert abs(out[1].excess_phase_span_deg - out[0].excess_phase_span_deg) <= span_bound
        tau_e = 2.0 * np.maximum(b0.delay(be0[0], be0[2]), b1.delay(be1[0], be1[2]))
        assert np.all(np.abs(out[1].excess_group_delay_seconds - out[0].excess_group_delay_seconds) * FS <= tau_e)
    tau_min = 2.0 * max(b0.delay(b0.phi_min(), b0.phi_min()), b1.delay(b1.phi_min(), b1.phi_min()))
    assert np.all(np.abs(out[1].minimum_group_delay_seconds - out[0].minimum_group_delay_seconds) * FS <= tau_min)


def test_the_response_against_the_restatement():
    """minimum_phase_impulse_responses against minphase_ref.minimum_phase_ir on the mixed-length batch of
    test_every_shape_against_the_restatement at oversample 4, per sample within Bounds.response."""
    D = _mp()
    lens = (5, 64, 100, 257, 4097, 16)
    chans = [channel(n, i, peak_at=2 + i) for i, n in enumerate(lens)]
    st = D.MinPhaseSettings(oversample=4)
    hs = D.minimum_phase_impulse_responses(chans, FS, st)
    worst = 0.0
    for ch, (x, h) in enumerate(zip(chans, hs)):
        d, n = R.sizes(x.size, 2 + ch, FS, 4)
        assert h.dtype == np.float32 and h.shape == (d,) and d == lens[ch]
        ref, b = reference(x, 2 + ch, d, n)
        want = R.minimum_phase_ir(ref)
        ratio = float(np.max(np.abs(h.astype(np.float64) - want) / b.response(ref, want)))
        print(f"response, D = {d}, N = {n}: worst error / bound {ratio:.3g}")
        worst = max(worst, ratio)
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------ analytic cases
def _padded(x, length):
    out = np.zeros(length, dtype=np.float32)
    out[: len(x)] = x
    return out


@pytest.mark.parametrize("length", [64, 128])
def test_analytic_cases_on_the_device(length):
    """(a) .. (e) of tests/minphase_ref.py against the device, N = 256 and 512; no bin is floored in any of them."""
    D = _mp()
    eng = _eng()
    a = R.min_phase_fir()
    z, n = a.size - 1, 4 * length
    k_all = np.arange(n // 2 + 1)
    phi, alias = R.fir_phase(n), R.aliasing(n)
    delayed = np.zeros(length, dtype=np.float32)
    delayed[17 : 17 + a.size] = a
    reversed_ = _padded(a[::-1].copy(), length)
    chans = [_padded(a, length), delayed, R.fir_through_allpass(length), reversed_, reversed_]
    st = D.MinPhaseSettings(f_max_hz=24000.0)
    peaks = D.minphase_device(eng, eng.upload(chans), FS, st)
    assert list(peaks.centre) == [0, 17, 1, z, z]                           # the all-pass moves the peak: (c) needs the override
    res = D.minphase_device(eng, eng.upload(chans), FS, st, centre_samples=[0, 17, 0, z, 0])
    assert list(res.n_fft) == [n] * 5 and list(res.floored) == [0] * 5 and res.bins[0].max() >= n // 2 - 4
    zero = np.zeros(n // 2 + 1)
    expected = [zero, zero, R.allpass_phase(n), -2.0 * phi, -2.0 * phi - 2.0 * np.pi * k_all * z / n]
    worst = {}
    for ch, (x, want) in enumerate(zip(chans, expected)):
        ref, b, near = hold(res, ch, x, f"analytic case {ch}, N = {n}", worst, analytic_excess=want, alias=alias)
        assert not ref["floored"].any() and not near.any()
        if ch in (0, 1):                                                    # phi_min is the closed form
            worst["analytic"] = max(worst["analytic"], float(np.max(
                np.abs(2.0 * res.records[ch, :, 3] - phi[res.bins[ch]]) / (alias + b.phi_min(analytic=True)))))
    assert worst["analytic"] <= 1.0
    out = D.minphase_results(res, FS, list("abcde"))
    assert all(r.floored_share == 0.0 for r in out)
    # (c): the excess phase runs from (nearly) 0 to (nearly) -180 degrees over the grid
    k = res.bins[2]
    short = 180.0 - np.degrees(R.allpass_phase(n)[k[0]] - R.allpass_phase(n)[k[-1]])
    ref, b = reference(chans[2], 0, length, n)
    assert 0.0 < short < 6.0 and abs(out[2].excess_phase_span_deg - (180.0 - short)) <= np.degrees(
        2.0 * np.max(alias + b.phi_min(analytic=True) + b.phi_rel(k, 1)))
    assert abs(out[0].excess_phase_span_deg) <= np.degrees(2.0 * (alias + b.phi_min(analytic=True) + np.max(b.phi_rel(k, 1))))
    # (e) the response: (a) from (a) and from its reversal, with the input's energy
    hs = D.minimum_phase_impulse_responses([chans[0], reversed_], FS, st)
    want = _padded(a, length).astype(np.float64)
    l1, energy = float(np.sum(np.abs(want))), float(np.sum(want ** 2))
    ref, b = reference(chans[0], 0, length, n)
    each = 2.0 ** -24 * float(np.max(np.abs(want))) * (1.0 + 2.0 ** -20) + (alias + b.phi_min(analytic=True)) * l1
    for h in hs:
        assert h.dtype == np.float32 and h.shape == (length,)
        worst["response"] = max(worst.get("response", 0.0), float(np.max(np.abs(h.astype(np.float64) - want))) / each)
        got = float(np.sum(h.astype(np.float64) ** 2))
        worst["energy"] = max(worst.get("energy", 0.0),
                              abs(got - energy) / (2.0 * math.sqrt(energy) * math.sqrt(length) * each + length * each * each))
    report(f"analytic cases, N = {n}", worst)
    assert worst["response"] <= 1.0 and worst["energy"] <= 1.0


# ------------------------------------------------------------------------------------------------ module and command line
def test_cli_on_a_stereo_wav_equals_the_python_api(tmp_path):
    D = _mp()
    chans = [channel(6000, 61, peak_at=100), channel(6000, 62, peak_at=140)]
    wav = tmp_path / "room.wav"
    wav.write_bytes(O.recorder_wav_bytes(0.15 * np.stack(chans, axis=1).reshape(-1), FS))
    env = dict(os.environ, PYTHONPATH=str(REPO))
    out_json, out_dir = tmp_path / "room.json", tmp_path / "min"
    args = ["--oversample", "2", "--post-ms", "20", "--points-per-octave", "6", "--f-min", "50", "--floor-db", "-100"]
    r = subprocess.run([sys.executable, "-m", "analyse.minphase", "--input", str(wav), *args, "--json", str(out_json),
                        "--write-minimum-phase", str(out_dir)], capture_output=True, text=True, cwd=str(REPO), env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "NaN" not in out_json.read_text()
    doc = json.loads(out_json.read_text())
    st = D.MinPhaseSettings(oversample=2, post_ms=20.0, points_per_octave=6, f_min_hz=50.0, floor_db=-100.0)
    api = D.analyse_minphase_files([wav], st)
    assert [d["channel_name"] for d in doc["minimum_phase"]] == ["room.wav:left", "room.wav:right"]
    assert doc == D.minphase_results_to_json(api) and r.stdout == D.summarise_minphase_text(api)
    assert [d["segment_samples"] for d in doc["minimum_phase"]] == [1061, 1101] and doc["minimum_phase"][0]["fft_size"] == 4096
    assert len(doc["minimum_phase"][0]["level_db"]) == 52 and D.minphase_results_from_json(doc)[1].centre_samples == 140
    from scipy.io import wavfile
    rate, h = wavfile.read(str(out_dir / "room_minphase.wav"))
    assert rate == FS and h.dtype == np.float32 and h.shape == (1101, 2) and not h[1061:, 0].any()
    loaded = [c for _, c in __import__("audio_analysis_amd.analyse._common", fromlist=["wav_channels"]).wav_channels(wav, False)[1]]
    want = D.minimum_phase_impulse_responses(loaded, FS, st)
    assert np.array_equal(h[:1061, 0], want[0]) and np.array_equal(h[:, 1], want[1])
    assert int(np.argmax(np.abs(h[:, 0]))) < 20                             # the energy has moved to the front
