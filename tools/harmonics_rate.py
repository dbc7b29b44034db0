#!/usr/bin/env python3
"""Device time of the harmonic distortion measure on 256 synthetic recordings of a 10 s logarithmic sweep (20 Hz .. 20 kHz at
48 kHz) plus 2 s of tail, n_fft = 2^20, K = 5 harmonics, 3 points per octave: ira_harmonic_windows, the rfft_any call over
its 1280 rows and ira_harmonic_band_powers from the engine's events (the three calls enqueued on ready-made responses, as
harmonic_distortion_device enqueues them) -- median and spread over the repeats -- and the bytes the gather moves per second
beside the HBM copy rate tools/mtf_rate.py uses as its yardstick.  Then the whole measure end to end (upload excluded:
deconvolution, peak pick, the three calls, the results on the host), a host clock around calls that end in a device
synchronise."""
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from audio_analysis_amd.analyse import harmonics as H
from audio_analysis_amd.analyse.deconvolve import DeconvolveSettings, deconvolve_device
from audio_analysis_amd.engine import Engine

CH, SR, T, TAIL, REPS, WARM, E2E_REPS = 256, 48_000, 10.0, 2.0, 7, 2, 5
HBM_COPY_TB_S = 6.29                                  # MI355X: measured float4 copy (tools/mtf_rate.py)
st = H.HarmonicDistortionSettings()


def recording(c2, c3, amp=0.5):
    """(sweep, recording): x = amp sin(theta), theta = 2 pi f1 L (exp(t / L) - 1), with second and third harmonics added by
    phase, and silence appended."""
    n = int(T * SR)
    t = np.arange(n, dtype=np.float64) / SR
    L = st.sweep_rate_seconds
    theta = 2.0 * math.pi * st.start_frequency_hz * L * (np.exp(t / L) - 1.0)
    x = amp * np.sin(theta)
    y = x - c2 * amp * np.cos(2.0 * theta) - c3 * amp * np.sin(3.0 * theta)
    tail = np.zeros(int(TAIL * SR))
    return np.concatenate([x, tail]).astype(np.float32), np.concatenate([y, tail]).astype(np.float32)


eng = Engine("cuda:0")
pairs = [(0.03, 0.01), (0.05, 0.002), (0.01, 0.03), (0.002, 0.0005)]
made = [recording(*p) for p in pairs]
sweeps = eng.upload([made[0][0]])
rec = eng.upload([made[i % len(made)][1] for i in range(CH)])
group, sweep_of = list(range(CH)), [0] * CH
plan = H.harmonic_plan(st, SR)
k, nrow = st.max_harmonic, CH * st.max_harmonic
resp = deconvolve_device(eng, rec, group, sweeps, sweep_of, SR,
                         DeconvolveSettings(regularization_relative=st.regularization_relative, normalise_peak=False,
                                            remove_dc=False, output_length_mode="full_fft"))
n_fft = np.asarray(resp["n_fft"], dtype=np.int64)
assert int(n_fft.max()) == 1 << 20
peak, _ = eng.harmonic_peaks(resp["h"], resp["off"], n_fft - plan.search_margin)
row_off = np.arange(nrow, dtype=np.int64) * plan.seg
sizes = np.full(nrow, plan.fft_size, np.int32)
runs = {"windows": [], "rfft": [], "band_powers": []}
for rep in range(WARM + REPS):
    eng.sync()
    eng.events = []
    with eng.tagged("[w]"):
        rows = eng.harmonic_windows(resp["h"], resp["off"], n_fft, peak, plan.lags, plan.guard, plan.window)
    with eng.tagged("[f]"):
        spec, spec_off = eng.rfft_any(rows, row_off, sizes, False, data_len=np.full(nrow, plan.seg, np.int32), win_len=sizes)
    with eng.tagged("[p]"):
        eng.harmonic_band_powers(spec, spec_off, plan.lo, plan.cnt, plan.fft_size // 2 + 1)
    ev = eng.collect_events()
    if rep >= WARM:
        for name, tag in (("windows", "[w]"), ("rfft", "[f]"), ("band_powers", "[p]")):
            runs[name].append(float(sum(np.sum(v) for n, v in ev.items() if n.endswith(tag))))
eng.events = None

e2e = []
for rep in range(1 + E2E_REPS):
    eng.sync()
    t0 = time.perf_counter()
    res = H.harmonic_distortion_device(eng, rec, group, sweeps, sweep_of, SR, st)      # ends in copies to the host
    results = H.harmonic_distortion_results(res, SR, [str(i) for i in range(CH)], st)
    eng.sync()
    if rep:
        e2e.append(1000.0 * (time.perf_counter() - t0))
assert all(r.status == 0 for r in results)


def stat(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))


out = dict(channels=CH, n_fft=int(n_fft.max()), harmonics=k, points=int(plan.frequencies.size), rows=nrow, seg=plan.seg,
           fft_size=plan.fft_size, repeats=REPS, windows=stat(runs["windows"]), rfft=stat(runs["rfft"]),
           band_powers=stat(runs["band_powers"]), end_to_end=stat(e2e), end_to_end_repeats=E2E_REPS)
out["gather_bytes"] = 2.0 * 4.0 * nrow * plan.seg                                      # every sample read once, written once
out["gather_tb_per_s"] = out["gather_bytes"] / out["windows"]["median_ms"] / 1e9
out["gather_fraction_of_copy"] = out["gather_tb_per_s"] / HBM_COPY_TB_S
out["band_power_bytes"] = 16.0 * CH * float(plan.cnt.sum())
out["band_power_tb_per_s"] = out["band_power_bytes"] / out["band_powers"]["median_ms"] / 1e9
for name, key in (("ira_harmonic_windows", "windows"), ("rfft_any between them", "rfft"),
                  ("ira_harmonic_band_powers", "band_powers")):
    s = out[key]
    print(f"{name}: median {s['median_ms']:.4f} ms (min {s['min_ms']:.4f}, max {s['max_ms']:.4f}) over {REPS} repeats")
print(f"ira_harmonic_windows: {nrow} rows x {plan.seg} samples, {out['gather_bytes'] / 1e6:.1f} MB read + written at "
      f"{out['gather_tb_per_s']:.3f} TB/s = {100.0 * out['gather_fraction_of_copy']:.1f} % of the {HBM_COPY_TB_S} TB/s copy rate")
print(f"ira_harmonic_band_powers: {nrow} rows x {plan.frequencies.size} bands, {out['band_power_bytes'] / 1e6:.1f} MB of bins "
      f"read at {out['band_power_tb_per_s']:.3f} TB/s")
s = out["end_to_end"]
print(f"end to end, {CH} channels of {int(n_fft.max())} points: median {s['median_ms']:.2f} ms (min {s['min_ms']:.2f}, max "
      f"{s['max_ms']:.2f}) over {E2E_REPS} repeats = {CH / s['median_ms'] * 1000.0:.0f} channels/s")
print(json.dumps(out))
