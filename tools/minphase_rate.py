#!/usr/bin/env python3
"""Device time of the minimum-phase / excess-phase analysis on 256 synthetic 480 000-sample IRs (10 s at 48 kHz) at the
default settings (oversample 4: N = 2^21 points per channel, 479 grid points, sub-batches of 46 channels under the 4 GiB
scratch budget), from the engine's events, median and min .. max of 7 after 2 warm-ups: the whole chain, and its split
between the three transforms (two ira_rfft_smooth, one ira_band_irfft_smooth), the existing ira_phase_unwrap and the new
kernels (ira_minphase_logmag, ira_minphase_excess, ira_minphase_gather) with the bytes each of those moves and the rate
that is; then the end-to-end analyse_minphase_batch time (upload, peak and onset, the records' way back to the host and
the host arithmetic included) and the same for minimum_phase_device (ira_minphase_spectrum and the second inverse in
place of the excess phase).
--one-call: one analysis at the defaults after one warm-up, nothing else on the device -- the run a kernel trace is taken
from.
--budgets: the chain's device time and the end-to-end time with engine.MINPHASE_SCRATCH_BYTES at 256 MiB, 1 GiB, 4 GiB
and 16 GiB (3, 11, 46 and 186 channels a sub-batch), the budgets alternating run by run."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from audio_analysis_amd.analyse import minphase as D
from audio_analysis_amd.engine import Engine
from audio_analysis_amd.synth import synth_ir

B, N_SAMPLES, SR, REPS, WARM = 256, 480_000, 48_000, 7, 2
eng = Engine("cuda:0")
host = [synth_ir(i, 0, N_SAMPLES, SR) for i in range(B)]
batch = eng.upload(host)
st = D.MinPhaseSettings()

if "--one-call" in sys.argv:
    for _ in range(2):
        D.minphase_device(eng, batch, SR, st)
        eng.sync()
    sys.exit(0)


def events_of(call):
    eng.events = []
    res = call()
    ev = eng.collect_events()
    eng.events = None
    return res, ev


def spread(ts):
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


def budget_sweep():
    names = [str(h) for h in range(B)]
    budgets = [256 << 20, 1 << 30, 4 << 30, 16 << 30]
    chain, e2e = {b: [] for b in budgets}, {b: [] for b in budgets}
    for rep in range(1 + 5):
        for b in budgets:
            D.E.MINPHASE_SCRATCH_BYTES = b
            res, ev = events_of(lambda: D.minphase_device(eng, batch, SR, st))
            eng.sync()
            t0 = time.perf_counter()
            D.analyse_minphase_batch(host, SR, names, st)
            dt = time.perf_counter() - t0
            if rep:
                chain[b].append(sum(float(np.sum(v)) for v in ev.values()))
                e2e[b].append(dt * 1e3)
    for b in budgets:
        c, e = spread(chain[b]), spread(e2e[b])
        D.E.MINPHASE_SCRATCH_BYTES = b
        print(f"budget {b >> 20} MiB, {len(D.E.minphase_cut(res.n_fft))} sub-batches: "
              f"chain {c[0]:.2f} ms ({c[1]:.2f} .. {c[2]:.2f}), end-to-end {e[0]:.0f} ms ({e[1]:.0f} .. {e[2]:.0f})", flush=True)


CALLS = ("ira_rfft_smooth", "ira_band_irfft_smooth", "ira_phase_unwrap", "ira_minphase_logmag", "ira_minphase_excess",
         "ira_minphase_gather", "ira_minphase_spectrum")


def measure(call):
    per = {name: [] for name in CALLS}
    total = []
    for rep in range(WARM + REPS):
        res, ev = events_of(call)
        if rep >= WARM:
            sums = {name: sum(float(np.sum(v)) for k, v in ev.items() if k.split("[")[0] == name) for name in CALLS}
            other = sum(float(np.sum(v)) for k, v in ev.items() if k.split("[")[0] not in CALLS)
            for name in CALLS:
                per[name].append(sums[name])
            total.append(sum(sums.values()) + other)
    return res, {name: spread(v) for name, v in per.items()}, spread(total)


if "--budgets" in sys.argv:
    budget_sweep()
    sys.exit(0)

res, per, total = measure(lambda: D.minphase_device(eng, batch, SR, st))
n_fft = int(res.n_fft[0])
nbins = n_fft // 2 + 1
assert np.all(res.n_fft == n_fft) and np.isfinite(res.records).all()
# bytes the new kernels move per channel: logmag reads X twice (the maximum, then G) and writes G; excess reads X and T and
# writes a double per bin; the gather touches 479 records
moved = {"ira_minphase_logmag": B * nbins * (16 + 16 + 16), "ira_minphase_excess": B * nbins * (16 + 16 + 8),
         "ira_minphase_gather": B * res.records.shape[1] * (16 + 3 * 16 + 3 * 8 + 64)}
new_ms = sum(per[name][0] for name in moved)
transforms_ms = per["ira_rfft_smooth"][0] + per["ira_band_irfft_smooth"][0]
names = [str(h) for h in range(B)]
D.analyse_minphase_batch(host, SR, names, st)
eng.sync()
t0 = time.perf_counter()
D.analyse_minphase_batch(host, SR, names, st)
e2e = time.perf_counter() - t0
row = dict(what="default analysis", irs=B, samples=N_SAMPLES, n_fft=n_fft, points=int(res.records.shape[1]),
           sub_batches=len(D.E.minphase_cut(res.n_fft)), chain_ms=total, per_call_ms=per, transforms_ms=transforms_ms,
           new_kernels_ms=new_ms, unwrap_ms=per["ira_phase_unwrap"][0],
           GBps={name: moved[name] / (per[name][0] * 1e6) for name in moved}, end_to_end_s=e2e)
print(f"default analysis: {B} x {N_SAMPLES} samples, N = 2^{n_fft.bit_length() - 1}, {row['points']} points, "
      f"{row['sub_batches']} sub-batches;  chain {total[0]:.2f} ms ({total[1]:.2f} .. {total[2]:.2f});  two forward transforms "
      f"{per['ira_rfft_smooth'][0]:.2f} ms, the inverse {per['ira_band_irfft_smooth'][0]:.2f} ms, unwrap "
      f"{per['ira_phase_unwrap'][0]:.2f} ms, new kernels {new_ms:.2f} ms (logmag {per['ira_minphase_logmag'][0]:.2f} ms "
      f"{row['GBps']['ira_minphase_logmag']:.0f} GB/s, excess {per['ira_minphase_excess'][0]:.2f} ms "
      f"{row['GBps']['ira_minphase_excess']:.0f} GB/s, gather {per['ira_minphase_gather'][0]:.3f} ms);  end-to-end "
      f"{e2e * 1e3:.0f} ms", flush=True)
rows = [row]

dev, per, total = measure(lambda: D.minimum_phase_device(eng, batch, SR, st))
moved_spec = B * nbins * (16 + 16 + 16)
row = dict(what="minimum-phase response", irs=B, samples=N_SAMPLES, n_fft=n_fft, chain_ms=total, per_call_ms=per,
           spectrum_GBps=moved_spec / (per["ira_minphase_spectrum"][0] * 1e6))
print(f"minimum-phase response: chain {total[0]:.2f} ms ({total[1]:.2f} .. {total[2]:.2f});  two forward transforms "
      f"{per['ira_rfft_smooth'][0]:.2f} ms, two inverses {per['ira_band_irfft_smooth'][0]:.2f} ms, logmag "
      f"{per['ira_minphase_logmag'][0]:.2f} ms, spectrum {per['ira_minphase_spectrum'][0]:.2f} ms "
      f"({row['spectrum_GBps']:.0f} GB/s)", flush=True)
rows.append(row)
print(json.dumps(rows))
