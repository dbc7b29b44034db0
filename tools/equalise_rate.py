#!/usr/bin/env python3
"""Device time of the equalisation filter design on 64 synthetic channels of 2 s at 48 kHz: N = 2^18, 1/3 octave smoothing
(b = 3), 8192 taps.  Per library call of equalise_device from the engine's events (every launch of a call summed; median
and spread over the repeats), the share the three new streaming calls (ira_eq_power, ira_eq_pyramid, ira_eq_smooth) take of
the whole chain, ira_eq_smooth beside the long transforms, and the bytes each streaming call moves per second beside the
HBM copy rate tools/mtf_rate.py uses as its yardstick.  Then the whole design end to end (upload excluded), a host clock
around calls that end in a device synchronise."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from audio_analysis_amd.analyse import equalise as Q
from audio_analysis_amd.engine import Engine, equalise_row_doubles

CH, SR, SECONDS, REPS, WARM, E2E_REPS = 64, 48_000, 2.0, 7, 2, 5
HBM_COPY_TB_S = 6.29                                  # MI355X: measured float4 copy (tools/mtf_rate.py)
st = Q.EqualiseSettings(smoothing=3)


def response(seed):
    """Decaying noise behind a direct sound: a room-like response of 2 s."""
    rng = np.random.default_rng(seed)
    n = int(SECONDS * SR)
    x = rng.standard_normal(n) * np.exp(-np.arange(n) / (0.3 * SR)) * 0.2
    x[100] = 1.0
    return x.astype(np.float32)


eng = Engine("cuda:0")
made = [response(s) for s in range(8)]
batch = eng.upload([made[i % len(made)] for i in range(CH)])
runs = {}
for rep in range(WARM + REPS):
    eng.sync()
    eng.events = []
    rec = Q.equalise_device(eng, batch, SR, st)
    ev = eng.collect_events()
    if rep >= WARM:
        for name, v in ev.items():
            runs.setdefault(name, []).append((len(v), float(np.sum(v))))
eng.events = None
n_fft = rec.n_fft
assert n_fft == 1 << 18 and len(rec.rows) == CH and np.all(np.isfinite(rec.ref))

e2e = []
for rep in range(1 + E2E_REPS):
    eng.sync()
    t0 = time.perf_counter()
    rec = Q.equalise_device(eng, batch, SR, st)
    results = Q.equalise_results(rec, SR, [str(i) for i in range(CH)])
    eng.sync()
    if rep:
        e2e.append(1000.0 * (time.perf_counter() - t0))


def stat(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))


calls = {name: dict(launches=v[0][0], **stat([ms for _, ms in v])) for name, v in runs.items()}
total = sum(c["median_ms"] for c in calls.values())
new = ("ira_eq_power", "ira_eq_pyramid", "ira_eq_smooth")
nbins = n_fft // 2 + 1
moved = {                                             # bytes per call of the chain (both invocations), rows = CH
    "ira_eq_power": CH * nbins * (16.0 + 8.0) + CH * nbins * (32.0 + 8.0),
    "ira_eq_pyramid": 2.0 * CH * 8.0 * (nbins + 2.0 * (equalise_row_doubles(n_fft) - nbins)),
    "ira_eq_smooth": 2.0 * CH * nbins * (8.0 + 8.0 + 8.0),      # level 0 once (the walk is served from the caches), S, the tables
}
out = dict(channels=CH, n_fft=n_fft, smoothing=st.smoothing, taps=st.taps, repeats=REPS, calls=calls, chain_ms=total,
           new_calls_share=sum(calls[n]["median_ms"] for n in new) / total, end_to_end=stat(e2e), end_to_end_repeats=E2E_REPS)
print(f"{CH} channels x {int(SECONDS * SR)} samples, N = {n_fft}, b = {st.smoothing}, {st.taps} taps; per call of the chain "
      f"(all its launches), median (min .. max) over {REPS} repeats:")
for name, c in sorted(calls.items(), key=lambda kv: -kv[1]["median_ms"]):
    extra = ""
    if name in moved:
        extra = f", {moved[name] / 1e9:.2f} GB moved: {moved[name] / c['median_ms'] / 1e9:.3f} TB/s " \
                f"= {100.0 * moved[name] / c['median_ms'] / 1e9 / HBM_COPY_TB_S:.0f} % of the copy rate"
    print(f"  {name}: {c['median_ms']:.3f} ms ({c['min_ms']:.3f} .. {c['max_ms']:.3f}), {c['launches']} timed calls, "
          f"{100.0 * c['median_ms'] / total:.1f} % of the chain{extra}")
transforms = sum(c["median_ms"] for n, c in calls.items() if "fft" in n)
print(f"the chain: {total:.3f} ms of device time; the three new streaming calls {100.0 * out['new_calls_share']:.1f} % of it; "
      f"ira_eq_smooth {calls['ira_eq_smooth']['median_ms']:.3f} ms (two invocations) beside {transforms:.3f} ms of transforms "
      f"(three forward, two inverse)")
s = out["end_to_end"]
print(f"end to end: median {s['median_ms']:.2f} ms (min {s['min_ms']:.2f}, max {s['max_ms']:.2f}) over {E2E_REPS} repeats = "
      f"{CH / s['median_ms'] * 1000.0:.0f} filters/s; deviation from the target {np.mean([r.deviation_before_db for r in results]):.2f}"
      f" dB before, {np.mean([r.deviation_after_db for r in results]):.2f} dB after")
print(json.dumps(out))
