#!/usr/bin/env python3
"""Device time of the energy decay relief on the benchmark's batch shape, 256 channels of 10 s at 48 kHz from
audio_analysis_amd.synth, at the default settings (n_fft 2048, hop 256, 3 rows an octave) and at (8192, 512, 24 an octave):
edr.edr_device per batch and per launch (ira_peak_index, ira_edr_power, ira_edr_integrate, ira_curve_fits) from the engine's
events, median (min .. max) of 7 repeats after 2 warm-ups.  Beside it, on the same run, ira_xspec_accumulate over the same
frames (the same channels as reference and measurement of 256 pairs, from the peak on): it does one packed transform per
frame where ira_edr_power does one per frame pair."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from audio_analysis_amd.analyse import edr
from audio_analysis_amd.engine import Engine
from audio_analysis_amd.synth import synth_batch

CHANNELS, N, SR, REPS, WARM = 256, 10 * 48_000, 48_000, 7, 2
eng = Engine("cuda:0")
batch = eng.upload(list(synth_batch(0, CHANNELS, N)))


def stats(v):
    return [float(np.median(v)), float(np.min(v)), float(np.max(v))]


def timed(run):
    """{call: [ms per repeat]} of run() and the total per repeat."""
    per, total = {}, []
    for rep in range(WARM + REPS):
        eng.events = []
        keep = run()
        ev = eng.collect_events()
        eng.events = None
        del keep
        if rep >= WARM:
            total.append(sum(float(np.sum(v)) for v in ev.values()))
            for k, v in ev.items():
                per.setdefault(k, []).append(float(np.sum(v)))
    return {k: stats(v) for k, v in per.items()}, stats(total)


rows = []
for n_fft, hop, ppo in ((2048, 256, 3), (8192, 512, 24)):
    st = edr.EdrSettings(n_fft=n_fft, hop_length=hop, points_per_octave=ppo)
    dev = edr.edr_device(eng, batch, SR, st)
    starts, lens, frames, nrows = dev.starts, dev.lens, dev.frames, int(dev.rows.first.size)
    del dev
    per, total = timed(lambda: edr.edr_device(eng, batch, SR, st))
    xs, _ = timed(lambda: eng.cross_spectra(batch.x, batch.off + starts, batch.off + starts, lens, n_fft, hop, True))
    acc = next(v for k, v in xs.items() if k.startswith("ira_xspec_accumulate"))
    row = dict(n_fft=n_fft, hop=hop, points_per_octave=ppo, rows=nrows, channels=CHANNELS, samples=N,
               frames_per_channel=int(frames[0]), edr_device_ms=total, per_call_ms=per, xspec_accumulate_ms=acc)
    rows.append(row)
    print(f"n_fft {n_fft} hop {hop} {ppo}/octave: {nrows} rows, {int(frames.sum())} frames;  edr_device {total[0]:.3f} ms "
          f"({total[1]:.3f} .. {total[2]:.3f});  " + ";  ".join(f"{k} {v[0]:.3f} ms ({v[1]:.3f} .. {v[2]:.3f})" for k, v in per.items())
          + f";  ira_xspec_accumulate over the same frames {acc[0]:.3f} ms ({acc[1]:.3f} .. {acc[2]:.3f})", flush=True)
print(json.dumps(rows))
