#!/usr/bin/env python3
"""Device time of the early-reflection detection on 256 synthetic 480 000-sample IRs (10 s at 48 kHz) at the default
settings (1 ms Hann smoothing, W = 49; a 200 ms search) and with the search unbounded (--max-time-ms none): ira_reflections
alone (its four launches) from the engine's events, median and min .. max of 7 after 2 warm-ups; beside it the time a plain
device copy of the bytes the call reads would take, ira_echo_density at one sample per step limited to the same number
of positions (kmax) with the same window -- the closest existing kernel: the same loads and W multiply-adds per position
in its first pass, the envelope launch is to be judged against it --, the end-to-end analyse_reflections_batch time
(upload, onset, the rows' way back to the host and the host conversion included), and the float64 NumPy restatement of
tests/reflections_ref.py on 4 channels, SCALED to the 256 (labelled as scaled: nobody waits for the whole batch)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import reflections_ref as R
from audio_analysis_amd.analyse import echodensity as N
from audio_analysis_amd.analyse import reflections as D
from audio_analysis_amd.engine import Engine, refl_row_room
from audio_analysis_amd.synth import synth_ir

B, N_SAMPLES, SR, REPS, WARM, HOST_CHANNELS = 256, 480_000, 48_000, 7, 2, 4
eng = Engine("cuda:0")
host = [synth_ir(i, 0, N_SAMPLES, SR) for i in range(B)]
batch = eng.upload(host)


def copy_ms(nbytes):
    """A device-to-device copy that READS nbytes (and writes as many), median of REPS, from events."""
    n = max(1, int(nbytes) // 4)
    src, dst = torch.empty(n, dtype=torch.float32, device="cuda:0"), torch.empty(n, dtype=torch.float32, device="cuda:0")
    src.fill_(1.0)
    ts = []
    for i in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if i >= WARM:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def device_ms(call, prefix):
    times = []
    for rep in range(WARM + REPS):
        eng.events = []
        res = call()
        ev = eng.collect_events()
        eng.events = None
        if rep >= WARM:
            times.append(sum(float(np.sum(v)) for k, v in ev.items() if k.startswith(prefix)))
    return res, [float(np.median(times)), float(np.min(times)), float(np.max(times))]


rows = []
for max_time_ms in (200.0, None):
    st = D.ReflectionSettings(max_time_ms=max_time_ms)
    res, dev = device_ms(lambda: D.reflections_device(eng, batch, SR, st, keep_curve=False), "ira_reflections")
    c = res.counts
    held = refl_row_room(np.maximum(res.length - res.onset, 0), c.direct, c.tn, c.background)       # R per channel
    positions = float(np.sum(held))
    # float32 samples: the rows' spans for the envelope, the whole channel from the direct window on for the two energy
    # sums; float64 rows written once and read by the direct, the candidate (with its halo) and the record launches
    read = 4.0 * float(np.sum(held + 2 * c.half)) + 4.0 * float(np.sum(res.length - res.onset)) + 3.0 * 8.0 * positions
    kmax = int(held.max())
    ned = N.EchoDensitySettings(window_ms=st.smooth_ms, step_ms=0.0, max_time_ms=None)
    _, ned_dev = device_ms(lambda: eng.echo_density(batch.x, batch.off, batch.length, eng.onset_index(batch, ned.rel_energy)[0],
                                                    N.window_weights(c.half, "hann"), c.half, 1, kmax, (1.0,)),
                           "ira_echo_density")
    names = [str(h) for h in range(B)]
    D.analyse_reflections_batch(host, SR, names, st)
    eng.sync()
    t0 = time.perf_counter()
    out = D.analyse_reflections_batch(host, SR, names, st)
    e2e = time.perf_counter() - t0
    t0 = time.perf_counter()
    for ch in range(HOST_CHANNELS):
        R.detect(host[ch], int(res.onset[ch]), c.half, st.window, c.direct, c.direct_window, c.guard, c.separation,
                 c.background, c.tn, st.rel, st.prom, st.max_reflections)
    host_s = (time.perf_counter() - t0) * B / HOST_CHANNELS
    row = dict(max_time_ms=max_time_ms, window_samples=2 * c.half + 1, irs=B, samples=N_SAMPLES, row_entries=positions,
               candidates=float(np.sum(res.records[:, 2])), kept=float(np.sum(res.records[:, 3])), device_ms=dev,
               bytes_read=read, copy_same_bytes_ms=copy_ms(read), echo_density_same_positions_ms=ned_dev,
               end_to_end_s=e2e, numpy_scaled_s=host_s, numpy_measured_channels=HOST_CHANNELS)
    rows.append(row)
    print(f"search {'unbounded' if max_time_ms is None else f'{max_time_ms:g} ms'} (W {row['window_samples']}): "
          f"{positions / 1e6:.2f} M row entries, {row['candidates']:.0f} candidates, {row['kept']:.0f} kept;  "
          f"ira_reflections {dev[0]:.3f} ms ({dev[1]:.3f} .. {dev[2]:.3f});  copy of the {read / 1e6:.1f} MB it reads "
          f"{row['copy_same_bytes_ms']:.3f} ms;  ira_echo_density at step 1 over as many positions {ned_dev[0]:.3f} ms "
          f"({ned_dev[1]:.3f} .. {ned_dev[2]:.3f});  end-to-end {e2e * 1e3:.0f} ms;  NumPy float64, SCALED from "
          f"{HOST_CHANNELS} channels to the batch: {host_s:.0f} s", flush=True)
print(json.dumps(rows))
