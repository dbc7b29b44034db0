#!/usr/bin/env python3
"""Device time of the normalized echo density on 256 synthetic 480 000-sample IRs (10 s at 48 kHz) with the default 20 ms
Hann window (W = 961), at a step of 1 ms (48 samples, the default) and at a step of one sample: ira_echo_density alone
(its profile and record launches) from the engine's events, median and min .. max of 7 after 2 warm-ups; beside it the
time a plain device copy of the bytes the call reads would take, the multiply-add-compares (2 W K per channel: one pass
for the window sum, one for the count) over the device time, the end-to-end analyse_echo_density_batch time (upload,
onset, the profile's way back to the host and the host conversion included), and a vectorised NumPy restatement in
float64 on 4 channels, SCALED to the 256 (labelled as scaled: nobody waits for the whole batch)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from audio_analysis_amd.analyse import echodensity as D
from audio_analysis_amd.engine import Engine
from audio_analysis_amd.synth import synth_ir

B, N, SR, REPS, WARM, HOST_CHANNELS = 256, 480_000, 48_000, 7, 2, 4
eng = Engine("cuda:0")
host = [synth_ir(i, 0, N, SR) for i in range(B)]
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


def numpy_profile(x, onset, delta, w, step, chunk=512):
    """The definition in float64 NumPy, a chunk of positions at a time (whole windows only: positions whose window is
    clipped are left out, they are a few hundred of 480 000)."""
    h2 = x.astype(np.float64) ** 2
    k = (x.size - 1 - onset) // step + 1
    j = np.arange(k)
    c = onset + j * step
    j = j[(c - delta >= 0) & (c + delta < x.size)]
    a = float(np.cumsum(w)[-1])
    out = np.empty(j.size, np.float32)
    win = np.lib.stride_tricks.sliding_window_view(h2, w.size)
    for s in range(0, j.size, chunk):
        rows = win[onset + j[s : s + chunk] * step - delta]
        b = (rows * w).sum(axis=1)
        cnt = ((rows * a > (b * (1.0 + 2.0 ** -32))[:, None]) * w).sum(axis=1)
        out[s : s + chunk] = (cnt / a) / D.GAUSSIAN_FRACTION
    return out


rows = []
for step_ms, host_positions in ((1.0, None), (0.0, 20_000)):
    st = D.EchoDensitySettings(step_ms=step_ms)
    times = []
    for rep in range(WARM + REPS):
        eng.events = []
        res = D.echo_density_device(eng, batch, SR, st)
        ev = eng.collect_events()
        eng.events = None
        if rep >= WARM:
            times.append(sum(float(np.sum(v)) for k, v in ev.items() if k.startswith("ira_echo_density")))
    k = res.records[:, 0]
    w = 2 * res.delta + 1
    ops = 2.0 * w * float(np.sum(k))
    # float32 samples from the first window's start to the last one's end, the float32 profile written and read once more
    read = 4.0 * float(np.sum(np.minimum(res.length, res.onset + (k - 1) * res.step + res.delta + 1)
                              - np.maximum(res.onset - res.delta, 0))) + 4.0 * float(np.sum(k))
    names = [str(h) for h in range(B)]
    D.analyse_echo_density_batch(host, SR, names, st)
    eng.sync()
    t0 = time.perf_counter()
    D.analyse_echo_density_batch(host, SR, names, st)
    e2e = time.perf_counter() - t0
    # NumPy on HOST_CHANNELS channels; at one sample per step on the first host_positions positions only, scaled to K
    weights = D.window_weights(res.delta, st.window)
    t0 = time.perf_counter()
    done = 0
    for c in range(HOST_CHANNELS):
        x = host[c] if host_positions is None else host[c][: int(res.onset[c]) + host_positions + res.delta + 1]
        done += numpy_profile(x, int(res.onset[c]), res.delta, weights, res.step).size
    host_s = (time.perf_counter() - t0) * float(np.sum(k)) / done
    med = float(np.median(times))
    row = dict(step_ms=step_ms, step_samples=res.step, window_samples=w, irs=B, samples=N, positions=float(np.sum(k)),
               multiply_add_compares=ops, device_ms=[med, float(np.min(times)), float(np.max(times))],
               gops_per_s=ops / med / 1e6, bytes_read=read, copy_same_bytes_ms=copy_ms(read), end_to_end_s=e2e,
               numpy_scaled_s=host_s, numpy_measured_positions=done)
    rows.append(row)
    print(f"step {res.step} samples (W {w}): {row['positions'] / 1e6:.2f} M positions, {ops / 1e9:.1f} G multiply-add-compares;  "
          f"ira_echo_density {med:.3f} ms ({row['device_ms'][1]:.3f} .. {row['device_ms'][2]:.3f}) = {row['gops_per_s']:.0f} G/s;  "
          f"copy of the {read / 1e6:.1f} MB it reads {row['copy_same_bytes_ms']:.3f} ms;  end-to-end {e2e * 1e3:.0f} ms;  "
          f"NumPy float64, SCALED from {done} positions of {HOST_CHANNELS} channels to the batch: {host_s:.0f} s", flush=True)
print(json.dumps(rows))
