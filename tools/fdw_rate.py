#!/usr/bin/env python3
"""Device time of the frequency-dependent-window response on 256 synthetic 480 000-sample IRs (10 s at 48 kHz) at the
default settings (15 cycles, 48 points per octave, 20 Hz .. 20 kHz: 479 points, 2.51 M terms per channel) for both
windows: ira_fdw_response alone (its four launches) from the engine's events, median and min .. max of 7 after 2 warm-ups;
the terms summed and their rate; beside it the time a plain device copy of the bytes the call reads would take (every
window's float32 samples: the kernel is compute-bound, the copy shows by how much), the end-to-end analyse_fdw_batch time
(upload, peak and onset, the sums' way back to the host and the host arithmetic included), and the long-double restatement
of tests/fdw_ref.py on ONE channel, SCALED to the 256 (labelled as scaled: nobody waits for the whole batch).
--one-call: a single ira_fdw_response call at the defaults after one warm-up, nothing else on the device -- the run a
kernel trace is taken from (per-launch times: profiles/README.md)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import fdw_ref as R
from audio_analysis_amd.analyse import fdw as D
from audio_analysis_amd.engine import Engine
from audio_analysis_amd.synth import synth_ir

B, N_SAMPLES, SR, REPS, WARM = 256, 480_000, 48_000, 7, 2
eng = Engine("cuda:0")
host = [synth_ir(i, 0, N_SAMPLES, SR) for i in range(B)]
batch = eng.upload(host)

if "--one-call" in sys.argv:
    for _ in range(2):
        D.fdw_device(eng, batch, SR, D.FdwSettings())
        eng.sync()
    sys.exit(0)


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
for window in D.WINDOWS:
    st = D.FdwSettings(window=window)
    res, dev = device_ms(lambda: D.fdw_device(eng, batch, SR, st), "ira_fdw_response")
    half = res.half.astype(np.int64)
    terms = float(np.sum(res.sums[:, :, 5]))                                   # the terms inside the channels: N summed
    narrow_terms = float(np.sum(res.sums[:, half <= 127, 5]))
    read = 4.0 * terms
    names = [str(h) for h in range(B)]
    D.analyse_fdw_batch(host, SR, names, st)
    eng.sync()
    t0 = time.perf_counter()
    D.analyse_fdw_batch(host, SR, names, st)
    e2e = time.perf_counter() - t0
    t0 = time.perf_counter()
    for j in range(len(half)):
        R.reference(host[0], int(res.centre[0]), res.rho[j], int(half[j]), window)
    host_s = (time.perf_counter() - t0) * B
    row = dict(window=window, irs=B, samples=N_SAMPLES, points=int(half.size), narrow_points=int(np.count_nonzero(half <= 127)),
               terms=terms, narrow_terms=narrow_terms, device_ms=dev, terms_per_ns=terms / (dev[0] * 1e6),
               bytes_read=read, copy_same_bytes_ms=copy_ms(read), end_to_end_s=e2e, long_double_scaled_s=host_s,
               long_double_measured_channels=1)
    rows.append(row)
    print(f"{window}: {row['points']} points ({row['narrow_points']} narrow), {terms / 1e6:.1f} M terms ({narrow_terms / 1e6:.1f} M "
          f"narrow);  ira_fdw_response {dev[0]:.3f} ms ({dev[1]:.3f} .. {dev[2]:.3f}), {row['terms_per_ns']:.1f} terms/ns;  copy "
          f"of the {read / 1e6:.0f} MB it reads {row['copy_same_bytes_ms']:.3f} ms;  end-to-end {e2e * 1e3:.0f} ms;  long double, "
          f"SCALED from 1 channel to the batch: {host_s:.0f} s", flush=True)
print(json.dumps(rows))
