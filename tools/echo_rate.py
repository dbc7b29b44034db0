#!/usr/bin/env python3
"""Device time of the Dietsch-Kraak echo criterion on 256 synthetic 480 000-sample IRs (10 s at 48 kHz), default criteria
(speech and music, 512 segments): ira_echo_criterion alone (its init, partial, carry, emit and fold launches) with the
second sample pass forming |y|^n again from the samples and with it reading the float64 stash the first pass left
(Engine.echo_stash), the two alternating, for max_tau_ms = 1000 (the default) and None (the whole response); beside it the
time a plain device copy of the bytes the two sample passes read would take, and the end-to-end
analyse_echo_criterion_batch time (upload, onset, filter bank and host conversion included).  The band signals are built
once and passed in (band_signals=...), so only the timed call repeats."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from audio_analysis_amd.analyse import echo as E
from audio_analysis_amd.analyse.rt60bands import Rt60BandsAnalysisSettings, band_signals_device
from audio_analysis_amd.engine import ECHO_CHUNK, Engine
from audio_analysis_amd.synth import synth_ir

B, N, SR, REPS, WARM = 256, 480_000, 48_000, 7, 2
eng = Engine("cuda:0")
host = [synth_ir(i, 0, N, SR) for i in range(B)]
batch = eng.upload(host)
bands, _ = E.criterion_bands(E.EchoCriterionSettings().criteria)
sig = band_signals_device(eng, batch, SR, Rt60BandsAnalysisSettings(transition_width_octaves=E.TRANSITION_WIDTH_OCTAVES),
                          bands=bands)


def copy_ms(nbytes):
    """A device-to-device copy that READS nbytes (and writes as many), median of REPS, from events."""
    n = int(nbytes) // 4
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


rows = []
for max_tau in (1000.0, None):
    st = E.EchoCriterionSettings(max_tau_ms=max_tau)
    times = {False: [], True: []}
    for rep in range(WARM + REPS):
        for stash in (False, True):                       # alternating: both see the same neighbours on the machine
            eng.echo_stash = stash
            eng.events = []
            res = E.echo_criterion_device(eng, batch, SR, st, band_signals=sig)
            ev = eng.collect_events()
            eng.events = None
            if rep >= WARM:
                times[stash].append(sum(float(np.sum(v)) for k, v in ev.items() if k.startswith("ira_echo_criterion")))
    eng.echo_stash = False
    m = res.records[:, :, 6]
    chunks = np.ceil(np.maximum(m, 0) / ECHO_CHUNK)
    # float32 bytes read: the partial pass reads M samples; the emit pass reads its own chunk and the one in front of it
    read_partial = 4.0 * float(np.sum(m))
    read_emit = 4.0 * float(np.sum(m + np.maximum(chunks - 1, 0) * ECHO_CHUNK))
    names = [str(h) for h in range(B)]
    E.analyse_echo_criterion_batch(host, SR, names, st)
    eng.sync()
    t0 = time.perf_counter()
    E.analyse_echo_criterion_batch(host, SR, names, st)
    e2e = time.perf_counter() - t0
    row = dict(max_tau_ms=max_tau, irs=B, samples=N, segments=int(m.size), samples_evaluated=float(np.sum(m)),
               bytes_read_both_passes=read_partial + read_emit,
               recompute_ms=[float(np.median(times[False])), float(np.min(times[False])), float(np.max(times[False]))],
               stash_ms=[float(np.median(times[True])), float(np.min(times[True])), float(np.max(times[True]))],
               copy_same_bytes_ms=copy_ms(read_partial + read_emit), end_to_end_s=e2e)
    rows.append(row)
    print(f"max_tau_ms {max_tau}: {row['segments']} segments, {row['samples_evaluated'] / 1e6:.1f} M samples, "
          f"{row['bytes_read_both_passes'] / 1e9:.3f} GB read by the two passes;  ira_echo_criterion recompute "
          f"{row['recompute_ms'][0]:.3f} ms ({row['recompute_ms'][1]:.3f} .. {row['recompute_ms'][2]:.3f}), stash "
          f"{row['stash_ms'][0]:.3f} ms ({row['stash_ms'][1]:.3f} .. {row['stash_ms'][2]:.3f});  copy of the same bytes "
          f"{row['copy_same_bytes_ms']:.3f} ms;  end-to-end {e2e * 1e3:.0f} ms", flush=True)
print(json.dumps(rows))
