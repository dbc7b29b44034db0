#!/usr/bin/env python3
"""Device time of the dual-channel spectral sums on 256 pairs of 60 s at 48 kHz (256 reference and 256 measurement rows of
2 880 000 synthetic noise samples), overlap 0.5, delay 0, Hann, at n_fft 1024, 4096 and 8192: the two launches of
Engine.cross_spectra (ira_xspec_accumulate, ira_xspec_finish) from the engine's events, median (min .. max) of 7 repeats
after 2 warm-ups; beside them the time a plain device copy of the bytes the accumulate launch reads (every sample of both
rows once per frame that covers it, 4 bytes each) takes, and of the bytes it reads at least once."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from audio_analysis_amd.engine import XSPEC_FRAMES, Engine, xspec_frames

PAIRS, N, SR, REPS, WARM = 256, 60 * 48_000, 48_000, 7, 2
eng = Engine("cuda:0")
gen = torch.Generator(device="cuda:0")
gen.manual_seed(1)
x_dev = torch.randn(2 * PAIRS * N, dtype=torch.float32, device="cuda:0", generator=gen)   # row 2p: reference, 2p + 1: measurement
x_off = np.arange(PAIRS, dtype=np.int64) * 2 * N
y_off = x_off + N
n = np.full(PAIRS, N, dtype=np.int64)


def copy_ms(nbytes):
    """A device-to-device copy that READS nbytes (and writes as many), median of REPS, from events."""
    m = int(nbytes) // 4
    src, dst = torch.empty(m, dtype=torch.float32, device="cuda:0"), torch.empty(m, dtype=torch.float32, device="cuda:0")
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
    del src, dst
    return float(np.median(ts))


def stats(v):
    return [float(np.median(v)), float(np.min(v)), float(np.max(v))]


rows = []
for n_fft in (1024, 4096, 8192):
    hop = n_fft // 2
    acc, fin = [], []
    for rep in range(WARM + REPS):
        eng.events = []
        out = eng.cross_spectra(x_dev, x_off, y_off, n, n_fft, hop, True)
        ev = eng.collect_events()
        eng.events = None
        if rep >= WARM:
            acc.append(sum(float(np.sum(v)) for k, v in ev.items() if k.startswith("ira_xspec_accumulate")))
            fin.append(sum(float(np.sum(v)) for k, v in ev.items() if k.startswith("ira_xspec_finish")))
    frames = int(xspec_frames(n, n_fft, hop)[0])
    chunks = -(-frames // XSPEC_FRAMES)
    nbins = n_fft // 2 + 1
    read_frames = 2.0 * 4.0 * PAIRS * frames * n_fft             # both rows, every frame's samples
    read_once = 2.0 * 4.0 * PAIRS * ((frames - 1) * hop + n_fft)
    partial = 8.0 * PAIRS * chunks * 4 * nbins                    # written by accumulate, read by finish
    coh = out[:, 8, 1:].mean().item()
    del out
    row = dict(n_fft=n_fft, hop=hop, pairs=PAIRS, samples=N, frames_per_pair=frames, chunks_per_pair=chunks,
               bytes_read_per_frame=read_frames, bytes_read_once=read_once, partial_bytes=partial,
               accumulate_ms=stats(acc), finish_ms=stats(fin), copy_frame_bytes_ms=copy_ms(read_frames),
               copy_once_bytes_ms=copy_ms(read_once), copy_partial_bytes_ms=copy_ms(partial), mean_coherence=coh)
    rows.append(row)
    a, f = row["accumulate_ms"], row["finish_ms"]
    print(f"n_fft {n_fft} hop {hop}: {PAIRS} pairs x {frames} frames ({chunks} chunks), {PAIRS * frames / 1e6:.3f} M transforms;  "
          f"ira_xspec_accumulate {a[0]:.3f} ms ({a[1]:.3f} .. {a[2]:.3f}) = {a[0] * 1e3 / (PAIRS * frames):.3f} us per frame on the "
          f"whole device;  ira_xspec_finish {f[0]:.3f} ms ({f[1]:.3f} .. {f[2]:.3f});  samples read per frame "
          f"{read_frames / 1e9:.3f} GB (copy {row['copy_frame_bytes_ms']:.3f} ms), at least once {read_once / 1e9:.3f} GB (copy "
          f"{row['copy_once_bytes_ms']:.3f} ms), partial sums {partial / 1e9:.3f} GB (copy {row['copy_partial_bytes_ms']:.3f} ms)",
          flush=True)
print(json.dumps(rows))
