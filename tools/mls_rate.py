#!/usr/bin/env python3
"""Device time of the three MLS kernels (ira_mls_fold, ira_mls_hadamard, ira_mls_finish) per order, 64 channels of
Gaussian float32 samples, R = 4 averaged periods, from the engine's events: median and min .. max of 7 after 2 warm-ups,
with the bytes each call moves and the rate that is.  Orders 10, 12, T + 1 = 13, 16, 18 and 21 (T = 12, the tile order of
the transform): one, one, two, two, two and three passes of the transform (engine.mls_pass_plan, printed per order).
Bytes counted per channel: the fold reads its R P samples twice (the sum, then the residual), G once and writes 2^m doubles;
a pass of the transform reads and writes 2^m doubles; the finish reads P doubles through `out` (8 bytes each, scattered),
the table and writes P floats.  Tables are uploaded before the timing."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from audio_analysis_amd import engine as E
from audio_analysis_amd.engine import Engine

NB, R, REPS, WARM = 64, 4, 7, 2
ORDERS = (10, 12, E.MLS_TILE_LOG2 + 1, 16, 18, 21)
CALLS = ("ira_mls_fold", "ira_mls_hadamard", "ira_mls_finish")
eng = Engine("cuda:0")
t = eng.torch


def spread(ts):
    return [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]


rows = []
for m in ORDERS:
    p = (1 << m) - 1
    t.manual_seed(m)
    x = t.randn(NB * R * p, dtype=t.float32, device=eng.device)
    begin = np.arange(NB, dtype=np.int64) * (R * p)
    h = eng.empty(NB << m, t.float32)
    h_off = np.arange(NB, dtype=np.int64) << m
    eng.mls_device_tables(m)
    per = {name: [] for name in CALLS}
    for rep in range(WARM + REPS):
        eng.events = []
        w, sums = eng.mls_fold(x, begin, m, R)
        eng.mls_hadamard(w, NB, m)
        eng.mls_finish(w, NB, m, R, h, h_off)
        ev = eng.collect_events()
        eng.events = None
        if rep >= WARM:
            for name in CALLS:
                per[name].append(sum(float(np.sum(v)) for k, v in ev.items() if k.split("[")[0] == name))
        del w, sums
    plan = E.mls_pass_plan(m)
    moved = {"ira_mls_fold": NB * (2 * 4 * R * p + 4 * p + 8 * (1 << m)),
             "ira_mls_hadamard": NB * len(plan) * 16 * (1 << m),
             "ira_mls_finish": NB * (8 * p + 4 * p + 4 * p)}
    ms = {name: spread(per[name]) for name in CALLS}
    rate = {name: moved[name] / (ms[name][0] * 1e6) for name in CALLS}
    rows.append(dict(order=m, channels=NB, periods=R, pass_plan=plan, ms=ms, bytes=moved, GBps=rate))
    print(f"order {m}: {NB} channels, R = {R}, passes (first bit, bits) {plan};  "
          + ";  ".join(f"{name[4:]} {ms[name][0]:.3f} ms ({ms[name][1]:.3f} .. {ms[name][2]:.3f}), "
                       f"{moved[name] / 1e6:.1f} MB, {rate[name]:.0f} GB/s" for name in CALLS), flush=True)
    del x, h
print(json.dumps(rows))
