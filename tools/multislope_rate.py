#!/usr/bin/env python3
"""Device time of the multi-slope decay fits on 256 synthetic channels of 144 000 samples (3 s at 48 kHz) with the octave
bank (2560 rows: the broadband signal plus 9 octave bands of every channel), default settings (orders 1 to 3, a 64-point
grid, three refinements): ira_multislope_points once and ira_multislope_gram / ira_multislope_search per level, from the
engine's events -- median and spread over the repeats -- with the work each launch does: Gram jobs, multiply-adds and
exponentials, fit jobs and candidates.  The band signals are built once (the fits do not consume them)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from audio_analysis_amd.analyse import multislope as MS
from audio_analysis_amd.analyse.rt60bands import band_signals_device
from audio_analysis_amd.engine import MS_DOUBLES, Engine
from audio_analysis_amd.synth import synth_ir

CH, N, SR, REPS, WARM = 256, 144_000, 48_000, 7, 2
eng = Engine("cuda:0")
rng = np.random.default_rng(0)
host = []
for i in range(CH):
    x = synth_ir(i, 0, N, SR)
    host.append((x + rng.standard_normal(N).astype(np.float32) * np.float32(np.max(np.abs(x)) * 10.0 ** (-55.0 / 20.0))))
batch = eng.upload(host)
st = MS.MultiSlopeSettings()
band_signals = band_signals_device(eng, batch, SR, st.bands)
LEVELS = 1 + st.refine_levels
NAMES = ("ira_block_energy", "ira_multislope_points", "ira_multislope_gram", "ira_multislope_search")
runs = {n: [] for n in NAMES}
dev = None
for rep in range(WARM + REPS):
    eng.sync()
    eng.events = []
    dev = MS.multislope_device(eng, batch, SR, st, band_signals=band_signals)
    ev = eng.collect_events()
    if rep >= WARM:
        for n in NAMES:
            runs[n].append([float(v) for v in ev[n]])
eng.events = None


def stat(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))


info = dev.info.cpu().numpy()
levels = [r.cpu().numpy() for r in dev.level_records]
good = info[:, 0] == 0
J = info[good, 1].astype(np.float64)
out = dict(channels=CH, samples=N, rows=int(info.shape[0]), good_rows=int(good.sum()), repeats=REPS, mean_J=float(J.mean()),
           block_energy=stat([r[0] for r in runs["ira_block_energy"]]), points=stat([r[0] for r in runs["ira_multislope_points"]]),
           levels=[])
for lvl in range(LEVELS):
    rec = levels[lvl][good]                                            # (rows, 3, MS_DOUBLES)
    g = np.nan_to_num(rec[:, :, MS_DOUBLES - 1], nan=0.0)               # the grid size every fit job searched
    if lvl == 0:
        gram_jobs, funcs = int(good.sum()), np.full(int(good.sum()), st.grid + 2.0)
        pts = J
    else:
        gram_jobs, funcs = int(good.sum()) * st.max_order, (g[:, : st.max_order] + 2.0).reshape(-1)
        pts = np.repeat(J, st.max_order)
    # what the kernel executes: the full square of the padded function count would overstate it, the triangle understate it:
    # every thread holds NB x NB accumulators over 16 NB functions, all of them updated for every point
    nf = np.where(funcs <= 32, 32.0, np.where(funcs <= 80, 80.0, 144.0))
    level = dict(level=lvl, gram=stat([r[lvl] for r in runs["ira_multislope_gram"]]),
                 search=stat([r[lvl] for r in runs["ira_multislope_search"]]), gram_jobs=gram_jobs,
                 fit_jobs=int(good.sum()) * st.max_order, mean_grid=float(g[:, : st.max_order].mean()),
                 gram_fma_useful=float((pts * funcs * (funcs + 1.0) / 2.0).sum()), gram_fma_executed=float((pts * nf * nf).sum()),
                 gram_exponentials=float((pts * (funcs - 2.0)).sum()))
    level["gram_executed_tflops"] = 2.0 * level["gram_fma_executed"] / level["gram"]["median_ms"] / 1e9
    out["levels"].append(level)
status = np.array([int(levels[-1][r, s, 0]) for r in range(info.shape[0]) for s in range(st.max_order)])
out["record_status_counts"] = {int(k): int(np.sum(status == k)) for k in np.unique(status)}
print(f"ira_block_energy: median {out['block_energy']['median_ms']:.3f} ms; ira_multislope_points: median "
      f"{out['points']['median_ms']:.3f} ms (min {out['points']['min_ms']:.3f}, max {out['points']['max_ms']:.3f}) over {REPS} repeats")
for lv in out["levels"]:
    print(f"level {lv['level']}: ira_multislope_gram median {lv['gram']['median_ms']:.3f} ms (min {lv['gram']['min_ms']:.3f}, max "
          f"{lv['gram']['max_ms']:.3f}), {lv['gram_jobs']} jobs, {lv['gram_fma_executed'] / 1e9:.2f} G multiply-adds executed "
          f"({lv['gram_fma_useful'] / 1e9:.2f} G in the triangle), {lv['gram_exponentials'] / 1e9:.3f} G exponentials: "
          f"{lv['gram_executed_tflops']:.1f} TFLOP/s float64; ira_multislope_search median {lv['search']['median_ms']:.3f} ms (min "
          f"{lv['search']['min_ms']:.3f}, max {lv['search']['max_ms']:.3f}), {lv['fit_jobs']} jobs, mean grid {lv['mean_grid']:.1f}")
total = out["points"]["median_ms"] + sum(lv["gram"]["median_ms"] + lv["search"]["median_ms"] for lv in out["levels"])
print(f"all levels: {total:.3f} ms for {out['rows']} rows")
out["total_median_ms"] = total
print(json.dumps(out))
