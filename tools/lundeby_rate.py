#!/usr/bin/env python3
"""Device time of the Lundeby noise handling on 256 synthetic channels of 480 000 samples with the octave bank (2560 rows:
the broadband signal plus 9 octave bands of every channel): ira_block_energy, ira_lundeby_estimate, ira_edc_truncated and the
ira_curve_fits launch behind them, from the engine's events -- median and spread over the repeats, the bytes each sample
pass moves, the HBM bandwidth that implies and its share of the 8.0 TB/s peak and of the 6.29 TB/s a float4 copy reaches.  The band signals are built once; a band row's curve overwrites its signal,
so the signals are restored from a copy before every repeat (outside the timed calls).  Beside it, as the yardstick:
ira_edc_fits (the fused plain Schroeder curve + fits of the decay block) on the same 2560 rows from the same start indices."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from audio_analysis_amd.analyse import lundeby as L
from audio_analysis_amd.analyse._common import band_row_offsets
from audio_analysis_amd.analyse.decay import decay_fit_specs
from audio_analysis_amd.analyse.rt60bands import band_signals_device
from audio_analysis_amd.engine import Engine
from audio_analysis_amd.synth import synth_ir

CH, N, SR, REPS, WARM = 256, 480_000, 48_000, 7, 2
HBM_PEAK_TB_S, HBM_COPY_TB_S = 8.0, 6.29          # MI355X: specified peak, measured float4 copy
eng = Engine("cuda:0")
rng = np.random.default_rng(0)
host = []
for i in range(CH):
    x = synth_ir(i, 0, N, SR)
    host.append((x + rng.standard_normal(N).astype(np.float32) * np.float32(np.max(np.abs(x)) * 10.0 ** (-55.0 / 20.0))))
batch = eng.upload(host)
st = L.LundebySettings()
bands, y, y_off = band_signals_device(eng, batch, SR, st.bands)
y0 = y.clone()
NAMES = ("ira_block_energy", "ira_lundeby_estimate", "ira_edc_truncated", "ira_curve_fits")
runs = {n: [] for n in NAMES}
dev = None
for rep in range(WARM + REPS):
    y.copy_(y0)
    eng.sync()
    eng.events = []
    dev = L.lundeby_device(eng, batch, SR, st, band_signals=(bands, y, y_off))
    ev = eng.collect_events()
    if rep >= WARM:
        for n in NAMES:
            runs[n].append(float(np.sum(ev[n])))
rows = 1 + len(bands)
start = dev.start
row_len = np.repeat(batch.length.astype(np.int64) - start, rows)
curve_len = dev.lens_dev.cpu().numpy().astype(np.int64)
status = dev.records.cpu().numpy()[:, 0].astype(np.int64)
# the yardstick: the fused plain EDC + fits on the same rows
y.copy_(y0)
base, seg_off = band_row_offsets(batch, (bands, y, y_off))
seg_off = seg_off + np.repeat(start, rows)
_, ranges = decay_fit_specs(st.decay)
fused = []
for rep in range(WARM + REPS):
    eng.sync()
    eng.events = []
    eng.edc_fits(base, seg_off, row_len, st.decay.edc_epsilon, st.decay.edc_floor_db, 1.0, float(SR), ranges, 8,
                 cross=(0.0, -10.0))
    ev = eng.collect_events()
    if rep >= WARM:
        fused.append(float(np.sum(ev["ira_edc_fits"])))
eng.events = None


def stat(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))


samples = float(row_len.sum())
out = dict(channels=CH, samples=N, rows=int(row_len.size), repeats=REPS, status_counts={int(k): int(np.sum(status == k)) for k in np.unique(status)},
           mean_curve_fraction=float(curve_len.sum() / samples), kernels={n: stat(runs[n]) for n in NAMES}, edc_fits=stat(fused))
# pass 1 reads every sample of every row once; pass 2 reads and writes the samples in front of the cross-point
bytes1 = 4.0 * samples
bytes2 = 8.0 * float(curve_len.sum())
out["block_energy_bytes"], out["edc_truncated_bytes"] = bytes1, bytes2
out["block_energy_tb_per_s"] = bytes1 / out["kernels"]["ira_block_energy"]["median_ms"] / 1e9
out["edc_truncated_tb_per_s"] = bytes2 / out["kernels"]["ira_edc_truncated"]["median_ms"] / 1e9
for k in ("block_energy", "edc_truncated"):
    out[k + "_fraction_of_peak"] = out[k + "_tb_per_s"] / HBM_PEAK_TB_S
    out[k + "_fraction_of_copy"] = out[k + "_tb_per_s"] / HBM_COPY_TB_S
for n in NAMES:
    s = out["kernels"][n]
    print(f"{n}: median {s['median_ms']:.3f} ms (min {s['min_ms']:.3f}, max {s['max_ms']:.3f}) over {REPS} repeats")
print(f"ira_block_energy moves {bytes1 / 1e9:.2f} GB: {out['block_energy_tb_per_s']:.2f} TB/s; ira_edc_truncated moves "
      f"{bytes2 / 1e9:.2f} GB ({100.0 * out['mean_curve_fraction']:.1f} % of the samples lie in front of the cut): "
      f"{out['edc_truncated_tb_per_s']:.2f} TB/s")
for k in ("block_energy", "edc_truncated"):
    print(f"ira_{k}: {100.0 * out[k + '_fraction_of_peak']:.1f} % of the {HBM_PEAK_TB_S} TB/s HBM peak, "
          f"{100.0 * out[k + '_fraction_of_copy']:.1f} % of the {HBM_COPY_TB_S} TB/s copy rate")
s = out["edc_fits"]
print(f"ira_edc_fits on the same rows: median {s['median_ms']:.3f} ms (min {s['min_ms']:.3f}, max {s['max_ms']:.3f})")
print(json.dumps(out))
