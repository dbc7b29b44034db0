#!/usr/bin/env python3
"""Device time of the modulation transfer sums on 256 synthetic channels of 480 000 samples with the octave bank (2560 rows:
the broadband signal plus 9 octave bands of every channel): ira_mtf_sums at the 14 standard modulation frequencies, from the
engine's events -- median and spread over the repeats, its float64 FMA rate in the sample loop (2 per sample and frequency)
and the bytes it reads.  Beside it, as the yardstick: ira_energy_windows (a pure float64 stream of the same rows, two early
limits) from the broadband onsets.  The band signals are built once; both calls only read them."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from audio_analysis_amd.analyse import energy as E
from audio_analysis_amd.analyse import sti as S
from audio_analysis_amd.analyse._common import band_row_offsets
from audio_analysis_amd.analyse.rt60bands import Rt60BandsAnalysisSettings, band_signals_device
from audio_analysis_amd.engine import Engine
from audio_analysis_amd.synth import synth_ir

CH, N, SR, REPS, WARM = 256, 480_000, 48_000, 7, 2
FP64_PEAK_TFLOPS, HBM_COPY_TB_S = 78.6, 6.29      # MI355X: specified vector float64 peak, measured float4 copy
eng = Engine("cuda:0")
batch = eng.upload([synth_ir(i, 0, N, SR) for i in range(CH)])
bands, y, y_off = band_signals_device(eng, batch, SR, Rt60BandsAnalysisSettings(band_mode="octave"))
rows = 1 + len(bands)
base, seg_off = band_row_offsets(batch, (bands, y, y_off))
seg_len = np.repeat(batch.length.astype(np.int64), rows)
w = np.tile(S.modulation_turns(S.MODULATION_FREQUENCIES_HZ, SR), (seg_off.size, 1))
nf = int(w.shape[1])
onset, _, _ = eng.onset_index(batch, 0.01)
chan = np.repeat(np.arange(CH, dtype=np.int32), rows)
limits = np.tile(np.asarray(E.window_samples((50.0, 80.0), SR), dtype=np.int64), (seg_off.size, 1))
runs = {"ira_mtf_sums": [], "ira_energy_windows": []}
for rep in range(WARM + REPS):                        # the two calls alternate inside every repeat
    eng.sync()
    eng.events = []
    eng.mtf_sums(base, seg_off, seg_len, w)
    eng.energy_windows(base, seg_off, seg_len, chan, onset, limits)
    ev = eng.collect_events()
    if rep >= WARM:
        for n in runs:
            runs[n].append(float(np.sum(ev[n])))
eng.events = None


def stat(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))


samples = float(seg_len.sum())
out = dict(channels=CH, samples=N, rows=int(seg_len.size), frequencies=nf, repeats=REPS,
           mtf_sums=stat(runs["ira_mtf_sums"]), energy_windows=stat(runs["ira_energy_windows"]))
mtf_ms, en_ms = out["mtf_sums"]["median_ms"], out["energy_windows"]["median_ms"]
out["bytes"] = 4.0 * samples
out["mtf_fma"] = 2.0 * nf * samples
out["mtf_tfma_per_s"] = out["mtf_fma"] / mtf_ms / 1e9
out["mtf_fraction_of_fp64_peak"] = 2.0 * out["mtf_tfma_per_s"] / FP64_PEAK_TFLOPS
out["mtf_tb_per_s"] = out["bytes"] / mtf_ms / 1e9
out["energy_tb_per_s"] = out["bytes"] / en_ms / 1e9
out["energy_fraction_of_copy"] = out["energy_tb_per_s"] / HBM_COPY_TB_S
out["ratio"] = mtf_ms / en_ms
for n, k in (("ira_mtf_sums", "mtf_sums"), ("ira_energy_windows", "energy_windows")):
    s = out[k]
    print(f"{n}: median {s['median_ms']:.3f} ms (min {s['min_ms']:.3f}, max {s['max_ms']:.3f}) over {REPS} repeats")
print(f"ira_mtf_sums: {int(seg_len.size)} rows x {N} samples x {nf} frequencies: {out['mtf_tfma_per_s']:.2f} T float64 FMA/s in "
      f"the sample loop = {100.0 * out['mtf_fraction_of_fp64_peak']:.1f} % of the {FP64_PEAK_TFLOPS} TFLOPS vector float64 peak; "
      f"reads {out['bytes'] / 1e9:.2f} GB at {out['mtf_tb_per_s']:.2f} TB/s")
print(f"ira_energy_windows on the same rows: {out['energy_tb_per_s']:.2f} TB/s = {100.0 * out['energy_fraction_of_copy']:.1f} % of "
      f"the {HBM_COPY_TB_S} TB/s copy rate; ira_mtf_sums takes {out['ratio']:.2f} times as long")
print(json.dumps(out))
