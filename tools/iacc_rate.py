#!/usr/bin/env python3
"""Device time of the ISO 3382-1 inter-channel cross-correlation on 128 synthetic stereo pairs of 480 000 samples with the
octave bank: ira_xcorr_windows over the broadband signals plus the 9 octave bands of every pair (10 rows per pair, 97 lags
at 48 kHz, one early limit), its float64 FMA rate and its time per (sample x lag).  The band signals are built once and
passed in (band_signals=...), so only the onset search and the timed call repeat.  Beside it, as the yardstick: the lag
sums of the AR fit (ar_lag_kernel behind ira_ar_gram) at order 96, i.e. 97 lags of ONE signal, on the same 256 channels, from
the engine's events, and the same per (sample x lag) figure."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from audio_analysis_amd.analyse import iacc as I
from audio_analysis_amd.analyse.rt60bands import band_signals_device
from audio_analysis_amd.engine import Engine
from audio_analysis_amd.synth import synth_ir

PAIRS, N, SR, REPS, ORDER = 128, 480_000, 48_000, 5, 96
eng = Engine("cuda:0")
host = [synth_ir(i, c, N, SR) for i in range(PAIRS) for c in (0, 1)]
batch = eng.upload(host)
pairs = [(2 * i, 2 * i + 1) for i in range(PAIRS)]
st = I.IaccSettings()
sig = band_signals_device(eng, batch, SR, st.bands)
for _ in range(2):
    res = I.iacc_device(eng, batch, pairs, SR, st, band_signals=sig)
eng.sync()
eng.events = []
for _ in range(REPS):
    I.iacc_device(eng, batch, pairs, SR, st, band_signals=sig)
ev = eng.collect_events()
name = f"ira_xcorr_windows[T{res.max_lag}]"
xc_ms = float(np.median(ev[name]))
rows_per_pair = 1 + len(sig[0])
nlag = 2 * res.max_lag + 1
samples = float(rows_per_pair) * float(np.sum(res.length - res.onset))        # rows (n counted from the onset) of every segment
fma = samples * (nlag + 2)                                                    # the lag products, El and Er
for _ in range(2):
    eng.ar_fit(batch.x, batch.off, batch.length, None, ORDER)
eng.collect_events()
for _ in range(REPS):
    eng.ar_fit(batch.x, batch.off, batch.length, None, ORDER)
ev = eng.collect_events()
eng.events = None
ar_ms = float(np.median(ev["ira_ar_gram"]))
ar_samples = float(np.sum(batch.length - ORDER))
row = dict(pairs=PAIRS, samples=N, rows_per_pair=rows_per_pair, lags=nlag, xcorr_ms=xc_ms, xcorr_fma=fma,
           xcorr_gfma_per_s=fma / xc_ms / 1e6, xcorr_ps_per_sample_lag=xc_ms * 1e9 / (samples * nlag),
           ar_order=ORDER, ar_channels=batch.count, ar_lag_ms=ar_ms,
           ar_lag_ps_per_sample_lag=ar_ms * 1e9 / (ar_samples * (ORDER + 1)))
row["ratio"] = row["xcorr_ps_per_sample_lag"] / row["ar_lag_ps_per_sample_lag"]
print(f"{name}: {PAIRS} pairs x {rows_per_pair} rows x {N} samples, {nlag} lags: {xc_ms:.3f} ms, "
      f"{row['xcorr_gfma_per_s']:.0f} G float64 FMA/s, {row['xcorr_ps_per_sample_lag']:.3f} ps per (sample x lag)")
print(f"ira_ar_gram (ar_lag_kernel) order {ORDER}, {batch.count} channels x {N} samples: {ar_ms:.3f} ms, "
      f"{row['ar_lag_ps_per_sample_lag']:.3f} ps per (sample x lag); ratio {row['ratio']:.2f}")
print(json.dumps(row))
