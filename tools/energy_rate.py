#!/usr/bin/env python3
"""Device time of the ISO 3382-1 energy parameters on 256 synthetic 480 000-sample IRs: the onset search (ira_onset_index,
behind its peak pick) and the windowed energy sums (ira_energy_windows) over the broadband signal plus every octave (9) or
third-octave band (26), i.e. 10 or 27 signals per IR, read once each.  The band signals are built once per configuration
and passed in (band_signals=...), so only the two timed calls repeat; the end-to-end analyse_energy_parameters_batch time
(filter bank included) is printed beside them.  GB/s = bytes of signal the windows kernel reads / its device time."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from audio_analysis_amd.analyse import energy as E
from audio_analysis_amd.analyse.rt60bands import Rt60BandsAnalysisSettings, band_signals_device
from audio_analysis_amd.engine import Engine
from audio_analysis_amd.synth import synth_ir

B, N, SR, REPS = 256, 480_000, 48_000, 5
eng = Engine("cuda:0")
host = [synth_ir(i, 0, N, SR) for i in range(B)]
batch = eng.upload(host)
rows = []
for mode in ("octave", "third"):
    st = E.EnergyParameterSettings(bands=Rt60BandsAnalysisSettings(band_mode=mode))
    sig = band_signals_device(eng, batch, SR, st.bands)
    for _ in range(2):
        E.energy_parameters_device(eng, batch, SR, st, band_signals=sig)
    eng.sync()
    eng.events = []
    for _ in range(REPS):
        E.energy_parameters_device(eng, batch, SR, st, band_signals=sig)
    ev = eng.collect_events()
    eng.events = None
    ms = {k: float(np.median(v)) for k, v in ev.items()}
    nsig = 1 + len(sig[0])
    # bytes the windows kernel reads: every sample from the onset to the end of each of the nsig signals of every IR
    onset = E.energy_parameters_device(eng, batch, SR, st, band_signals=sig).onset
    read = 4.0 * nsig * float(np.sum(batch.length - onset))
    names = [str(h) for h in range(B)]
    E.analyse_energy_parameters_batch(host, SR, names, st)
    eng.sync()
    t0 = time.perf_counter()
    E.analyse_energy_parameters_batch(host, SR, names, st)
    e2e = time.perf_counter() - t0
    row = dict(mode=mode, irs=B, samples=N, signals_per_ir=nsig, bytes_read=read,
               peak_ms=ms["ira_peak_index"], onset_ms=ms["ira_onset_index"], windows_ms=ms["ira_energy_windows"],
               windows_gbps=read / ms["ira_energy_windows"] / 1e6, end_to_end_s=e2e)
    rows.append(row)
    print(f"{mode:6s} {nsig:2d} signals/IR  {read / 1e9:5.2f} GB  ira_peak_index {row['peak_ms']:.3f} ms  "
          f"ira_onset_index {row['onset_ms']:.3f} ms  ira_energy_windows {row['windows_ms']:.3f} ms "
          f"({row['windows_gbps']:.0f} GB/s)  end-to-end {e2e * 1e3:.0f} ms", flush=True)
print(json.dumps(rows))
