#!/usr/bin/env python3
"""
Goldens at sample rates other than 48 kHz from the REFERENCE implementation, run in the build container:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python3 tests/golden/make_rate_goldens.py

For the table of tests/rates_cases.py it stores what the reference's own functions return:
  rates.json  tables/<rate>/<mode>        _build_band_definitions: [name, centre, kind, low edge, high edge] per band
              degenerate/<rate>/<mode>    indices of the bands whose clipped upper edge is Nyquist (pass == stop edge)
              blocks/<rate>/<channel>     per report block the scalars the 48 kHz goldens hold: segment start and length,
                                          per-band T30 / T20 / EDT (None = no fit), decay fits, peak and centroid,
                                          waterfall slice indices, modal point count, spectrogram shape
  rates.npz   mask/<rate>/<mode>/<n>/<band index>   _make_*_mask on rfftfreq(n, 1 / rate).astype(float32), for the lowest,
                                          the highest and every degenerate band, n = 4 800 and 23 257
              modal/edges/<rate>          _build_log_bins for the clipped default range
              wf/times/<rate>/<channel>   the waterfall's slice times
Only names, settings and expected outputs are stored; no reference source text.  The archive is written with fixed
timestamps, so running this again gives the same bytes.
"""
from __future__ import annotations

import io
import json
import os
import sys
import zipfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
# the REFERENCE's `analyse` package must win over this repo's import-name shim of the same name
sys.path[:] = [p for p in sys.path if p.rstrip("/") != "/root/reference"]
sys.path.insert(0, "/root/reference")
os.environ.setdefault("MPLBACKEND", "Agg")

import rates_cases as RC  # noqa: E402

import analyse.decay as rdecay  # noqa: E402
import analyse.rt60bands as rbands  # noqa: E402
import analyse.spectrogram as rspec  # noqa: E402
import analyse.waterfall as rwf  # noqa: E402
import analyse.modalcloud as rmodal  # noqa: E402
import analyse.frequency_response as rfr  # noqa: E402
import analyse.filterplot as rfilt  # noqa: E402

ARR = {}
META = {"numpy": np.__version__, "rates": list(RC.TABLE_RATES), "tables": {}, "degenerate": {}, "blocks": {}}


def fit_to_list(f):
    if f is None:
        return None
    return [f.range_db[0], f.range_db[1], f.start_time_seconds, f.end_time_seconds,
            f.slope_db_per_second, f.intercept_db, f.r_squared, f.rt60_seconds]


def reference_mask(freqs, band, nyq):
    if band.kind == "lowpass":
        return rbands._make_lowpass_mask(freqs, band.high_edge_hz, RC.TRANSITION_OCT, nyq)
    if band.kind == "highpass":
        return rbands._make_highpass_mask(freqs, band.low_edge_hz, RC.TRANSITION_OCT, nyq)
    return rbands._make_bandpass_mask(freqs, band.low_edge_hz, band.high_edge_hz, RC.TRANSITION_OCT, nyq)


def tables_and_masks():
    for sr in RC.TABLE_RATES:
        nyq = 0.5 * float(sr)
        for mode in RC.MODES:
            bands = rbands._build_band_definitions(rbands.Rt60BandsAnalysisSettings(band_mode=mode), sr)
            META["tables"][f"{sr}/{mode}"] = [[b.name, b.centre_hz, b.kind, b.low_edge_hz, b.high_edge_hz] for b in bands]
            deg = [i for i, b in enumerate(bands) if b.kind != "highpass" and float(np.clip(b.high_edge_hz, 1.0, nyq)) >= nyq]
            META["degenerate"][f"{sr}/{mode}"] = deg
            for n in RC.MASK_GOLDEN_LENGTHS:
                freqs = RC.axis(n, sr)
                for i in RC.golden_mask_bands(len(bands), deg):
                    m = reference_mask(freqs, bands[i], nyq)
                    assert m.dtype == np.float32 and m.size == n // 2 + 1
                    ARR[f"mask/{sr}/{mode}/{n}/{i}"] = m


def blocks():
    for sr in RC.BLOCK_RATES + RC.MODAL_ONLY_RATES:
        nyq = 0.5 * float(sr)
        ARR[f"modal/edges/{sr}"] = rmodal._build_log_bins(float(np.clip(20.0, 1.0, nyq)), float(np.clip(20000.0, 20.0, nyq)),
                                                          24, 24)
        for ci, x in enumerate(RC.block_channels(sr)):
            case = {}
            r = rmodal.analyse_modal_cloud_for_channel(x, sr, "mono", rmodal.ModalCloudAnalysisSettings())
            case["modal"] = dict(start=r.analysis_start_sample_index, length=r.analysis_length_samples,
                                 points=len(r.points), centres=[p.centre_hz for p in r.points])
            if sr in RC.BLOCK_RATES:
                r = rdecay.analyse_decay_for_channel(x, sr, "mono", rdecay.DecayAnalysisSettings(compute_edt=True))
                case["decay"] = dict(start=r.analysis_start_sample_index, n=int(r.edc_db.size),
                                     early=r.early_decay_10db_time_seconds,
                                     fits={k: fit_to_list(v) for k, v in r.fits.items()})
                for mode in RC.MODES:
                    s = rbands.Rt60BandsAnalysisSettings(band_mode=mode, include_t20=True, include_edt=True)
                    r = rbands.analyse_rt60_bands_for_channel(x, sr, "mono", s)
                    case[f"rt60bands/{mode}"] = dict(
                        metrics={k: [m.rt60_t30_seconds, m.rt60_t20_seconds, m.edt_seconds]
                                 for k, m in r.band_metrics_by_name.items()},
                        summary=rbands.summarise_rt60_bands_results_text([r], True, True))
                r = rfr.analyse_frequency_response_for_channel(x, sr, "mono", rfr.FrequencyResponseAnalysisSettings())
                case["fr"] = dict(start=r.analysis_start_sample_index, length=r.analysis_length_samples,
                                  peak=r.peak_frequency_hz, centroid=r.spectral_centroid_hz)
                r = rfilt.analyse_filter_response_for_channel(x, sr, "mono", rfilt.FilterAnalysisSettings())
                case["filter"] = dict(start=r.analysis_start_sample_index, length=r.analysis_length_samples,
                                      peak=r.peak_frequency_hz, mag1k=r.magnitude_at_1khz_db)
                r = rspec.analyse_spectrogram_for_channel(x, sr, "mono", rspec.SpectrogramAnalysisSettings())
                case["spectrogram"] = dict(start=r.analysis_start_sample_index, length=r.analysis_length_samples,
                                           shape=list(r.magnitude_db.shape))
                ws = rwf.WaterfallAnalysisSettings()
                r = rwf.analyse_waterfall_for_channel(x, sr, "mono", ws)
                frames = 1 + (r.analysis_length_samples - ws.n_fft) // ws.hop_length
                ft = (np.arange(frames, dtype=np.float32) * float(ws.hop_length) / float(sr)).astype(np.float32)
                idx = rwf._select_slice_frame_indices(ft, ws)
                assert np.array_equal(ft[idx], r.slice_times_seconds)
                case["waterfall"] = dict(start=r.analysis_start_sample_index, length=r.analysis_length_samples,
                                         slices=[int(v) for v in idx], f_first=float(r.frequency_hz[0]),
                                         f_last=float(r.frequency_hz[-1]), f_bins=int(r.frequency_hz.size))
                ARR[f"wf/times/{sr}/{ci}"] = r.slice_times_seconds
            META["blocks"][f"{sr}/{ci}"] = case


def write_npz(path, arrays):
    """numpy.savez_compressed with fixed member timestamps (the same arrays give the same bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    tables_and_masks()
    blocks()
    write_npz(HERE / "rates.npz", ARR)
    (HERE / "rates.json").write_text(json.dumps(META, indent=1, sort_keys=True) + "\n")
    tot = (HERE / "rates.npz").stat().st_size + (HERE / "rates.json").stat().st_size
    print(f"wrote {len(ARR)} arrays, {tot / 1e6:.3f} MB")


if __name__ == "__main__":
    main()
