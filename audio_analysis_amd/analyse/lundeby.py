"""
Lundeby noise-floor truncation and compensated decay times (ISO 3382-1, 5.3.3 and 6) per channel and band.

The decay fits of analyse.decay / analyse.rt60bands integrate the squared response to the last sample of the file, which
is right for noise-free responses and wrong for measured ones: the backward integration must stop where the decay meets
the background noise, and the energy that would have decayed after that point must be added.  The reference has nothing
of the kind.  This module estimates the noise level and the cross-point by Lundeby's iteration and fits EDT, T20 and T30
on the truncated, compensated Schroeder curve.  This text is the specification; tests/lundeby_ref.py restates it.

Rows.  Row 0 of a channel is its broadband signal from its start index s on, s = the first maximum of |x| (ira_peak_index,
as trim_to_peak of the decay block); the band rows are the rt60bands filter bank's full-file zero-phase band signals
(rt60bands.band_signals_device) from the same s.  y = the row from s on, L its length, e[n] = float64(y[n])**2.  Times below
are in samples, levels in dB, slopes in dB per sample.

1 Base blocks.  B = max(ceil(fs / 1000), ceil(L / 4096)), nb = L // B full blocks; a partial tail block takes no part in
  the estimate.  E[j] = sum e[j B .. (j + 1) B), float64, in an order that depends on the row alone (ira_block_energy).
2 Interval means of m blocks.  M[k] = sum(E[k m .. (k + 1) m)) / (m B), k < K = nb // m; the centre of interval k is
  (k + 0.5) m B.  D[k] = 10 log10(max(M[k], 1e-300) / max M); kmax = the first maximiser.  The level of a mean v is
  10 log10(max(v, 1e-300) / max M) likewise.
3 Preliminary pass.  m0 = max(1, floor(0.030 fs / B + 0.5)).  Noise level Ln = the level of the mean of the last
  max(1, K // 10) values of M.  kend = the first k > kmax with D[k] < Ln + 10.  A least-squares line D ~ slope t + c over
  the intervals kmax .. kend - 1 (at their centres) gives the cross-point tx = (Ln - c) / slope.
4 Re-averaging.  m1 = clamp(floor((-10 / slope) / 5 / B + 0.5), 1, max(1, nb // 16)): five intervals per 10 dB of decay.
  M, D and kmax are formed again with m = m1.
5 Iteration, at most 5 rounds.  The noise starts at min(tx + (-10 / slope), 0.9 nb B); Ln = the level of the mean of M from
  the first interval whose centre is at or after that point (the last interval if there is none).  k1 = the first
  k > kmax with D[k] < Ln + 10; k0 = the first k in [kmax, k1) with D[k] <= Ln + 30 (k1 if there is none), lowered to k1 - 3
  if fewer than 3 intervals remain.  The line over [k0, k1) gives the new tx; the iteration stops after the round in
  which tx moved by less than one interval m1 B.
6 Result.  t1 = clamp(floor(tx / B) B, B, nb B): the cut is block-aligned, the cross-point is no sharper than an interval.
  The level of the line at t1 is lev = max M * 10**((c + slope t1) / 10), the compensation C = lev * 10 / (-slope ln 10): the
  integral of the fitted exponential from t1 to infinity, in energy times samples.  Curve: edc[i] = C + sum e[i .. t1) for
  i < t1, then max(., eps) / max(edc[0], eps), 10 log10, max(., floor_db), float32: the steps and the edc_epsilon /
  edc_floor_db settings of ira_edc_db (ira_edc_truncated).  Mode "truncate" uses C = 0; "compensate" is the default.
7 Status (bit flags).  Checked in this order, the first that applies ends the row:
    2 too short (nb < 32); 16 non-finite (a block energy, the tail block's included, is not finite; or Ln, slope, c, C or
    tx is not); 1 silent (max E == 0); 4 no decay range (no interval below Ln + 10 after kmax, or fewer than 3 intervals to
    fit: kend - kmax < 3 in step 3, k1 - kmax < 3 in step 5); 8 slope not negative.
    32 no noise floor inside the file (tx >= nb B): the curve is the plain full-length EDC of all L samples with C = 0,
    fits are reported, the flag is informational.
  Any of bits 1 to 16 gives NaN in every output of that row; the batch carries on.
8 Validity (ISO 3382-1: the noise at least 10 dB below the lower fit limit).  Dynamic range = -Ln;
  edt_valid = (-Ln >= 20), t20_valid = (-Ln >= 35), t30_valid = (-Ln >= 45).

Fits are ira_curve_fits on the curve with the device-side lengths (Engine.curve_fits(lens_dev=...)): the ranges are
decay_fit_specs of the settings' DecayAnalysisSettings with compute_edt=True, crossings at 0 and -10 dB, 8 points at
least.  EDT, T20 and T30 are -60 / slope of their ranges' lines.

The start indices come to the host once per batch (one int64 per channel): the host sizes B from L.  The kernels read
them on the device.  A band row's curve is written over the band signal it came from (band signals handed to
lundeby_device are consumed); broadband curves get a buffer of their own.

Length limit.  A channel holds at most MAX_CHANNEL_SAMPLES = 2047 * 4096 samples (174.7 s at 48 kHz), the longest curve
ira_curve_fits takes.  A longer channel is an argument error (ValueError naming the channel's place in the batch) raised
before anything is launched, not a per-row status: cut the file first.

Command line (no plots): python -m analyse.lundeby --input A.wav [B.wav ...] | --bundle DIR [--mono]
  [--bands {none,three,octave,third}] [--mode {truncate,compensate}] [--expected-sample-rate 48000] [--json OUT.json]
"""
from __future__ import annotations

import argparse
import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..engine import LUNDEBY_DOUBLES, LUNDEBY_MAX_LEN
from . import _measure as M
from ._common import band_row_offsets
from ._measure import BAND_MODES
from .decay import DecayAnalysisSettings, decay_fit_specs
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ
from .rt60bands import BandDefinition, Rt60BandsAnalysisSettings, band_signals_device

STATUS_SILENT = 1
STATUS_TOO_SHORT = 2
STATUS_NO_RANGE = 4
STATUS_SLOPE = 8
STATUS_NON_FINITE = 16
STATUS_NO_FLOOR = 32
STATUS_ERROR_MASK = 31
_STATUS_WORDS = ((STATUS_SILENT, "silent"), (STATUS_TOO_SHORT, "too short"), (STATUS_NO_RANGE, "no decay range"),
                 (STATUS_SLOPE, "slope not negative"), (STATUS_NON_FINITE, "non-finite"),
                 (STATUS_NO_FLOOR, "no noise floor in file"))

MODES = ("truncate", "compensate")
MAX_BLOCKS = 4096
MIN_BLOCKS = 32
MAX_CHANNEL_SAMPLES = LUNDEBY_MAX_LEN
FIT_MIN_POINTS = 8
# record layout of ira_lundeby_estimate
(REC_STATUS, REC_LN, REC_T1, REC_SLOPE, REC_INTERCEPT, REC_C, REC_ROUNDS, REC_M1, REC_KMAX, REC_K0, REC_K1, REC_TX0, REC_TX,
 REC_MMAX, REC_EDC0, REC_NCURVE) = range(LUNDEBY_DOUBLES)


@dataclass(frozen=True)
class LundebySettings:
    mode: str = "compensate"
    decay: DecayAnalysisSettings = field(default_factory=lambda: DecayAnalysisSettings(compute_edt=True))
    bands: Optional[Rt60BandsAnalysisSettings] = field(default_factory=lambda: Rt60BandsAnalysisSettings(band_mode="octave"))
    use_mono_downmix_for_stereo: bool = False

    def __post_init__(self):
        if self.mode not in MODES:
            raise ValueError(f"Unknown mode: {self.mode} (expected one of {', '.join(MODES)})")
        if not isinstance(self.decay, DecayAnalysisSettings):
            raise ValueError("decay must be a DecayAnalysisSettings")
        if not self.decay.compute_edt:
            raise ValueError("decay.compute_edt must be True: EDT is one of the reported fits")
        if int(self.decay.edc_smoothing_window_samples or 0) > 1:
            raise ValueError("decay.edc_smoothing_window_samples is not supported on the truncated curve")
        eps, floor_db = float(self.decay.edc_epsilon), float(self.decay.edc_floor_db)
        if not (eps >= 0.0 and math.isfinite(eps)) or not math.isfinite(floor_db):
            raise ValueError("decay.edc_epsilon must be finite and >= 0 and decay.edc_floor_db finite")
        decay_fit_specs(self.decay)                                   # validates the ranges
        if self.bands is not None:
            if not isinstance(self.bands, Rt60BandsAnalysisSettings):
                raise ValueError("bands must be an Rt60BandsAnalysisSettings or None")
            if str(self.bands.band_mode).lower() not in BAND_MODES:
                raise ValueError(f"Unknown band_mode: {self.bands.band_mode} (expected one of {', '.join(BAND_MODES)})")

    @property
    def compensate(self) -> bool:
        return self.mode == "compensate"


@dataclass(frozen=True)
class LundebyValues:
    status: int
    noise_db: float                        # Ln, relative to the largest interval mean
    cross_point_seconds: float             # t1 / fs
    dynamic_range_db: float                # -Ln
    late_slope_db_per_second: float
    compensation_energy: float             # C
    edt_seconds: float
    t20_seconds: float
    t30_seconds: float
    edt_valid: bool
    t20_valid: bool
    t30_valid: bool


@dataclass(frozen=True)
class LundebyChannelResult:
    channel_name: str
    sample_rate_hz: int
    mode: str
    start_samples: int
    broadband: LundebyValues
    band_definitions: List[BandDefinition]
    band_values_by_name: Dict[str, LundebyValues]


@dataclass
class LundebyDevice:
    """What lundeby_device leaves behind.  Row c * (1 + nbands) + b is channel c's broadband signal (b = 0) or band b - 1."""
    bands: List[BandDefinition]
    start: np.ndarray                      # int64 (nch,) start indices
    block_size: np.ndarray                 # int32 (nrows,)
    nblk: np.ndarray                       # int32 (nrows,)
    records: object                        # float64 device (nrows, LUNDEBY_DOUBLES)
    lens_dev: object                       # int64 device (nrows,) curve lengths
    fits: object                           # float64 device (nrows, 3, 8): EDT, T20, T30
    cross: object                          # float64 device (nrows, 2): 0 and -10 dB crossings
    edc: object                            # float32 device view the curve offsets count from (the lowest of buffers)
    edc_off: np.ndarray                    # int64 (nrows,) offsets of the curves in edc
    specs: list
    buffers: tuple = ()                    # the device tensors that own the memory behind edc (samples, band curves,
                                           # broadband curves): the curves live as long as this object does


# ---------------------------------------------------------------------------------------------------
# host helpers
# ---------------------------------------------------------------------------------------------------


def block_size(sample_rate_hz: float, length: int) -> int:
    """B = max(ceil(fs / 1000), ceil(L / 4096)): blocks of at least 1 ms, at most 4096 of them."""
    return max(int(math.ceil(float(sample_rate_hz) / 1000.0)), -(-int(length) // MAX_BLOCKS), 1)


def first_interval_blocks(sample_rate_hz: float, b: int) -> int:
    """m0 = max(1, floor(0.030 fs / B + 0.5)): 30 ms intervals for the preliminary pass."""
    return max(1, int(math.floor(0.030 * float(sample_rate_hz) / float(b) + 0.5)))


def check_channel_lengths(lengths: Sequence[int]) -> None:
    """ValueError for a channel longer than MAX_CHANNEL_SAMPLES (the module docstring's length limit)."""
    for i, n in enumerate(lengths):
        if int(n) > MAX_CHANNEL_SAMPLES:
            raise ValueError(f"channel {i} of the batch has {int(n)} samples: at most {MAX_CHANNEL_SAMPLES} "
                             f"(2047 * 4096, 174.7 s at 48 kHz) per channel; cut the file first")


def row_tables(lengths: Sequence[int], starts: Sequence[int], sample_rate_hz: float, nbands: int):
    """(L, B, nb, m0) per channel from the channel lengths and start indices, and the same repeated for the 1 + nbands rows
    of every channel (int64, int32, int32, int32)."""
    ln = np.asarray(lengths, dtype=np.int64) - np.asarray(starts, dtype=np.int64)
    if np.any(ln < 0):
        raise ValueError("a start index lies behind the end of its channel")
    b = np.array([block_size(sample_rate_hz, v) for v in ln], dtype=np.int32)
    nb = (ln // np.maximum(b, 1)).astype(np.int32)
    m0 = np.array([first_interval_blocks(sample_rate_hz, v) for v in b], dtype=np.int32)
    rep = 1 + int(nbands)
    return ln, np.repeat(b, rep), np.repeat(nb, rep), np.repeat(m0, rep)


def validity(noise_db: float) -> Tuple[bool, bool, bool]:
    """(edt_valid, t20_valid, t30_valid) from Ln: the noise at least 10 dB below the lower fit limit (-10, -25, -35 dB)."""
    if not math.isfinite(noise_db):
        return False, False, False
    return -noise_db >= 20.0, -noise_db >= 35.0, -noise_db >= 45.0


def status_text(status: int) -> str:
    return M.status_text(status, _STATUS_WORDS)


def values_from_records(rec: np.ndarray, fits: np.ndarray, sample_rate_hz: float) -> LundebyValues:
    """One row: its estimate record (LUNDEBY_DOUBLES) and its three fit records (EDT, T20, T30; ira_curve_fits layout)."""
    nan = float("nan")
    status = int(rec[REC_STATUS])
    if status & STATUS_ERROR_MASK:
        return LundebyValues(status, nan, nan, nan, nan, nan, nan, nan, nan, False, False, False)
    fs = float(sample_rate_hz)
    ln = float(rec[REC_LN])
    rt = [float(f[6]) if f[0] == 1.0 else nan for f in fits]
    ev, v20, v30 = validity(ln)
    return LundebyValues(status, ln, float(rec[REC_T1]) / fs, -ln, float(rec[REC_SLOPE]) * fs, float(rec[REC_C]),
                         rt[0], rt[1], rt[2], ev, v20, v30)


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def lundeby_device(eng, batch, sample_rate_hz: int, settings: Optional[LundebySettings] = None,
                   band_signals=None) -> LundebyDevice:
    """
    Every channel of a device batch, broadband and per band: one launch each of ira_peak_index, ira_block_energy,
    ira_lundeby_estimate, ira_edc_truncated and ira_curve_fits over all rows.  band_signals = (bands, y device, y_off
    (nch, nbands)) as band_signals_device returns them lets a caller that already built the band signals skip the filter
    bank (they are overwritten by their curves); otherwise settings.bands decides which are built (None: broadband only).
    """
    settings = settings or LundebySettings()
    t = eng.torch
    nch = batch.count
    check_channel_lengths(batch.length)
    start_dev, _ = eng._batch_peak_pick(batch)
    start_dev = start_dev[:nch]
    if band_signals is None and settings.bands is not None:
        band_signals = band_signals_device(eng, batch, sample_rate_hz, settings.bands)
    bands = band_signals[0] if band_signals is not None else []
    nbands = len(bands)
    start = start_dev.cpu().numpy().astype(np.int64) if nch else np.zeros(0, np.int64)
    lens64 = batch.length.astype(np.int64)
    row_len, b, nb, m0 = row_tables(lens64, start, sample_rate_hz, nbands)
    bb_off = np.cumsum(row_len) - row_len                              # broadband curves: a buffer of their own
    bb = eng.empty(int(row_len.sum()), t.float32)
    owners = (batch.x, band_signals[1], bb) if nbands else (batch.x, bb)
    base, seg_off, edc_off = band_row_offsets(batch, band_signals, curves=(bb, bb_off, start))
    rep = 1 + nbands
    rows = eng.lundeby_rows(seg_off, np.repeat(lens64, rep), np.repeat(np.arange(nch, dtype=np.int32), rep), b, nb, m0)
    blk = eng.block_energy(base, rows, start_dev)
    rec, lens_dev, suffix = eng.lundeby_estimate(rows, start_dev, blk, settings.compensate)
    eng.edc_truncated(base, rows, start_dev, rec, lens_dev, suffix, settings.decay.edc_epsilon, settings.decay.edc_floor_db,
                      base, edc_off)
    specs, ranges = decay_fit_specs(settings.decay)
    upper = np.repeat(row_len, rep)
    fits, cross = eng.curve_fits(base, edc_off, upper, 1.0, float(sample_rate_hz), ranges, FIT_MIN_POINTS,
                                 cross=(0.0, -10.0), lens_dev=lens_dev)
    return LundebyDevice(bands=list(bands), start=start, block_size=b, nblk=nb, records=rec, lens_dev=lens_dev, fits=fits,
                         cross=cross, edc=base, edc_off=edc_off, specs=specs, buffers=owners)


def lundeby_results(dev: LundebyDevice, sample_rate_hz: int, channel_names: Sequence[str],
                    settings: LundebySettings) -> List[LundebyChannelResult]:
    nch, rep = len(channel_names), 1 + len(dev.bands)
    rec = dev.records.cpu().numpy().reshape(nch, rep, LUNDEBY_DOUBLES) if nch else np.zeros((0, rep, LUNDEBY_DOUBLES))
    fits = dev.fits.cpu().numpy().reshape(nch, rep, len(dev.specs), 8) if nch else np.zeros((0, rep, len(dev.specs), 8))
    out = []
    for ch, name in enumerate(channel_names):
        vals = [values_from_records(rec[ch, r], fits[ch, r], sample_rate_hz) for r in range(rep)]
        out.append(LundebyChannelResult(
            channel_name=str(name), sample_rate_hz=int(sample_rate_hz), mode=settings.mode, start_samples=int(dev.start[ch]),
            broadband=vals[0], band_definitions=list(dev.bands),
            band_values_by_name={b.name: vals[1 + i] for i, b in enumerate(dev.bands)}))
    return out


# ---------------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------------


def _results_of_batch(eng, batch, sample_rate_hz, names, settings) -> List[LundebyChannelResult]:
    return lundeby_results(lundeby_device(eng, batch, sample_rate_hz, settings), sample_rate_hz, names, settings)


def analyse_lundeby_batch(channels: Sequence[np.ndarray], sample_rate_hz: int, channel_names: Sequence[str],
                          settings: Optional[LundebySettings] = None) -> List[LundebyChannelResult]:
    """Every channel through the device in batches of at most MAX_BATCH_CHANNELS channels."""
    return M.analyse_channel_batches(channels, sample_rate_hz, channel_names, settings or LundebySettings(), _results_of_batch)


def analyse_lundeby_from_wav_file(input_wav_file_path: str | Path, settings: Optional[LundebySettings] = None,
                                  expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> List[LundebyChannelResult]:
    """One WAV file (mono or stereo, rate checked against expected_sample_rate_hz); channels named "mono", "left", "right"."""
    return M.analyse_wav_file_channels(input_wav_file_path, settings or LundebySettings(), expected_sample_rate_hz,
                                       analyse_lundeby_batch)


def analyse_lundeby_files(paths: Sequence[str | Path], settings: Optional[LundebySettings] = None,
                          expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> List[LundebyChannelResult]:
    """Every channel of every file, MAX_BATCH_CHANNELS channels per device batch; channels named "<file name>:<channel>"."""
    return M.analyse_file_channels(paths, settings or LundebySettings(), expected_sample_rate_hz, analyse_lundeby_batch)


def analyse_lundeby_bundle(bundle_root: str | Path, settings: Optional[LundebySettings] = None,
                           expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> List[LundebyChannelResult]:
    """The taps a bundle's meta.json lists (taps/<name>.wav), read by the native ingest (ingest.TapSet) a group at a time
    (at most MAX_BATCH_CHANNELS channels per group); channels named "<tap>:<channel>"."""
    return M.analyse_bundle_channels(bundle_root, settings or LundebySettings(), expected_sample_rate_hz, _results_of_batch)


# ---------------------------------------------------------------------------------------------------
# text, Markdown, JSON
# ---------------------------------------------------------------------------------------------------

_COLUMNS = ("Noise_dB", "Cross_ms", "Range_dB", "Slope_dB_s", "C", "EDT_s", "T20_s", "T30_s", "Valid", "Status")


def _valid_text(v: LundebyValues) -> str:
    names = [n for n, ok in (("EDT", v.edt_valid), ("T20", v.t20_valid), ("T30", v.t30_valid)) if ok]
    return "+".join(names) if names else "none"


def _cells(v: LundebyValues) -> List[str]:
    c = "NA" if math.isnan(v.compensation_energy) else f"{v.compensation_energy:.4e}"
    return [M.fmt(v.noise_db, 2), M.fmt(1000.0 * v.cross_point_seconds, 1), M.fmt(v.dynamic_range_db, 2),
            M.fmt(v.late_slope_db_per_second, 2), c, M.fmt(v.edt_seconds, 3), M.fmt(v.t20_seconds, 3), M.fmt(v.t30_seconds, 3),
            _valid_text(v), status_text(v.status)]


def _rows(r: LundebyChannelResult) -> List[List[str]]:
    return [[name] + _cells(v) for name, v in M.band_rows(r, r.band_values_by_name)]


def summarise_lundeby_text(channel_results: List[LundebyChannelResult]) -> str:
    """
    Fixed text format, one block per channel followed by an empty line:
        [<channel name>]
        Start: <s> samples (<s / fs in ms, 3 decimals> ms)  Mode: compensate | truncate
        Band  Noise_dB  Cross_ms  Range_dB  Slope_dB_s  C  EDT_s  T20_s  T30_s  Valid  Status
        Broadband  <Ln, 2 decimals>  <t1 in ms, 1 decimal>  <-Ln, 2>  <slope in dB/s, 2>  <C, 4 decimals exponent>
                   <EDT, T20, T30 in s, 3 decimals>  <EDT+T20+T30 | a subset | none>  ok | <flags> (<words>)
        <band name>  ...                       (one row per band, ascending)
    Cells are separated by two spaces; NaN is "NA".
    """
    return M.join_blocks(M.text_block(
        r.channel_name,
        f"Start: {r.start_samples} samples ({1000.0 * r.start_samples / r.sample_rate_hz:.3f} ms)  Mode: {r.mode}",
        _COLUMNS, _rows(r)) for r in channel_results)


def summarise_lundeby_markdown(channel_results: List[LundebyChannelResult]) -> str:
    """The same values as a Markdown section per channel: a '### <channel name>' heading, a start / mode line and a table
    with the columns of the text format, rows Broadband then the bands."""
    cols = ("Noise (dB)", "Cross-point (ms)", "Range (dB)", "Late slope (dB/s)", "C", "EDT (s)", "T20 (s)", "T30 (s)", "Valid",
            "Status")
    return M.join_blocks(M.markdown_block(
        r.channel_name,
        f"Start: {r.start_samples} samples ({1000.0 * r.start_samples / r.sample_rate_hz:.3f} ms). Mode: {r.mode}.",
        cols, _rows(r)) for r in channel_results)


_FLOAT_FIELDS = ("noise_db", "cross_point_seconds", "dynamic_range_db", "late_slope_db_per_second", "compensation_energy",
                 "edt_seconds", "t20_seconds", "t30_seconds")
_BOOL_FIELDS = ("edt_valid", "t20_valid", "t30_valid")


def _values_json(v: LundebyValues) -> Dict:
    d: Dict = {"status": v.status}
    for k in _FLOAT_FIELDS:
        d[k] = M.json_num(getattr(v, k))
    for k in _BOOL_FIELDS:
        d[k] = bool(getattr(v, k))
    return d


def _values_from_json(d: Dict) -> LundebyValues:
    return LundebyValues(status=int(d["status"]),
                         **{k: M.num_json(d[k]) for k in _FLOAT_FIELDS},
                         **{k: bool(d[k]) for k in _BOOL_FIELDS})


def lundeby_results_to_json(channel_results: List[LundebyChannelResult]) -> Dict:
    """Plain JSON: NaN is null."""
    rows = []
    for r in channel_results:
        rows.append({
            "channel_name": r.channel_name, "sample_rate_hz": r.sample_rate_hz, "mode": r.mode,
            "start_samples": r.start_samples, "broadband": _values_json(r.broadband),
            "bands": [M.band_to_json(b, _values_json(r.band_values_by_name[b.name])) for b in r.band_definitions],
        })
    return {"lundeby": rows}


def lundeby_results_from_json(doc: Dict) -> List[LundebyChannelResult]:
    out = []
    for d in doc["lundeby"]:
        out.append(LundebyChannelResult(
            channel_name=d["channel_name"], sample_rate_hz=int(d["sample_rate_hz"]), mode=str(d["mode"]),
            start_samples=int(d["start_samples"]), broadband=_values_from_json(d["broadband"]),
            band_definitions=M.bands_from_json(d["bands"]),
            band_values_by_name={b["name"]: _values_from_json(b) for b in d["bands"]}))
    return out


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.lundeby",
        description="Noise level, cross-point and EDT / T20 / T30 on the truncated, compensated Schroeder curve "
                    "(Lundeby's method, ISO 3382-1) per channel and band.  A channel holds at most "
                    f"{MAX_CHANNEL_SAMPLES} samples (174.7 s at 48 kHz); a longer file is refused.")
    M.add_source_arguments(p)
    M.add_bands_argument(p)
    p.add_argument("--mode", choices=list(MODES), default="compensate",
                   help="compensate: add the energy the decay would have had after the cross-point (default); "
                        "truncate: stop the integration there")
    M.add_output_arguments(p)
    return p


def settings_from_args(args) -> LundebySettings:
    bands = None if args.bands == "none" else Rt60BandsAnalysisSettings(band_mode=args.bands)
    return LundebySettings(mode=args.mode, bands=bands, use_mono_downmix_for_stereo=bool(args.mono))


def main(argv: Optional[Sequence[str]] = None) -> None:
    M.run_cli(build_parser(), argv, settings_from_args, analyse_lundeby_files, analyse_lundeby_bundle, summarise_lundeby_text,
              lundeby_results_to_json)


if __name__ == "__main__":
    main()
