"""
Dietsch-Kraak echo criterion EK per channel: is a late reflection an audible echo, for speech and for music.

The reference reports decay times only, and C80 / Ts (energy.py) integrate over the whole response: a strong reflection at
150 ms moves them a little and is not flagged.  EK (Dietsch & Kraak, Acustica 60, 1986) is the established
objective measure: the growth of the running centre time of |p|^n over a window.

Take a float32 signal y, the channel itself or one of its band signals, batch.length[c] samples long; o the channel's
broadband onset as in energy.py (ira_onset_index, onset_db = -20 by default); fs the sample rate.  A criterion is
(name, exponent n, window in ms, band edges or none, threshold_10, threshold_50).  Then

  s[m]  = float64(|y[o+m]|) ** n          m = 0 .. L-1, L = len(y) - o     (0 where y is 0)
  W[m]  = s[0] + ... + s[m]               V[m] = 0*s[0] + 1*s[1] + ... + m*s[m]
  ts[m] = V[m] / (fs * W[m])  seconds     (0 where W[m] == 0);  ts[m] = 0 for m < 0
  D     = max(1, floor(window_ms * fs / 1000.0 + 0.5))   samples          (lag_samples)
  EK[m] = (ts[m] - ts[m-D]) / (D / fs)    m = 0 .. M-1
  M     = min(L - G, Mmax)
  G     = ceil(end_guard_ms * fs / 1000.0)
  Mmax  = 1 + ceil(max_tau_ms * fs / 1000.0), or unbounded when max_tau_ms is None

Per channel and criterion: ek_max = max EK; tau_max_seconds = (first index of the maximum) / fs; first_tau_10_seconds and
first_tau_50_seconds = (first m with EK[m] >= threshold) / fs, NaN when there is none; a rating word: "inaudible"
(ek_max < threshold_10), "marginal" (>= threshold_10), "audible" (>= threshold_50); build_up_seconds = ts[M-1]; and, with
curve_step_ms > 0, the curve: for step k of S = max(1, floor(curve_step_ms * fs / 1000 + 0.5)) samples the float32 of
max EK[k S .. min((k+1) S, M) - 1].  All of it is formed on the device (ira_echo_criterion), M from the onset included:
the onset never returns to the host first.

The default criteria are the values commonly tabulated from Dietsch & Kraak -- speech: n = 2/3, 9 ms, 700-1400 Hz,
thresholds 0.9 / 1.0; music: n = 1, 14 ms, 700-2800 Hz, 1.5 / 1.8.  No copy of the paper was at hand, so they are the
defaults of a settings object, not constants of the kernel.  threshold_10 / threshold_50: the EK at which 10 % / 50 % of
listeners hear an echo.

Bands are BandDefinition(name, sqrt(lo * hi), "bandpass", lo, hi) through the mask records of rt60bands
(transition_width_octaves = 1/6): circular irfft(rfft(x) * mask) over the FULL file.  Criteria with equal edges share one
inverse transform; a criterion without edges reads the channel itself.  The masks are real, so the filters are zero-phase;
a reflection's pre-ring that falls in front of the onset is dropped, as in energy.py.

Why end_guard_ms exists (measured on the CPU with the oracle's masks): the filter bank is circular, so a band filter's
pre-ringing of the direct sound wraps to the END of the file.  With n < 2 compressing the dynamic range, that wrap-around
alone gave EK ~ 2.5 at 1994 ms of a 2 s synthetic response that has no echo at all.  The build-up sums are causal, so
ending the evaluation G samples before the end removes the artefact without touching any earlier value.  max_tau_ms is the
user's lever against a noisy tail (the evaluation limit is not coupled to the Lundeby cross-point).

Per-channel status (bit flags; a channel with a non-zero status has NaN in every value and the rating "NA", the batch
carries on): 1 silent (|x[peak]| == 0), 2 too short (M <= D for any criterion), 4 non-finite (any criterion's W[M-1] or
V[M-1] not finite).

Command line (no plots): python -m analyse.echo --input A.wav [B.wav ...] | --bundle DIR [--mono]
  [--criteria speech music] [--onset-db -20] [--max-tau-ms 1000] [--end-guard-ms 50] [--curve-step-ms 1]
  [--expected-sample-rate 48000] [--json OUT.json]
"""
from __future__ import annotations

import argparse
import math
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _measure as M
from ._common import band_row_offsets
from ._measure import MAX_BATCH_CHANNELS  # noqa: F401  (part of this module's surface)
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ
from .rt60bands import BandDefinition, Rt60BandsAnalysisSettings, band_signals_device

STATUS_SILENT = 1
STATUS_TOO_SHORT = 2
STATUS_NON_FINITE = 4
_STATUS_WORDS = ((STATUS_SILENT, "silent"), (STATUS_TOO_SHORT, "too short"), (STATUS_NON_FINITE, "non-finite"))

MAX_CRITERIA = 4
MAX_LAG_SAMPLES = 2048          # IRA_ECHO_MAX_LAG: the halo the kernel keeps; 14 ms at 96 kHz is 1344 samples
UNBOUNDED = 1 << 31             # Mmax when max_tau_ms is None: no segment is longer
TRANSITION_WIDTH_OCTAVES = 1.0 / 6.0
RATINGS = ("inaudible", "marginal", "audible")


@dataclass(frozen=True)
class EchoCriterion:
    name: str
    exponent: float
    window_ms: float
    band_hz: Optional[Tuple[float, float]]
    threshold_10: float
    threshold_50: float

    def __post_init__(self):
        if not isinstance(self.name, str) or not self.name.strip():
            raise ValueError("a criterion needs a non-empty name")
        n, w = float(self.exponent), float(self.window_ms)
        if not (math.isfinite(n) and n > 0.0):
            raise ValueError(f"exponent must be positive and finite, got {self.exponent}")
        if not (math.isfinite(w) and w > 0.0):
            raise ValueError(f"window_ms must be positive and finite, got {self.window_ms}")
        band = self.band_hz
        if band is not None:
            try:
                lo, hi = (float(v) for v in band)
            except (TypeError, ValueError):
                raise ValueError("band_hz must be (low edge, high edge) in Hz or None") from None
            if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo < hi):
                raise ValueError(f"band_hz must be 0 < low edge < high edge, got {band}")
            band = (lo, hi)
        t10, t50 = float(self.threshold_10), float(self.threshold_50)
        if not (math.isfinite(t10) and math.isfinite(t50)):
            raise ValueError(f"thresholds must be finite, got {self.threshold_10}, {self.threshold_50}")
        if t50 < t10:
            raise ValueError(f"threshold_50 must not lie below threshold_10, got {t10}, {t50}")
        for k, v in (("exponent", n), ("window_ms", w), ("band_hz", band), ("threshold_10", t10), ("threshold_50", t50)):
            object.__setattr__(self, k, v)

    def rating(self, ek_max: float) -> str:
        if math.isnan(ek_max):
            return "NA"
        return "audible" if ek_max >= self.threshold_50 else ("marginal" if ek_max >= self.threshold_10 else "inaudible")


SPEECH = EchoCriterion("speech", 2.0 / 3.0, 9.0, (700.0, 1400.0), 0.9, 1.0)
MUSIC = EchoCriterion("music", 1.0, 14.0, (700.0, 2800.0), 1.5, 1.8)
CRITERIA = {c.name: c for c in (SPEECH, MUSIC)}


@dataclass(frozen=True)
class EchoCriterionSettings:
    criteria: Tuple[EchoCriterion, ...] = (SPEECH, MUSIC)
    onset_db: float = -20.0
    max_tau_ms: Optional[float] = 1000.0
    end_guard_ms: float = 50.0
    curve_step_ms: float = 1.0                     # 0: no curve
    use_mono_downmix_for_stereo: bool = False

    def __post_init__(self):
        try:
            crit = tuple(self.criteria)
        except TypeError:
            raise ValueError(f"criteria must be a sequence of 1 to {MAX_CRITERIA} EchoCriterion") from None
        if not 1 <= len(crit) <= MAX_CRITERIA:
            raise ValueError(f"criteria needs 1 to {MAX_CRITERIA} entries, got {len(crit)}")
        if not all(isinstance(c, EchoCriterion) for c in crit):
            raise ValueError("criteria must hold EchoCriterion objects")
        if len({c.name for c in crit}) != len(crit):
            raise ValueError(f"criteria names must be unique, got {[c.name for c in crit]}")
        onset = float(self.onset_db)
        if not math.isfinite(onset) or onset > 0.0:
            raise ValueError(f"onset_db must be a finite level <= 0 dB relative to the peak, got {self.onset_db}")
        tau = self.max_tau_ms
        if tau is not None:
            tau = float(tau)
            if not (math.isfinite(tau) and tau > 0.0):
                raise ValueError(f"max_tau_ms must be positive and finite, or None, got {self.max_tau_ms}")
        guard, step = float(self.end_guard_ms), float(self.curve_step_ms)
        if not (math.isfinite(guard) and guard >= 0.0):
            raise ValueError(f"end_guard_ms must be finite and >= 0, got {self.end_guard_ms}")
        if not (math.isfinite(step) and step >= 0.0):
            raise ValueError(f"curve_step_ms must be finite and >= 0 (0: no curve), got {self.curve_step_ms}")
        for k, v in (("criteria", crit), ("onset_db", onset), ("max_tau_ms", tau), ("end_guard_ms", guard),
                     ("curve_step_ms", step)):
            object.__setattr__(self, k, v)

    @property
    def rel_energy(self) -> float:
        return 10.0 ** (self.onset_db / 10.0)


@dataclass(frozen=True)
class EchoCriterionValues:
    ek_max: float
    tau_max_seconds: float
    first_tau_10_seconds: float                    # NaN: EK never reaches threshold_10
    first_tau_50_seconds: float
    rating: str                                    # inaudible | marginal | audible | NA
    build_up_seconds: float                        # ts[M-1]
    curve: Optional[Tuple[float, ...]] = None      # max EK per step of curve_step_seconds; None: not computed


@dataclass(frozen=True)
class EchoCriterionChannelResult:
    channel_name: str
    sample_rate_hz: int
    onset_samples: int
    onset_seconds: float
    status: int
    criteria: Tuple[EchoCriterion, ...]
    curve_step_seconds: float                      # S / fs; 0 without a curve
    values_by_name: Dict[str, EchoCriterionValues]


@dataclass
class EchoRecords:
    """What echo_criterion_device leaves on the host: per channel the onset and |x[peak]|, per (channel, criterion) the
    kernel's record [EK_max, its index, first index >= threshold_10 (-1: none), the same for threshold_50, ts[M-1],
    W[M-1], M, V[M-1]] and the curve."""
    criteria: Tuple[EchoCriterion, ...]
    length: np.ndarray                             # int64 (nch,)
    onset: np.ndarray                              # int64 (nch,)
    peak_abs: np.ndarray                           # float32 (nch,)
    records: np.ndarray                            # float64 (nch, ncrit, 8)
    curve: Optional[np.ndarray]                    # float32 (nch, ncrit, ncurve), NaN past a row's range; None: no curve
    lag: np.ndarray                                # int64 (ncrit,) D
    step: int                                      # S; 0 without a curve


def lag_samples(window_ms: float, sample_rate_hz: float) -> int:
    """D = max(1, floor(window_ms * fs / 1000 + 0.5)) samples, float64 in exactly that order (9 ms: 198 / 397 / 432 / 864 at
    22.05 / 44.1 / 48 / 96 kHz)."""
    return max(1, int(math.floor(float(window_ms) * float(sample_rate_hz) / 1000.0 + 0.5)))


def guard_samples(end_guard_ms: float, sample_rate_hz: float) -> int:
    return int(math.ceil(float(end_guard_ms) * float(sample_rate_hz) / 1000.0))


def max_samples(max_tau_ms: Optional[float], sample_rate_hz: float) -> int:
    """Mmax = 1 + ceil(max_tau_ms * fs / 1000): the evaluation reaches tau = max_tau_ms; None: unbounded."""
    if max_tau_ms is None:
        return UNBOUNDED
    return min(UNBOUNDED, 1 + int(math.ceil(float(max_tau_ms) * float(sample_rate_hz) / 1000.0)))


def curve_step_samples(curve_step_ms: float, sample_rate_hz: float) -> int:
    if curve_step_ms <= 0.0:
        return 0
    return max(1, int(math.floor(float(curve_step_ms) * float(sample_rate_hz) / 1000.0 + 0.5)))


def criterion_params(criterion: EchoCriterion, sample_rate_hz: float, settings: "EchoCriterionSettings") -> List[float]:
    """The kernel's parameter set of one criterion at one sample rate: [n, D, G, Mmax, S, threshold_10, threshold_50, fs]."""
    d = lag_samples(criterion.window_ms, sample_rate_hz)
    if d > MAX_LAG_SAMPLES:
        raise ValueError(f"window_ms {criterion.window_ms:g} is {d} samples at {sample_rate_hz:g} Hz: at most {MAX_LAG_SAMPLES}")
    return [criterion.exponent, float(d), float(guard_samples(settings.end_guard_ms, sample_rate_hz)),
            float(max_samples(settings.max_tau_ms, sample_rate_hz)),
            float(curve_step_samples(settings.curve_step_ms, sample_rate_hz)), criterion.threshold_10,
            criterion.threshold_50, float(sample_rate_hz)]


def criterion_bands(criteria: Sequence[EchoCriterion]) -> Tuple[List[BandDefinition], List[int]]:
    """(the distinct bands of the criteria in order of first use, per criterion its signal row: 0 = the channel itself,
    1 + i = band i).  Criteria with equal edges share a band, hence one inverse transform."""
    bands: List[BandDefinition] = []
    edges: List[Tuple[float, float]] = []
    rows = []
    for c in criteria:
        if c.band_hz is None:
            rows.append(0)
            continue
        if c.band_hz not in edges:
            lo, hi = c.band_hz
            edges.append(c.band_hz)
            bands.append(BandDefinition(f"{lo:g}-{hi:g}Hz", math.sqrt(lo * hi), "bandpass", lo, hi))
        rows.append(1 + edges.index(c.band_hz))
    return bands, rows


def status_text(status: int) -> str:
    return M.status_text(status, _STATUS_WORDS)


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def echo_criterion_device(eng, batch, sample_rate_hz: int, settings: Optional[EchoCriterionSettings] = None,
                          band_signals=None) -> EchoRecords:
    """
    Onset, records and curves of every channel of a device batch for every criterion, in ONE ira_echo_criterion launch.
    band_signals = (bands, y device, y_off (nch, nbands)) as band_signals_device returns them for criterion_bands' list
    lets a caller that already built the band signals skip the filter bank.
    """
    settings = settings or EchoCriterionSettings()
    crit = settings.criteria
    nch, nc = batch.count, len(crit)
    params = np.asarray([criterion_params(c, sample_rate_hz, settings) for c in crit], dtype=np.float64)
    onset_dev, _, peak_abs_dev = eng.onset_index(batch, settings.rel_energy)
    bands, rows = criterion_bands(crit)
    if band_signals is None and bands:
        band_signals = band_signals_device(
            eng, batch, sample_rate_hz, Rt60BandsAnalysisSettings(transition_width_octaves=TRANSITION_WIDTH_OCTAVES),
            bands=bands)
    nb = len(bands)
    if band_signals is not None and len(band_signals[0]) != nb:
        raise ValueError("band_signals must hold the bands of criterion_bands(settings.criteria)")
    # signal rows: channel c's own samples, then its bands (row c * (1 + nb) + b); segment (c, k) reads criterion k's row
    base, row_off = band_row_offsets(batch, band_signals if nb else None)
    seg_off = np.asarray(row_off, dtype=np.int64).reshape(nch, 1 + nb)[:, rows].reshape(-1)
    seg_len = np.repeat(batch.length.astype(np.int64), nc)
    chan = np.repeat(np.arange(nch, dtype=np.int32), nc)
    step = int(params[0, 4])
    if nch:
        rec_dev, curve_dev = eng.echo_criterion(base, seg_off, seg_len, chan, onset_dev, params,
                                                np.tile(np.arange(nc, dtype=np.int32), nch))
        records = rec_dev.cpu().numpy().reshape(nch, nc, 8)
        curve = curve_dev.cpu().numpy().reshape(nch, nc, -1) if step else None
    else:
        records, curve = np.zeros((0, nc, 8)), (np.zeros((0, nc, 0), np.float32) if step else None)
    return EchoRecords(criteria=crit, length=batch.length.astype(np.int64).copy(), onset=onset_dev.cpu().numpy().copy(),
                       peak_abs=peak_abs_dev.cpu().numpy().copy(), records=records, curve=curve,
                       lag=params[:, 1].astype(np.int64), step=step)


# ---------------------------------------------------------------------------------------------------
# host: records -> results
# ---------------------------------------------------------------------------------------------------


def _nan_values(with_curve: bool, ncurve: int) -> EchoCriterionValues:
    nan = float("nan")
    return EchoCriterionValues(nan, nan, nan, nan, "NA", nan, tuple([nan] * ncurve) if with_curve else None)


def echo_criterion_results(res: EchoRecords, sample_rate_hz: int, channel_names: Sequence[str]) -> List[EchoCriterionChannelResult]:
    fs = float(sample_rate_hz)
    out = []
    for ch, name in enumerate(channel_names):
        rec = res.records[ch]
        m = rec[:, 6]
        status = 0
        if float(res.peak_abs[ch]) == 0.0:
            status |= STATUS_SILENT
        if np.any(m <= res.lag):
            status |= STATUS_TOO_SHORT
        if not (np.all(np.isfinite(rec[:, 5])) and np.all(np.isfinite(rec[:, 7]))):
            status |= STATUS_NON_FINITE
        values = {}
        for k, c in enumerate(res.criteria):
            ncurve = int(math.ceil(max(float(m[k]), 0.0) / res.step)) if res.step else 0
            if status:
                values[c.name] = _nan_values(res.curve is not None, ncurve)
                continue
            r = rec[k]
            values[c.name] = EchoCriterionValues(
                ek_max=float(r[0]), tau_max_seconds=float(r[1]) / fs,
                first_tau_10_seconds=float(r[2]) / fs if r[2] >= 0 else float("nan"),
                first_tau_50_seconds=float(r[3]) / fs if r[3] >= 0 else float("nan"),
                rating=c.rating(float(r[0])), build_up_seconds=float(r[4]),
                curve=tuple(float(v) for v in res.curve[ch, k, :ncurve]) if res.curve is not None else None)
        onset = int(res.onset[ch])
        out.append(EchoCriterionChannelResult(
            channel_name=str(name), sample_rate_hz=int(sample_rate_hz), onset_samples=onset, onset_seconds=onset / fs,
            status=status, criteria=tuple(res.criteria), curve_step_seconds=res.step / fs, values_by_name=values))
    return out


# ---------------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------------


def _results_of_batch(eng, batch, sample_rate_hz, names, settings) -> List[EchoCriterionChannelResult]:
    return echo_criterion_results(echo_criterion_device(eng, batch, sample_rate_hz, settings), sample_rate_hz, names)


def analyse_echo_criterion_batch(
    channels: Sequence[np.ndarray],
    sample_rate_hz: int,
    channel_names: Sequence[str],
    settings: Optional[EchoCriterionSettings] = None,
) -> List[EchoCriterionChannelResult]:
    """Every channel through the device in batches of at most MAX_BATCH_CHANNELS channels."""
    return M.analyse_channel_batches(channels, sample_rate_hz, channel_names, settings or EchoCriterionSettings(),
                                     _results_of_batch)


def analyse_echo_criterion_from_wav_file(
    input_wav_file_path: str | Path,
    settings: Optional[EchoCriterionSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[EchoCriterionChannelResult]:
    """One WAV file (mono or stereo, rate checked against expected_sample_rate_hz); channels named as by
    get_analysis_channels ("mono", "left", "right")."""
    return M.analyse_wav_file_channels(input_wav_file_path, settings or EchoCriterionSettings(), expected_sample_rate_hz,
                                       analyse_echo_criterion_batch)


def analyse_echo_criterion_files(
    paths: Sequence[str | Path],
    settings: Optional[EchoCriterionSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[EchoCriterionChannelResult]:
    """Every channel of every file in one device batch per MAX_BATCH_CHANNELS channels; channels named
    "<file name>:<channel>"."""
    return M.analyse_file_channels(paths, settings or EchoCriterionSettings(), expected_sample_rate_hz,
                                   analyse_echo_criterion_batch)


def analyse_echo_criterion_bundle(
    bundle_root: str | Path,
    settings: Optional[EchoCriterionSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[EchoCriterionChannelResult]:
    """The taps a bundle's meta.json lists (taps/<name>.wav), read by the native ingest (ingest.TapSet) a group at a
    time; channels named "<tap>:<channel>"."""
    return M.analyse_bundle_channels(bundle_root, settings or EchoCriterionSettings(), expected_sample_rate_hz,
                                     _results_of_batch)


# ---------------------------------------------------------------------------------------------------
# text, Markdown, JSON
# ---------------------------------------------------------------------------------------------------


def _cells(v: EchoCriterionValues) -> List[str]:
    return [M.fmt(v.ek_max, 3), M.fmt(1000.0 * v.tau_max_seconds, 2), M.fmt(1000.0 * v.first_tau_10_seconds, 2),
            M.fmt(1000.0 * v.first_tau_50_seconds, 2), v.rating]


def _rows(r: EchoCriterionChannelResult) -> List[List[str]]:
    return [[c.name] + _cells(r.values_by_name[c.name]) for c in r.criteria]


def summarise_echo_criterion_text(channel_results: List[EchoCriterionChannelResult]) -> str:
    """
    Fixed text format, one block per channel followed by an empty line:
        [<channel name>]
        Onset: <o> samples (<o / fs in ms, 3 decimals> ms)  Status: ok | <flags> (<words>)
        Criterion  EK_max  tau_max_ms  tau_10_ms  tau_50_ms  Rating
        <criterion name>  <EK_max, 3 decimals>  <ms, 2 decimals>  <ms>  <ms>  inaudible | marginal | audible | NA
    Cells are separated by two spaces; NaN (no crossing, or a channel with a status) is "NA".
    """
    return M.join_blocks(M.text_block(
        r.channel_name, f"Onset: {r.onset_samples} samples ({1000.0 * r.onset_seconds:.3f} ms)  Status: {status_text(r.status)}",
        ["EK_max", "tau_max_ms", "tau_10_ms", "tau_50_ms", "Rating"], _rows(r), first="Criterion") for r in channel_results)


def summarise_echo_criterion_markdown(channel_results: List[EchoCriterionChannelResult]) -> str:
    """The same values as a Markdown section per channel: a '### <channel name>' heading, an onset / status line and a
    table with a row per criterion."""
    return M.join_blocks(M.markdown_block(
        r.channel_name, f"Onset: {r.onset_samples} samples ({1000.0 * r.onset_seconds:.3f} ms). Status: {status_text(r.status)}.",
        ["EK_max", "tau_max (ms)", "tau_10 (ms)", "tau_50 (ms)", "Rating"], _rows(r), first="Criterion")
        for r in channel_results)


def _criterion_json(c: EchoCriterion) -> Dict:
    return {"name": c.name, "exponent": c.exponent, "window_ms": c.window_ms,
            "band_hz": list(c.band_hz) if c.band_hz is not None else None, "threshold_10": c.threshold_10,
            "threshold_50": c.threshold_50}


def _values_json(v: EchoCriterionValues) -> Dict:
    d = {"ek_max": M.json_num(v.ek_max), "tau_max_seconds": M.json_num(v.tau_max_seconds),
         "first_tau_10_seconds": M.json_num(v.first_tau_10_seconds),
         "first_tau_50_seconds": M.json_num(v.first_tau_50_seconds), "rating": v.rating,
         "build_up_seconds": M.json_num(v.build_up_seconds)}
    if v.curve is not None:                                   # the curve is in the JSON only when it was computed
        d["curve"] = [M.json_num(x) for x in v.curve]
    return d


def _values_from_json(d: Dict) -> EchoCriterionValues:
    return EchoCriterionValues(M.num_json(d["ek_max"]), M.num_json(d["tau_max_seconds"]), M.num_json(d["first_tau_10_seconds"]),
                               M.num_json(d["first_tau_50_seconds"]), str(d["rating"]), M.num_json(d["build_up_seconds"]),
                               tuple(M.num_json(x) for x in d["curve"]) if "curve" in d else None)


def echo_results_to_json(channel_results: List[EchoCriterionChannelResult]) -> Dict:
    """Plain JSON: NaN is null."""
    rows = []
    for r in channel_results:
        rows.append({
            "channel_name": r.channel_name, "sample_rate_hz": r.sample_rate_hz, "onset_samples": r.onset_samples,
            "onset_seconds": r.onset_seconds, "status": r.status, "curve_step_seconds": r.curve_step_seconds,
            "criteria": [dict(_criterion_json(c), **_values_json(r.values_by_name[c.name])) for c in r.criteria],
        })
    return {"echo_criterion": rows}


def echo_results_from_json(doc: Dict) -> List[EchoCriterionChannelResult]:
    out = []
    for d in doc["echo_criterion"]:
        crit = tuple(EchoCriterion(c["name"], c["exponent"], c["window_ms"],
                                   tuple(c["band_hz"]) if c["band_hz"] is not None else None, c["threshold_10"],
                                   c["threshold_50"]) for c in d["criteria"])
        out.append(EchoCriterionChannelResult(
            channel_name=d["channel_name"], sample_rate_hz=int(d["sample_rate_hz"]), onset_samples=int(d["onset_samples"]),
            onset_seconds=float(d["onset_seconds"]), status=int(d["status"]), criteria=crit,
            curve_step_seconds=float(d["curve_step_seconds"]),
            values_by_name={c["name"]: _values_from_json(c) for c in d["criteria"]}))
    return out


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.echo",
        description="Dietsch-Kraak echo criterion EK per channel: maximum, its delay, first threshold crossings and a rating.")
    M.add_source_arguments(p)
    p.add_argument("--criteria", nargs="+", choices=sorted(CRITERIA), default=["speech", "music"],
                   help="criteria to evaluate (default: speech music)")
    p.add_argument("--onset-db", type=float, default=-20.0,
                   help="onset: first sample within this level of the peak (default: -20 dB, ISO 3382-1)")
    p.add_argument("--max-tau-ms", type=float, default=1000.0,
                   help="evaluate up to this delay after the onset (default: 1000 ms); the lever against a noisy tail")
    p.add_argument("--end-guard-ms", type=float, default=50.0,
                   help="leave out this much of the end of the file, where circular band filters wrap (default: 50 ms)")
    p.add_argument("--curve-step-ms", type=float, default=1.0,
                   help="step of the EK curve written to the JSON (default: 1 ms; 0: no curve)")
    M.add_output_arguments(p)
    return p


def settings_from_args(args) -> EchoCriterionSettings:
    return EchoCriterionSettings(criteria=tuple(CRITERIA[n] for n in args.criteria), onset_db=args.onset_db,
                                 max_tau_ms=args.max_tau_ms, end_guard_ms=args.end_guard_ms,
                                 curve_step_ms=args.curve_step_ms, use_mono_downmix_for_stereo=bool(args.mono))


def main(argv: Optional[Sequence[str]] = None) -> None:
    M.run_cli(build_parser(), argv, settings_from_args, analyse_echo_criterion_files, analyse_echo_criterion_bundle,
              summarise_echo_criterion_text, echo_results_to_json)


if __name__ == "__main__":
    main()
