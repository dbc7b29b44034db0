"""
Multi-slope decay fits (coupled rooms) per channel and band: sums of exponentials plus a noise term on the Schroeder curve.

Every other decay figure of this package (EDT, T20, T30, the band bank, Lundeby's truncated curve, the modal cloud) assumes one
exponential.  Coupled volumes (a stage house behind a proscenium, a reverberation chamber beside a hall, a nave with side
chapels) do not decay that way: their Schroeder curve bends, T20 and T30 disagree and one number describes neither part.
This module fits the accepted model, a sum of one to three exponentials plus a noise term on the Schroeder curve (Xiang
and Goggans 2001; Xiang et al. 2011), by an exhaustive search over a grid of decay times that is refined around the winner.
The reference has nothing of the kind.  This text is the specification; tests/multislope_ref.py restates it.

Rows.  As in analyse.lundeby: row 0 of a channel is its broadband signal from its start index s on, s = the first maximum
of |x| (ira_peak_index); the band rows are the rt60bands filter bank's full-file zero-phase band signals
(rt60bands.band_signals_device) from the same s.  L = the row's length, B = lundeby.block_size(fs, L), nb = L // B;
E[0 .. nb) and the partial tail block's energy come from ira_block_energy.  Times are in samples unless seconds are named.

1 Points.  d[j] = tail + E[nb - 1] + ... + E[j], float64, summed from the end, j < nb.  J = max(1, floor(fit_fraction nb)),
  the product rounded to float64; fit_fraction defaults to 0.9, 0 < fit_fraction <= 1.  t_j = j B.  The last tenth of the file
  is left out: there the curve runs into its own upper integration limit and relative errors mean nothing.
2 Basis.  For a decay time T in seconds lambda = ln(10^6) / (T fs) and phi_T(t) = exp(-lambda t) - exp(-lambda L); the noise
  term is nu(t) = (L - t) / L.  Model: m(t) = sum_s a_s phi_{T_s}(t) + a_nu nu(t).  Residuals are relative (the linear
  stand-in for a fit of the dB curve): u_i[j] = phi_{T_i}(t_j) / d[j], u_nu[j] = nu(t_j) / d[j], and the coefficients minimise
  sum_{j < J} (sum_i a_i u_i[j] - 1)^2.
3 Gram.  For a grid of g <= 128 ascending decay times: G_ik = sum_j u_i[j] u_k[j] and b_i = sum_j u_i[j] over the g + 1
  functions, the noise term last.  Float64 sums in ascending j, an order that depends on the row alone.
4 Candidates of order S (1, 2 or 3).  Grid indices i_1 < ... < i_S with T[i_{k+1}] >= min_ratio T[i_k] (min_ratio defaults to
  1.5 and must exceed 1), each tried once with the noise term and once without.  The S (+ 1) normal equations are solved by
  Cholesky, the functions in the order i_1 .. i_S, noise.  A candidate is inadmissible if a pivot (the diagonal entry less
  the squares of its row of the factor so far) is <= 1e-12 times that diagonal entry, or if any coefficient is <= 0 or not
  finite.  Cost c = max(J - b^T a, 0).  The winner has the smallest c; on an exact tie the earlier candidate wins, in
  lexicographic index order with the noise variant first.
5 Levels.  Level 0 is the same grid for every row: T_k = t_min (t_max / t_min)^(k / (G - 1)), k < G (defaults t_min 0.05 s,
  t_max 20 s, G = 64), its step h_0 = ln(t_max / t_min) / (G - 1).  Levels 1 .. refine_levels (default 3) are per row and
  order: h_l = h_{l-1} / (R + 1) with R = 3, and the grid is the ascending union (equal values once), over the previous
  winner's slopes, of T_s exp(k h_l), k = -R .. R: at most 21 points, the previous winner among them (k = 0).  Only that
  order is searched.  The final step, 0.15 % of T with the defaults, is the stated resolution of the result.
6 Per order, from the last level's winner: T_s ascending, a_s, a_nu (0 if the winner has no noise term);
  rms_db = (10 / ln 10) sqrt(c / J); the start level of slope s, 10 log10(a_s phi_{T_s}(0) / d[0]); the noise share
  10 log10(a_nu / d[0]) (-inf if a_nu is 0); for S >= 2 the turning point between slopes s and s + 1,
  t_x = ln(a_s / a_{s+1}) / (lambda_s - lambda_{s+1}) in seconds (NaN if it is not > 0) and the level there,
  10 log10(a_s exp(-lambda_s t_x) / d[0]).  Host arithmetic from the device record.
7 Preferred order.  The smallest S <= max_order (default 3) whose rms_db <= accept_rms_db (default 0.15 dB), otherwise
  the largest fitted order.  accept_rms_db is a user setting, not a measured constant: on synthetic decays a single slope
  fits to 0.03 dB while a 0.4 s / 1.5 s pair fitted as one slope leaves 0.46 dB.  Every order's fit is reported, so the
  reader can judge.  (BIC is not used: the points of a Schroeder curve are strongly correlated.)
8 Status (bit flags).  Checked in this order, the first that applies ends the row and every output of it is NaN:
    2 too short (nb < 32); 16 non-finite (a block energy or the tail is not finite); 1 silent (d[0] == 0);
    4 digital silence inside the fit range (d[J - 1] == 0).
  Per order "no admissible candidate", 32 for order 1, 64 for order 2, 128 for order 3: the constraints leave no candidate
  or every candidate is inadmissible.  That order is NaN, the other orders stand; the batch always carries on.

Length limit.  A channel holds at most MAX_CHANNEL_SAMPLES samples, as in analyse.lundeby: a longer channel is a ValueError
raised before anything is launched.

Kernels (ira_multislope.hip): ira_multislope_points once, then per level ira_multislope_gram and ira_multislope_search;
the search writes the next level's grids on the device, the levels chain without a host round trip.

Command line (no plots): python -m analyse.multislope --input A.wav [B.wav ...] | --bundle DIR [--mono]
  [--bands {none,three,octave,third}] [--max-order 3] [--t-min 0.05] [--t-max 20] [--grid 64] [--refine-levels 3]
  [--min-ratio 1.5] [--fit-fraction 0.9] [--accept-rms-db 0.15] [--expected-sample-rate 48000] [--json OUT.json]
"""
from __future__ import annotations

import argparse
import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..engine import MS_DOUBLES, MS_MAX_GRID, MS_MAX_ORDER, MS_REFINE_R, MS_REFINED
from . import _measure as M
from ._common import band_row_offsets
from ._measure import BAND_MODES
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ
from .lundeby import MAX_CHANNEL_SAMPLES, check_channel_lengths, row_tables
from .rt60bands import BandDefinition, Rt60BandsAnalysisSettings, band_signals_device

STATUS_SILENT = 1
STATUS_TOO_SHORT = 2
STATUS_ZERO_IN_RANGE = 4
STATUS_NON_FINITE = 16
STATUS_NO_CANDIDATE = 32                   # << (order - 1)
STATUS_ERROR_MASK = 23
_STATUS_WORDS = ((STATUS_SILENT, "silent"), (STATUS_TOO_SHORT, "too short"), (STATUS_ZERO_IN_RANGE, "silence in fit range"),
                 (STATUS_NON_FINITE, "non-finite"), (32, "no order-1 candidate"), (64, "no order-2 candidate"),
                 (128, "no order-3 candidate"))
LN_1E6 = math.log(1e6)
# record layout of ira_multislope_search
REC_STATUS, REC_J, REC_NOISE, REC_COST, REC_INDEX, REC_T, REC_A, REC_A_NOISE, REC_D0, REC_G = 0, 1, 2, 3, 4, 7, 10, 13, 14, 15


@dataclass(frozen=True)
class MultiSlopeSettings:
    max_order: int = 3
    t_min: float = 0.05
    t_max: float = 20.0
    grid: int = 64
    refine_levels: int = 3
    min_ratio: float = 1.5
    fit_fraction: float = 0.9
    accept_rms_db: float = 0.15
    bands: Optional[Rt60BandsAnalysisSettings] = field(default_factory=lambda: Rt60BandsAnalysisSettings(band_mode="octave"))
    use_mono_downmix_for_stereo: bool = False

    def __post_init__(self):
        if not (isinstance(self.max_order, int) and 1 <= self.max_order <= MS_MAX_ORDER):
            raise ValueError(f"max_order must be 1 .. {MS_MAX_ORDER}")
        if not (isinstance(self.grid, int) and 1 <= self.grid <= MS_MAX_GRID):
            raise ValueError(f"grid must be 1 .. {MS_MAX_GRID} decay times")
        if not (math.isfinite(self.t_min) and math.isfinite(self.t_max) and 0.0 < self.t_min <= self.t_max):
            raise ValueError("t_min and t_max must be finite with 0 < t_min <= t_max")
        if self.grid > 1 and not self.t_min < self.t_max:
            raise ValueError("t_min must lie below t_max for a grid of more than one decay time")
        if not (isinstance(self.refine_levels, int) and 0 <= self.refine_levels <= 8):
            raise ValueError("refine_levels must be 0 .. 8")
        if not (math.isfinite(self.min_ratio) and self.min_ratio > 1.0):
            raise ValueError("min_ratio must be finite and exceed 1")
        if not 0.0 < self.fit_fraction <= 1.0:
            raise ValueError("fit_fraction must satisfy 0 < fit_fraction <= 1")
        if not (math.isfinite(self.accept_rms_db) and self.accept_rms_db >= 0.0):
            raise ValueError("accept_rms_db must be finite and >= 0")
        if self.bands is not None:
            if not isinstance(self.bands, Rt60BandsAnalysisSettings):
                raise ValueError("bands must be an Rt60BandsAnalysisSettings or None")
            if str(self.bands.band_mode).lower() not in BAND_MODES:
                raise ValueError(f"Unknown band_mode: {self.bands.band_mode} (expected one of {', '.join(BAND_MODES)})")


@dataclass(frozen=True)
class MultiSlopeFit:
    """One order's values (step 6).  The tuples have one entry per slope, ascending in T; the turning points one per
    neighbouring pair of slopes."""
    order: int
    decay_times_seconds: Tuple[float, ...]
    coefficients: Tuple[float, ...]
    noise_coefficient: float
    cost: float
    rms_db: float
    start_levels_db: Tuple[float, ...]
    noise_share_db: float
    turning_points_seconds: Tuple[float, ...]
    turning_levels_db: Tuple[float, ...]


@dataclass(frozen=True)
class MultiSlopeValues:
    status: int
    fits_by_order: Dict[int, MultiSlopeFit]
    preferred_order: int                   # 0 when no order has a fit


@dataclass(frozen=True)
class MultiSlopeChannelResult:
    channel_name: str
    sample_rate_hz: int
    start_samples: int
    broadband: MultiSlopeValues
    band_definitions: List[BandDefinition]
    band_values_by_name: Dict[str, MultiSlopeValues]


@dataclass
class MultiSlopeDevice:
    """What multislope_device leaves behind.  Row c * (1 + nbands) + b is channel c's broadband signal (b = 0) or band b - 1."""
    bands: List[BandDefinition]
    start: np.ndarray                      # int64 (nch,) start indices
    row_len: np.ndarray                    # int64 (nrows,) L
    block_size: np.ndarray                 # int32 (nrows,)
    nblk: np.ndarray                       # int32 (nrows,)
    records: object                        # float64 device (nrows, MS_MAX_ORDER, MS_DOUBLES): the last level's
    level_records: list                    # the same after every level (device), level 0 first
    points: object                         # float64 device: d, row j at rows["blk_off"][j]
    info: object                           # int32 device (nrows, 2): status, J
    rows: dict


# ---------------------------------------------------------------------------------------------------
# host helpers
# ---------------------------------------------------------------------------------------------------


def level0_grid(settings: MultiSlopeSettings) -> Tuple[np.ndarray, float]:
    """(T_k = t_min (t_max / t_min)^(k / (G - 1)), k < G, float64; h_0 = ln(t_max / t_min) / (G - 1)).  G = 1: (t_min, 0)."""
    g = settings.grid
    if g == 1:
        return np.array([settings.t_min], dtype=np.float64), 0.0
    k = np.arange(g, dtype=np.float64)
    return settings.t_min * (settings.t_max / settings.t_min) ** (k / (g - 1)), math.log(settings.t_max / settings.t_min) / (g - 1)


def refined_grid(decay_times: Sequence[float], step: float) -> np.ndarray:
    """The ascending union (equal values once) of T exp(k step), k = -R .. R, over decay_times: what ira_multislope_search
    writes for the next level."""
    k = np.arange(-MS_REFINE_R, MS_REFINE_R + 1, dtype=np.float64)
    return np.unique(np.concatenate([float(t) * np.exp(k * float(step)) for t in decay_times]))


def refine_steps(settings: MultiSlopeSettings) -> List[float]:
    """h_1 .. h_refine_levels: h_l = h_{l-1} / (R + 1)."""
    h = level0_grid(settings)[1]
    out = []
    for _ in range(settings.refine_levels):
        h = h / (MS_REFINE_R + 1)
        out.append(h)
    return out


def status_text(status: int) -> str:
    return M.status_text(status, _STATUS_WORDS)


def _db(v: float) -> float:
    if math.isnan(v) or v < 0.0:
        return float("nan")
    return -math.inf if v == 0.0 else 10.0 * math.log10(v)


def fit_from_record(rec: np.ndarray, order: int, sample_rate_hz: float, length: int) -> Optional[MultiSlopeFit]:
    """Step 6 for one order's record (MS_DOUBLES doubles) of a row of `length` samples; None if the record has no winner."""
    ts = [float(rec[REC_T + s]) for s in range(order)]
    if int(rec[REC_STATUS]) != 0 or math.isnan(float(rec[REC_COST])) or not all(t > 0.0 for t in ts):
        return None
    fs, big_l = float(sample_rate_hz), float(length)
    a = [float(rec[REC_A + s]) for s in range(order)]
    a_nu, c, j, d0 = float(rec[REC_A_NOISE]), float(rec[REC_COST]), float(rec[REC_J]), float(rec[REC_D0])
    lam = [LN_1E6 / (t * fs) for t in ts]
    start = tuple(_db(a[s] * (1.0 - math.exp(-lam[s] * big_l)) / d0) for s in range(order))
    turn_t, turn_l = [], []
    for s in range(order - 1):
        tx = math.log(a[s] / a[s + 1]) / (lam[s] - lam[s + 1])
        if tx > 0.0:
            turn_t.append(tx / fs)
            turn_l.append(_db(a[s] * math.exp(-lam[s] * tx) / d0))
        else:
            turn_t.append(float("nan"))
            turn_l.append(float("nan"))
    return MultiSlopeFit(order=order, decay_times_seconds=tuple(ts), coefficients=tuple(a), noise_coefficient=a_nu, cost=c,
                         rms_db=(10.0 / math.log(10.0)) * math.sqrt(c / j), start_levels_db=start, noise_share_db=_db(a_nu / d0),
                         turning_points_seconds=tuple(turn_t), turning_levels_db=tuple(turn_l))


def preferred_order(fits_by_order: Dict[int, MultiSlopeFit], accept_rms_db: float) -> int:
    """Step 7; 0 when there is no fit at all."""
    for s in sorted(fits_by_order):
        if fits_by_order[s].rms_db <= accept_rms_db:
            return s
    return max(fits_by_order) if fits_by_order else 0


def values_from_records(rec: np.ndarray, sample_rate_hz: float, length: int, settings: MultiSlopeSettings) -> MultiSlopeValues:
    """One row: its (MS_MAX_ORDER, MS_DOUBLES) records."""
    status = int(rec[0, REC_STATUS]) & STATUS_ERROR_MASK
    if status:
        return MultiSlopeValues(status, {}, 0)
    fits: Dict[int, MultiSlopeFit] = {}
    for s in range(1, settings.max_order + 1):
        f = fit_from_record(rec[s - 1], s, sample_rate_hz, length)
        if f is None:
            status |= STATUS_NO_CANDIDATE << (s - 1)
        else:
            fits[s] = f
    return MultiSlopeValues(status, fits, preferred_order(fits, settings.accept_rms_db))


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def multislope_device(eng, batch, sample_rate_hz: int, settings: Optional[MultiSlopeSettings] = None,
                      band_signals=None) -> MultiSlopeDevice:
    """
    Every channel of a device batch, broadband and per band: ira_peak_index, ira_block_energy and ira_multislope_points
    once over all rows, then ira_multislope_gram and ira_multislope_search once per level (level 0: one Gram job per row on
    the shared grid and one search job per row and order; later levels: one of each per row and order on the grid the
    search before wrote).  band_signals = (bands, y device, y_off (nch, nbands)) as band_signals_device returns them skips
    the filter bank; otherwise settings.bands decides which are built (None: broadband only).
    """
    settings = settings or MultiSlopeSettings()
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
    base, seg_off = band_row_offsets(batch, band_signals)
    rep = 1 + nbands
    nrows = nch * rep
    rows = eng.lundeby_rows(seg_off, np.repeat(lens64, rep), np.repeat(np.arange(nch, dtype=np.int32), rep), b, nb, m0)
    blk = eng.block_energy(base, rows, start_dev)
    d, info, rec = eng.multislope_points(rows, start_dev, blk, settings.fit_fraction)
    orders = np.arange(1, settings.max_order + 1, dtype=np.int32)
    steps = refine_steps(settings)
    grid0, _ = level0_grid(settings)
    g0 = int(grid0.size)
    grid_dev, grid_n_dev = eng.job_tables(grid0, np.array([g0], dtype=np.int32))
    r = np.arange(nrows, dtype=np.int32)
    zero = np.zeros(nrows, dtype=np.int32)
    gram = eng.multislope_gram(rows, start_dev, d, info, np.stack([r, zero, r], axis=1), grid_dev, grid_n_dev, g0, 1, g0,
                               sample_rate_hz, max(nrows, 1))
    rr, oo = np.repeat(r, orders.size), np.tile(orders, nrows)
    nxt = eng.multislope_search(nrows, info, np.stack([rr, oo, rr, np.zeros_like(rr)], axis=1), grid_dev, grid_n_dev, g0, 1, g0,
                                gram, max(nrows, 1), settings.min_ratio, rec, steps[0] if steps else 0.0)
    level_records = [rec.clone()] if steps else [rec]
    slot = rr * MS_MAX_ORDER + (oo - 1)
    nslots = max(nrows * MS_MAX_ORDER, 1)
    gram = None
    for lvl in range(len(steps)):
        grid_dev, grid_n_dev = nxt
        gram = eng.multislope_gram(rows, start_dev, d, info, np.stack([rr, slot, slot], axis=1), grid_dev, grid_n_dev,
                                   MS_REFINED, nslots, MS_REFINED, sample_rate_hz, nslots, gram_dev=gram)
        nxt = eng.multislope_search(nrows, info, np.stack([rr, oo, slot, slot], axis=1), grid_dev, grid_n_dev, MS_REFINED, nslots,
                                    MS_REFINED, gram, nslots, settings.min_ratio, rec,
                                    steps[lvl + 1] if lvl + 1 < len(steps) else 0.0)
        level_records.append(rec.clone() if lvl + 1 < len(steps) else rec)
    return MultiSlopeDevice(bands=list(bands), start=start, row_len=np.repeat(row_len, rep), block_size=b, nblk=nb, records=rec,
                            level_records=level_records, points=d, info=info, rows=rows)


def multislope_results(dev: MultiSlopeDevice, sample_rate_hz: int, channel_names: Sequence[str],
                       settings: MultiSlopeSettings) -> List[MultiSlopeChannelResult]:
    nch, rep = len(channel_names), 1 + len(dev.bands)
    shape = (nch, rep, MS_MAX_ORDER, MS_DOUBLES)
    rec = dev.records.cpu().numpy().reshape(shape) if nch else np.zeros(shape)
    out = []
    for ch, name in enumerate(channel_names):
        vals = [values_from_records(rec[ch, r], sample_rate_hz, int(dev.row_len[ch * rep + r]), settings) for r in range(rep)]
        out.append(MultiSlopeChannelResult(
            channel_name=str(name), sample_rate_hz=int(sample_rate_hz), start_samples=int(dev.start[ch]), broadband=vals[0],
            band_definitions=list(dev.bands), band_values_by_name={b.name: vals[1 + i] for i, b in enumerate(dev.bands)}))
    return out


# ---------------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------------


def _results_of_batch(eng, batch, sample_rate_hz, names, settings) -> List[MultiSlopeChannelResult]:
    return multislope_results(multislope_device(eng, batch, sample_rate_hz, settings), sample_rate_hz, names, settings)


def analyse_multislope_batch(channels: Sequence[np.ndarray], sample_rate_hz: int, channel_names: Sequence[str],
                             settings: Optional[MultiSlopeSettings] = None) -> List[MultiSlopeChannelResult]:
    """Every channel through the device in batches of at most MAX_BATCH_CHANNELS channels."""
    return M.analyse_channel_batches(channels, sample_rate_hz, channel_names, settings or MultiSlopeSettings(), _results_of_batch)


def analyse_multislope_from_wav_file(input_wav_file_path: str | Path, settings: Optional[MultiSlopeSettings] = None,
                                     expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ
                                     ) -> List[MultiSlopeChannelResult]:
    """One WAV file (mono or stereo, rate checked against expected_sample_rate_hz); channels named "mono", "left", "right"."""
    return M.analyse_wav_file_channels(input_wav_file_path, settings or MultiSlopeSettings(), expected_sample_rate_hz,
                                       analyse_multislope_batch)


def analyse_multislope_files(paths: Sequence[str | Path], settings: Optional[MultiSlopeSettings] = None,
                             expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> List[MultiSlopeChannelResult]:
    """Every channel of every file, MAX_BATCH_CHANNELS channels per device batch; channels named "<file name>:<channel>"."""
    return M.analyse_file_channels(paths, settings or MultiSlopeSettings(), expected_sample_rate_hz, analyse_multislope_batch)


def analyse_multislope_bundle(bundle_root: str | Path, settings: Optional[MultiSlopeSettings] = None,
                              expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> List[MultiSlopeChannelResult]:
    """The taps a bundle's meta.json lists (taps/<name>.wav), a group at a time; channels named "<tap>:<channel>"."""
    return M.analyse_bundle_channels(bundle_root, settings or MultiSlopeSettings(), expected_sample_rate_hz, _results_of_batch)


# ---------------------------------------------------------------------------------------------------
# text, Markdown, JSON
# ---------------------------------------------------------------------------------------------------

_COLUMNS = ("Order", "Pref", "RMS_dB", "T_s", "Start_dB", "Noise_dB", "Turn_ms", "Turn_dB", "Status")


def _join(values: Sequence[float], digits: int, scale: float = 1.0) -> str:
    return "/".join(M.fmt(scale * v, digits) for v in values) if values else "-"


def _fit_cells(f: MultiSlopeFit, preferred: bool, status: int) -> List[str]:
    return [str(f.order), "*" if preferred else "-", M.fmt(f.rms_db, 3), _join(f.decay_times_seconds, 3),
            _join(f.start_levels_db, 2), M.fmt(f.noise_share_db, 2), _join(f.turning_points_seconds, 1, 1000.0),
            _join(f.turning_levels_db, 2), status_text(status)]


def _rows(r: MultiSlopeChannelResult) -> List[List[str]]:
    out = []
    for name, v in M.band_rows(r, r.band_values_by_name):
        if not v.fits_by_order:
            out.append([name, "NA", "-", "NA", "NA", "NA", "NA", "NA", "NA", status_text(v.status)])
        for s in sorted(v.fits_by_order):
            out.append([name] + _fit_cells(v.fits_by_order[s], s == v.preferred_order, v.status))
    return out


def summarise_multislope_text(channel_results: List[MultiSlopeChannelResult]) -> str:
    """
    Fixed text format, one block per channel followed by an empty line:
        [<channel name>]
        Start: <s> samples (<s / fs in ms, 3 decimals> ms)
        Band  Order  Pref  RMS_dB  T_s  Start_dB  Noise_dB  Turn_ms  Turn_dB  Status
        Broadband  <S>  * | -  <rms_db, 3 decimals>  <T_1/../T_S in s, 3>  <start levels in dB, 2>  <noise share in dB, 2>
                   <turning points in ms, 1 | -> <their levels in dB, 2 | ->  ok | <flags> (<words>)
        ...                          (one row per fitted order, "*" marks the preferred one; then the bands, ascending)
    A row without any fit is one line "<band>  NA  -  NA  NA  NA  NA  NA  NA  <status>".  Cells are separated by two spaces,
    the values of a cell by "/"; NaN is "NA", a noise share without a noise term "-inf".
    """
    return M.join_blocks(M.text_block(
        r.channel_name, f"Start: {r.start_samples} samples ({1000.0 * r.start_samples / r.sample_rate_hz:.3f} ms)",
        _COLUMNS, _rows(r)) for r in channel_results)


def summarise_multislope_markdown(channel_results: List[MultiSlopeChannelResult]) -> str:
    """The same values as a Markdown section per channel: a '### <channel name>' heading, a start line and a table with the
    columns of the text format."""
    cols = ("Order", "Preferred", "RMS (dB)", "T (s)", "Start (dB)", "Noise (dB)", "Turning point (ms)", "Level there (dB)",
            "Status")
    return M.join_blocks(M.markdown_block(
        r.channel_name, f"Start: {r.start_samples} samples ({1000.0 * r.start_samples / r.sample_rate_hz:.3f} ms).",
        cols, _rows(r)) for r in channel_results)


_TUPLE_FIELDS = ("decay_times_seconds", "coefficients", "start_levels_db", "turning_points_seconds", "turning_levels_db")
_SCALAR_FIELDS = ("noise_coefficient", "cost", "rms_db", "noise_share_db")


def _values_json(v: MultiSlopeValues) -> Dict:
    fits = []
    for s in sorted(v.fits_by_order):
        f = v.fits_by_order[s]
        d: Dict = {"order": f.order}
        for k in _TUPLE_FIELDS:
            d[k] = [M.json_num(x) for x in getattr(f, k)]
        for k in _SCALAR_FIELDS:
            d[k] = M.json_num(getattr(f, k))
        fits.append(d)
    return {"status": v.status, "preferred_order": v.preferred_order, "fits": fits}


def _values_from_json(d: Dict) -> MultiSlopeValues:
    fits = {}
    for f in d["fits"]:
        fits[int(f["order"])] = MultiSlopeFit(order=int(f["order"]),
                                              **{k: tuple(M.num_json(x) for x in f[k]) for k in _TUPLE_FIELDS},
                                              **{k: M.num_json(f[k]) for k in _SCALAR_FIELDS})
    return MultiSlopeValues(status=int(d["status"]), fits_by_order=fits, preferred_order=int(d["preferred_order"]))


def multislope_results_to_json(channel_results: List[MultiSlopeChannelResult]) -> Dict:
    """Plain JSON: NaN is null, -inf the string "-inf"."""
    rows = []
    for r in channel_results:
        rows.append({
            "channel_name": r.channel_name, "sample_rate_hz": r.sample_rate_hz, "start_samples": r.start_samples,
            "broadband": _values_json(r.broadband),
            "bands": [M.band_to_json(b, _values_json(r.band_values_by_name[b.name])) for b in r.band_definitions],
        })
    return {"multislope": rows}


def multislope_results_from_json(doc: Dict) -> List[MultiSlopeChannelResult]:
    out = []
    for d in doc["multislope"]:
        out.append(MultiSlopeChannelResult(
            channel_name=d["channel_name"], sample_rate_hz=int(d["sample_rate_hz"]), start_samples=int(d["start_samples"]),
            broadband=_values_from_json(d["broadband"]), band_definitions=M.bands_from_json(d["bands"]),
            band_values_by_name={b["name"]: _values_from_json(b) for b in d["bands"]}))
    return out


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.multislope",
        description="Multi-slope decay fits (coupled rooms): one to three exponentials plus a noise term fitted to the "
                    "Schroeder curve per channel and band.  A channel holds at most "
                    f"{MAX_CHANNEL_SAMPLES} samples (174.7 s at 48 kHz); a longer file is refused.")
    M.add_source_arguments(p)
    M.add_bands_argument(p)
    p.add_argument("--max-order", type=int, default=3, help="fit orders 1 .. this (default: 3)")
    p.add_argument("--t-min", type=float, default=0.05, help="shortest decay time of the grid in seconds (default: 0.05)")
    p.add_argument("--t-max", type=float, default=20.0, help="longest decay time of the grid in seconds (default: 20)")
    p.add_argument("--grid", type=int, default=64, help=f"decay times of the first grid, at most {MS_MAX_GRID} (default: 64)")
    p.add_argument("--refine-levels", type=int, default=3, help="refinements around the winner (default: 3)")
    p.add_argument("--min-ratio", type=float, default=1.5, help="smallest ratio of neighbouring decay times (default: 1.5)")
    p.add_argument("--fit-fraction", type=float, default=0.9, help="leading share of the curve that is fitted (default: 0.9)")
    p.add_argument("--accept-rms-db", type=float, default=0.15,
                   help="the preferred order is the smallest whose rms error is at most this (default: 0.15)")
    M.add_output_arguments(p)
    return p


def settings_from_args(args) -> MultiSlopeSettings:
    bands = None if args.bands == "none" else Rt60BandsAnalysisSettings(band_mode=args.bands)
    return MultiSlopeSettings(max_order=args.max_order, t_min=args.t_min, t_max=args.t_max, grid=args.grid,
                              refine_levels=args.refine_levels, min_ratio=args.min_ratio, fit_fraction=args.fit_fraction,
                              accept_rms_db=args.accept_rms_db, bands=bands, use_mono_downmix_for_stereo=bool(args.mono))


def main(argv: Optional[Sequence[str]] = None) -> None:
    M.run_cli(build_parser(), argv, settings_from_args, analyse_multislope_files, analyse_multislope_bundle,
              summarise_multislope_text, multislope_results_to_json)


if __name__ == "__main__":
    main()
