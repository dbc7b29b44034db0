"""
Energy decay relief (EDR): decay time and initial level per frequency.

Jot's energy decay relief is the Schroeder backward integration done separately at every frequency of a
short-time transform.  Two curves are read from it, the decay time against frequency and the initial energy against
frequency: what a feedback-delay-network design is matched to.  decay.py and rt60bands.py integrate backwards too, but in
one band or a few filter-bank bands; modalcloud.py fits lines to the raw STFT magnitude of each log bin, without the
integration, so its points scatter with every beat between neighbouring modes.  This is the smooth, fittable counterpart.

Definitions (include/ira_edr.h pins the device side):

  segment   of a channel: as spectrogram.select_stft_segments chooses it (trim_to_peak, ignore_leading_seconds,
            analysis_duration_seconds); `len` samples
  frames    n_fft a power of two 256 .. 8192, 1 <= hop <= n_fft, T = 1 + (len - n_fft) // hop frames, frame m starts at
            m * hop, no padding; window Engine.window(n_fft, use_hann, 64), twiddles Engine.twiddle(n_fft, 64)
  rows      contiguous runs of rFFT bins [first_j, first_j + count_j) within 0 .. n_fft / 2: the log bins of
            modalcloud.log_bin_rows over the edges lo * 2^linspace(0, span, count + 1), count = ceil(span *
            points_per_octave), between f_min_hz and f_max_hz (clipped to 1 Hz .. Nyquist): modalcloud._build_log_bins
            without its floor of four bins an octave (the same edges bit for bit from four an octave on).  A row may have
            count_j == 0: an empty row, reported as empty and never refused.  At most 256 rows.
  power     P(m, j) = sum over k in row j of |X_m[k]|^2, float64, X_m the transform of the windowed frame
  noise     (Chu's subtraction, off by default) q = floor(noise_tail_fraction * T) frames; q >= 1: N_j = S_raw(T - q, j) / q,
            S_raw the backward sum of P, and P'(m, j) = P(m, j) - N_j; q = 0: N_j = 0, P' = P, nothing is subtracted
  backward sum  S(m, j) = sum over m' >= m of P'(m', j), in this order and no other: the T values of a row are cut into
            blocks of 64 frames counted from the END, block b = [max(T - 64 (b + 1), 0), T - 64 b); lane l of a block holds
            frame T - 64 (b + 1) + l, or 0.0 where that index is negative; six simultaneous steps d = 1, 2, 4, 8, 16, 32:
            v[l] = v[l] + v[l + d] for l + d < 64; out[l] = v[l] + carry, carry = 0.0 for block 0 and out[0] of the block
            before otherwise
  curve     L(m, j) = float32(max(10 log10(max(S(m, j), eps) / S(0, j)), floor_db)); S(0, j) finite and <= eps: the whole
            row is floor_db; S(0, j) NaN: the row is NaN
  record    per segment and row four doubles: S(0, j), N_j, max over m of P(m, j), the first frame of that maximum
            (numpy.max / numpy.argmax: a NaN wins)
  fits      Engine.curve_fits on the curves with t_mul = hop, t_div = sample rate, rel_to_peak = False, min_points =
            min_fit_points, ranges EDT (0, -10), T20 (-5, -25), T30 (-5, -35): the crossing-and-line-fit kernel of the decay
            modules, no new fitting code

Device work: ira_edr_power (frames -> band powers, two frames per float64 transform), ira_edr_integrate (the backward sums,
records and curves, one wavefront per channel and row), ira_curve_fits.

Per row the result holds the centre and edge frequencies, the bin count, initial_level_db = 10 log10 S(0, j) minus the
channel's largest, total_energy = S(0, j), the noise power N_j, the time of the loudest frame, EDT / T20 / T30 with r^2 and a
valid flag each, and a status word: 1 empty (count_j == 0), 2 silent (S(0, j) finite and <= eps), 4 non-finite (S(0, j) is
not finite).  A row with a status has NaN times and level.  Per channel: the median T30 over the valid rows, the centre
frequency of the longest valid T30 and, unless with_relief is off, the relief L itself.

Command line (no plots): python -m analyse.edr --input A.wav [B.wav ...] | --bundle DIR [--mono] [--n-fft 2048] [--hop 256]
  [--window hann|rect] [--points-per-octave 3] [--f-min 20] [--f-max 20000] [--noise-tail-fraction 0] [--duration S]
  [--ignore-leading S] [--no-trim] [--floor-db -120] [--min-fit-points 5] [--no-relief] [--expected-sample-rate 48000]
  [--json OUT.json]
"""
from __future__ import annotations

import argparse
import math
from dataclasses import dataclass
from math import ceil, log2
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _measure as M
from ..engine import EDR_DOUBLES, EDR_MAX_FFT, EDR_MAX_ROWS, EDR_MIN_FFT
from ._measure import MAX_BATCH_CHANNELS  # noqa: F401  (part of this module's surface)
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ
from .modalcloud import log_bin_rows
from .spectrogram import select_stft_segments

STATUS_EMPTY = 1
STATUS_SILENT = 2
STATUS_NON_FINITE = 4
_STATUS_WORDS = ((STATUS_EMPTY, "empty"), (STATUS_SILENT, "silent"), (STATUS_NON_FINITE, "non-finite"))

WINDOWS = ("hann", "rect")
FIT_RANGES = ((0.0, -10.0), (-5.0, -25.0), (-5.0, -35.0))         # EDT, T20, T30
FIT_NAMES = ("edt", "t20", "t30")
MAX_ROWS = EDR_MAX_ROWS


@dataclass(frozen=True)
class EdrSettings:
    use_mono_downmix_for_stereo: bool = False
    trim_to_peak: bool = True
    ignore_leading_seconds: float = 0.0
    analysis_duration_seconds: Optional[float] = None
    n_fft: int = 2048
    hop_length: int = 256
    use_hann_window: bool = True
    f_min_hz: float = 20.0
    f_max_hz: float = 20000.0
    points_per_octave: int = 3
    noise_tail_fraction: float = 0.0
    eps: float = 1e-30
    floor_db: float = -120.0
    min_fit_points: int = 5
    with_relief: bool = True

    def __post_init__(self):
        n_fft, hop = self.n_fft, self.hop_length
        if not (isinstance(n_fft, (int, np.integer)) and EDR_MIN_FFT <= n_fft <= EDR_MAX_FFT and n_fft & (n_fft - 1) == 0):
            raise ValueError(f"n_fft must be a power of two from {EDR_MIN_FFT} to {EDR_MAX_FFT}, got {n_fft}")
        if not (isinstance(hop, (int, np.integer)) and 1 <= hop <= n_fft):
            raise ValueError(f"hop_length must be 1 .. n_fft, got {hop}")
        lead, dur = float(self.ignore_leading_seconds), self.analysis_duration_seconds
        if not (math.isfinite(lead) and lead >= 0.0):
            raise ValueError(f"ignore_leading_seconds must be finite and >= 0, got {self.ignore_leading_seconds}")
        if dur is not None:
            dur = float(dur)
            if not (math.isfinite(dur) and dur > 0.0):
                raise ValueError(f"analysis_duration_seconds must be positive and finite, or None, got {dur}")
        f_lo, f_hi = float(self.f_min_hz), float(self.f_max_hz)
        if not (math.isfinite(f_lo) and math.isfinite(f_hi) and 0.0 < f_lo < f_hi):
            raise ValueError(f"0 < f_min_hz < f_max_hz, both finite, got {self.f_min_hz} and {self.f_max_hz}")
        ppo = self.points_per_octave
        if not (isinstance(ppo, (int, np.integer)) and 1 <= ppo <= 48):
            raise ValueError(f"points_per_octave must be a whole number 1 .. 48, got {ppo}")
        frac = float(self.noise_tail_fraction)
        if not (math.isfinite(frac) and 0.0 <= frac <= 1.0):
            raise ValueError(f"noise_tail_fraction must be in 0 .. 1, got {self.noise_tail_fraction}")
        eps, floor_db = float(self.eps), float(self.floor_db)
        if not (math.isfinite(eps) and eps >= 0.0):
            raise ValueError(f"eps must be finite and >= 0, got {self.eps}")
        if not (math.isfinite(floor_db) and floor_db < -35.0):
            raise ValueError(f"floor_db must be finite and below the -35 dB end of the T30 range, got {self.floor_db}")
        if not (isinstance(self.min_fit_points, (int, np.integer)) and self.min_fit_points >= 2):
            raise ValueError(f"min_fit_points must be a whole number >= 2, got {self.min_fit_points}")
        for k, v in (("n_fft", int(n_fft)), ("hop_length", int(hop)), ("ignore_leading_seconds", lead),
                     ("analysis_duration_seconds", dur), ("f_min_hz", f_lo), ("f_max_hz", f_hi), ("points_per_octave", int(ppo)),
                     ("noise_tail_fraction", frac), ("eps", eps), ("floor_db", floor_db),
                     ("min_fit_points", int(self.min_fit_points)), ("use_mono_downmix_for_stereo", bool(self.use_mono_downmix_for_stereo)),
                     ("trim_to_peak", bool(self.trim_to_peak)), ("use_hann_window", bool(self.use_hann_window)),
                     ("with_relief", bool(self.with_relief))):
            object.__setattr__(self, k, v)


@dataclass(frozen=True)
class EdrRows:
    """The rows of one (n_fft, sample rate, f_min, f_max, points per octave): float32 centres and edges as log_bin_rows
    forms them, first rFFT bin and bin count per row."""
    centre_hz: np.ndarray         # float32 (J,)
    low_edge_hz: np.ndarray       # float32 (J,)
    high_edge_hz: np.ndarray      # float32 (J,)
    first: np.ndarray             # int32 (J,): rFFT bin
    count: np.ndarray             # int32 (J,)


def log_edges(f_min_hz: float, f_max_hz: float, points_per_octave: int) -> np.ndarray:
    """Log-spaced row edges (float32): modalcloud._build_log_bins without its floor of four bins an octave (and with no
    least count); from four an octave on the two give the same bits."""
    lo = float(max(1.0, f_min_hz))
    hi = float(max(lo * 1.001, f_max_hz))
    span = float(log2(hi / lo))
    count = int(max(1, ceil(span * float(points_per_octave))))
    return (lo * (2.0 ** np.linspace(0.0, span, count + 1, dtype=np.float64))).astype(np.float32)


def edr_rows(n_fft: int, sample_rate_hz: float, f_min_hz: float, f_max_hz: float, points_per_octave: int) -> EdrRows:
    """The row tables: the rFFT bins with f_lo <= f <= f_hi (float32 frequencies, the limits clipped to 1 Hz .. Nyquist) are
    dealt to the log bins by modalcloud.log_bin_rows (lo <= f < hi in float32)."""
    freq = np.fft.rfftfreq(int(n_fft), d=1.0 / float(sample_rate_hz)).astype(np.float32)
    nyq = 0.5 * float(sample_rate_hz)
    f_lo = float(np.clip(f_min_hz, 1.0, nyq))
    f_hi = float(np.clip(f_max_hz, f_lo, nyq))
    sel = np.nonzero((freq >= f_lo) & (freq <= f_hi))[0]
    edges = log_edges(f_lo, f_hi, int(points_per_octave))
    k_base = int(sel[0]) if sel.size else 0
    centres, first, count = log_bin_rows(freq[sel], edges)
    return EdrRows(centre_hz=centres, low_edge_hz=edges[:-1].copy(), high_edge_hz=edges[1:].copy(),
                   first=(first + k_base).astype(np.int32), count=count.astype(np.int32))


@dataclass(frozen=True, eq=False)
class EdrChannelResult:
    channel_name: str
    sample_rate_hz: int
    analysis_start_sample_index: int
    analysis_length_samples: int
    n_fft: int
    hop_length: int
    frames: int                               # T
    noise_frames: int                         # q
    frame_seconds: float                      # hop / fs: the time step of the relief
    centre_hz: np.ndarray                     # float64 (J,)
    low_edge_hz: np.ndarray
    high_edge_hz: np.ndarray
    bin_count: np.ndarray                     # int64 (J,)
    status: np.ndarray                        # int64 (J,): STATUS_* bits
    initial_level_db: np.ndarray              # 10 log10 S(0, j) minus the largest of the channel; NaN for a row with a status
    total_energy: np.ndarray                  # S(0, j)
    noise_power: np.ndarray                   # N_j
    peak_time_seconds: np.ndarray             # the first loudest frame of the row, m * hop / fs
    edt_seconds: np.ndarray
    edt_r2: np.ndarray
    edt_valid: np.ndarray                     # bool (J,)
    t20_seconds: np.ndarray
    t20_r2: np.ndarray
    t20_valid: np.ndarray
    t30_seconds: np.ndarray
    t30_r2: np.ndarray
    t30_valid: np.ndarray
    median_t30_seconds: float                 # over the rows with a valid T30; NaN: none
    longest_t30_hz: float                     # the centre of the row with the longest valid T30; NaN: none
    relief_db: Optional[np.ndarray] = None    # float32 (J, T): L(m, j); None: not kept


@dataclass
class EdrRecords:
    """What edr_device leaves behind: the row tables and per-channel segment on the host, the records, fits and curves on
    the device (curves: (J, T_c) float32 of channel c at curve_off[c])."""
    settings: EdrSettings
    rows: EdrRows
    starts: np.ndarray                        # int64 (nch,)
    lens: np.ndarray                          # int64 (nch,)
    frames: np.ndarray                        # int64 (nch,)
    noise_frames: np.ndarray                  # int64 (nch,)
    records: "object"                         # torch.float64 (nch, J, EDR_DOUBLES) on device
    fits: "object"                            # torch.float64 (nch * J, 3, 8) on device
    curves: "object"                          # torch.float32 flat on device
    curve_off: np.ndarray                     # int64 (nch,)


def status_text(status: int) -> str:
    return M.status_text(int(status), _STATUS_WORDS)


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def edr_device(eng, batch, sample_rate_hz: int, settings: Optional[EdrSettings] = None) -> EdrRecords:
    """Band powers, backward sums, curves and fits of every channel of a device batch: ira_edr_power, ira_edr_integrate,
    ira_curve_fits, one call each; records, fits and curves stay on the device."""
    settings = settings or EdrSettings()
    starts, lens, nframes = select_stft_segments(eng, batch, sample_rate_hz, settings, "energy decay relief")
    n_fft, hop = settings.n_fft, settings.hop_length
    rows = edr_rows(n_fft, sample_rate_hz, settings.f_min_hz, settings.f_max_hz, settings.points_per_octave)
    nrows = int(rows.first.size)
    if not 1 <= nrows <= MAX_ROWS:
        raise ValueError(f"{nrows} rows between {settings.f_min_hz:g} and {settings.f_max_hz:g} Hz at "
                         f"{settings.points_per_octave} an octave: at most {MAX_ROWS}")
    p_dev, frames, _ = eng.edr_power(batch.x, batch.off + starts, lens, n_fft, hop, settings.use_hann_window, rows.first,
                                     rows.count)
    q = np.floor(settings.noise_tail_fraction * frames.astype(np.float64)).astype(np.int64)
    curves, c_off, rec, _ = eng.edr_integrate(p_dev, frames, nrows, q, settings.eps, settings.floor_db)
    f_off = (c_off[:, None] + np.arange(nrows, dtype=np.int64)[None, :] * frames[:, None]).reshape(-1)
    fits, _ = eng.curve_fits(curves, f_off, np.repeat(frames, nrows), float(hop), float(sample_rate_hz), FIT_RANGES,
                             settings.min_fit_points)
    return EdrRecords(settings=settings, rows=rows, starts=np.asarray(starts, dtype=np.int64),
                      lens=np.asarray(lens, dtype=np.int64), frames=frames, noise_frames=q, records=rec, fits=fits,
                      curves=curves, curve_off=c_off)


# ---------------------------------------------------------------------------------------------------
# host: records -> results
# ---------------------------------------------------------------------------------------------------


def row_status(count: np.ndarray, s0: np.ndarray, eps: float) -> np.ndarray:
    """The status word per row: empty (no bin), else silent (S(0) finite and <= eps), else non-finite (S(0) not finite)."""
    count, s0 = np.asarray(count), np.asarray(s0, dtype=np.float64)
    fin = np.isfinite(s0)
    st = np.where(fin, np.where(s0 <= eps, STATUS_SILENT, 0), STATUS_NON_FINITE)
    return np.where(count == 0, STATUS_EMPTY, st).astype(np.int64)


def edr_results(res: EdrRecords, sample_rate_hz: int, channel_names: Sequence[str]) -> List[EdrChannelResult]:
    st, rows = res.settings, res.rows
    fs = float(sample_rate_hz)
    nch, nrows = len(channel_names), int(rows.first.size)
    rec = res.records.cpu().numpy().reshape(nch, nrows, EDR_DOUBLES)
    fits = res.fits.cpu().numpy().reshape(nch, nrows, len(FIT_RANGES), 8)
    curves = res.curves.cpu().numpy() if st.with_relief else None
    out = []
    for ch, name in enumerate(channel_names):
        s0 = rec[ch, :, 0]
        status = row_status(rows.count, s0, st.eps)
        ok = status == 0
        with np.errstate(all="ignore"):
            level = np.where(ok, 10.0 * np.log10(np.where(ok, s0, 1.0)), np.nan)
        if ok.any():
            level = level - np.nanmax(level)
        times = {}
        for k, fit in enumerate(FIT_NAMES):
            valid = ok & (fits[ch, :, k, 0] == 1.0)
            times[f"{fit}_seconds"] = np.where(valid, fits[ch, :, k, 6], np.nan)
            times[f"{fit}_r2"] = np.where(valid, fits[ch, :, k, 5], np.nan)
            times[f"{fit}_valid"] = valid
        t30, v30 = times["t30_seconds"], times["t30_valid"]
        T = int(res.frames[ch])
        relief = None
        if curves is not None:
            a = int(res.curve_off[ch])
            relief = curves[a : a + nrows * T].reshape(nrows, T).copy()
        out.append(EdrChannelResult(
            channel_name=str(name), sample_rate_hz=int(sample_rate_hz), analysis_start_sample_index=int(res.starts[ch]),
            analysis_length_samples=int(res.lens[ch]), n_fft=st.n_fft, hop_length=st.hop_length, frames=T,
            noise_frames=int(res.noise_frames[ch]), frame_seconds=st.hop_length / fs,
            centre_hz=rows.centre_hz.astype(np.float64), low_edge_hz=rows.low_edge_hz.astype(np.float64),
            high_edge_hz=rows.high_edge_hz.astype(np.float64), bin_count=rows.count.astype(np.int64), status=status,
            initial_level_db=level, total_energy=s0.copy(), noise_power=rec[ch, :, 1].copy(),
            peak_time_seconds=np.where(rows.count > 0, rec[ch, :, 3] * st.hop_length / fs, np.nan),
            median_t30_seconds=float(np.median(t30[v30])) if v30.any() else float("nan"),
            longest_t30_hz=float(rows.centre_hz[int(np.argmax(np.where(v30, t30, -np.inf)))]) if v30.any() else float("nan"),
            relief_db=relief, **times))
    return out


# ---------------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------------


def _results_of_batch(eng, batch, sample_rate_hz, names, settings) -> List[EdrChannelResult]:
    return edr_results(edr_device(eng, batch, sample_rate_hz, settings), sample_rate_hz, names)


def analyse_edr_batch(channels: Sequence[np.ndarray], sample_rate_hz: int, channel_names: Sequence[str],
                      settings: Optional[EdrSettings] = None) -> List[EdrChannelResult]:
    """Every channel through the device in batches of at most MAX_BATCH_CHANNELS channels."""
    return M.analyse_channel_batches(channels, sample_rate_hz, channel_names, settings or EdrSettings(), _results_of_batch)


def analyse_edr_for_channel(samples: np.ndarray, sample_rate_hz: int, channel_name: str,
                            settings: Optional[EdrSettings] = None) -> EdrChannelResult:
    return analyse_edr_batch([samples], sample_rate_hz, [channel_name], settings)[0]


def analyse_edr_from_wav_file(input_wav_file_path: str | Path, settings: Optional[EdrSettings] = None,
                              expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> List[EdrChannelResult]:
    """One WAV file (mono or stereo, rate checked against expected_sample_rate_hz); channels named as by
    get_analysis_channels ("mono", "left", "right")."""
    return M.analyse_wav_file_channels(input_wav_file_path, settings or EdrSettings(), expected_sample_rate_hz,
                                       analyse_edr_batch)


def analyse_edr_files(paths: Sequence[str | Path], settings: Optional[EdrSettings] = None,
                      expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> List[EdrChannelResult]:
    """Every channel of every file in one device batch per MAX_BATCH_CHANNELS channels; channels named
    "<file name>:<channel>"."""
    return M.analyse_file_channels(paths, settings or EdrSettings(), expected_sample_rate_hz, analyse_edr_batch)


def analyse_edr_bundle(bundle_root: str | Path, settings: Optional[EdrSettings] = None,
                       expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> List[EdrChannelResult]:
    """The taps a bundle's meta.json lists (taps/<name>.wav), read by the native ingest a group at a time; channels named
    "<tap>:<channel>"."""
    return M.analyse_bundle_channels(bundle_root, settings or EdrSettings(), expected_sample_rate_hz, _results_of_batch)


# ---------------------------------------------------------------------------------------------------
# text, JSON
# ---------------------------------------------------------------------------------------------------

_COLUMNS = ["bins", "level_dB", "EDT_s", "T20_s", "T30_s", "r2_T30", "status"]


def _rows_text(r: EdrChannelResult) -> List[List[str]]:
    return [[f"{r.centre_hz[j]:.1f}", str(int(r.bin_count[j])), M.fmt(float(r.initial_level_db[j]), 2),
             M.fmt(float(r.edt_seconds[j]), 3), M.fmt(float(r.t20_seconds[j]), 3), M.fmt(float(r.t30_seconds[j]), 3),
             M.fmt(float(r.t30_r2[j]), 4), status_text(int(r.status[j]))] for j in range(r.centre_hz.size)]


def summarise_edr_text(channel_results: List[EdrChannelResult]) -> str:
    """
    Fixed text format, one block per channel followed by an empty line:
        [<channel name>]
        Frames: <T> of <n_fft> every <hop> samples (<hop / fs in ms, 3 decimals> ms)  Noise frames: <q>  Rows: <J>
        freq_Hz  bins  level_dB  EDT_s  T20_s  T30_s  r2_T30  status
        <centre, 1 decimal>  <bin count>  <2 decimals>  <3 decimals> x 3  <4 decimals>  ok | <flags> (<words>)
        median T30: <3 decimals> s over <valid rows> rows, longest at <1 decimal> Hz
    Cells are separated by two spaces; NaN (no fit, or a row with a status) is "NA".
    """
    return M.join_blocks(M.text_block(
        r.channel_name,
        f"Frames: {r.frames} of {r.n_fft} every {r.hop_length} samples ({1000.0 * r.frame_seconds:.3f} ms)  "
        f"Noise frames: {r.noise_frames}  Rows: {r.centre_hz.size}",
        _COLUMNS, _rows_text(r),
        tail=[f"median T30: {M.fmt(r.median_t30_seconds, 3)} s over {int(np.sum(r.t30_valid))} rows, longest at "
              f"{M.fmt(r.longest_t30_hz, 1)} Hz"], first="freq_Hz") for r in channel_results)


_SCALARS = (("channel_name", str), ("sample_rate_hz", int), ("analysis_start_sample_index", int),
            ("analysis_length_samples", int), ("n_fft", int), ("hop_length", int), ("frames", int), ("noise_frames", int),
            ("frame_seconds", float))
_FLOAT_ROWS = ("centre_hz", "low_edge_hz", "high_edge_hz", "initial_level_db", "total_energy", "noise_power",
               "peak_time_seconds", "edt_seconds", "edt_r2", "t20_seconds", "t20_r2", "t30_seconds", "t30_r2")
_INT_ROWS = ("bin_count", "status")
_BOOL_ROWS = ("edt_valid", "t20_valid", "t30_valid")


def edr_results_to_json(channel_results: List[EdrChannelResult], with_relief: bool = True) -> Dict:
    """Plain JSON: NaN is null, an infinity "+inf" / "-inf".  The relief is written for the channels that kept one unless
    with_relief is False."""
    docs = []
    for r in channel_results:
        d = {k: kind(getattr(r, k)) for k, kind in _SCALARS}
        for k in _FLOAT_ROWS:
            d[k] = [M.json_num(float(v)) for v in getattr(r, k)]
        for k in _INT_ROWS:
            d[k] = [int(v) for v in getattr(r, k)]
        for k in _BOOL_ROWS:
            d[k] = [bool(v) for v in getattr(r, k)]
        d["median_t30_seconds"] = M.json_num(r.median_t30_seconds)
        d["longest_t30_hz"] = M.json_num(r.longest_t30_hz)
        if with_relief and r.relief_db is not None:
            d["relief_db"] = [[M.json_num(float(v)) for v in row] for row in r.relief_db]
        docs.append(d)
    return {"energy_decay_relief": docs}


def edr_results_from_json(doc: Dict) -> List[EdrChannelResult]:
    out = []
    for d in doc["energy_decay_relief"]:
        kw = {k: kind(d[k]) for k, kind in _SCALARS}
        for k in _FLOAT_ROWS:
            kw[k] = np.asarray([M.num_json(v) for v in d[k]], dtype=np.float64)
        for k in _INT_ROWS:
            kw[k] = np.asarray(d[k], dtype=np.int64)
        for k in _BOOL_ROWS:
            kw[k] = np.asarray(d[k], dtype=bool)
        relief = None
        if "relief_db" in d:
            relief = np.asarray([[M.num_json(v) for v in row] for row in d["relief_db"]],
                                dtype=np.float32).reshape(len(d["centre_hz"]), kw["frames"])
        out.append(EdrChannelResult(median_t30_seconds=M.num_json(d["median_t30_seconds"]),
                                    longest_t30_hz=M.num_json(d["longest_t30_hz"]), relief_db=relief, **kw))
    return out


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.edr",
        description="Energy decay relief (Jot): the Schroeder backward integration per log-frequency row of a short-time "
                    "transform; decay times (EDT, T20, T30) and initial level against frequency.")
    M.add_source_arguments(p)
    p.add_argument("--n-fft", type=int, default=2048, help="frame length, a power of two 256 .. 8192 (default: 2048)")
    p.add_argument("--hop", type=int, default=256, help="frame advance in samples, 1 .. n_fft (default: 256)")
    p.add_argument("--window", choices=WINDOWS, default="hann", help="frame window (default: hann)")
    p.add_argument("--points-per-octave", type=int, default=3, help="rows per octave, 1 .. 48 (default: 3)")
    p.add_argument("--f-min", type=float, default=20.0, help="lower edge of the first row in Hz (default: 20)")
    p.add_argument("--f-max", type=float, default=20000.0, help="upper edge of the last row in Hz (default: 20000)")
    p.add_argument("--noise-tail-fraction", type=float, default=0.0,
                   help="subtract the mean power of this last share of the frames from every frame (Chu; default: 0, off)")
    p.add_argument("--duration", type=float, default=None, help="analyse this many seconds (default: to the end)")
    p.add_argument("--ignore-leading", type=float, default=0.0, help="skip this many seconds at the start (default: 0)")
    p.add_argument("--no-trim", action="store_true", help="start at the first sample, not at the peak")
    p.add_argument("--floor-db", type=float, default=-120.0, help="floor of the relief in dB (default: -120)")
    p.add_argument("--min-fit-points", type=int, default=5, help="frames a line fit needs at least (default: 5)")
    p.add_argument("--no-relief", action="store_true", help="leave the relief itself out of the results and the JSON")
    M.add_output_arguments(p)
    return p


def settings_from_args(args) -> EdrSettings:
    return EdrSettings(use_mono_downmix_for_stereo=bool(args.mono), trim_to_peak=not args.no_trim,
                       ignore_leading_seconds=args.ignore_leading, analysis_duration_seconds=args.duration,
                       n_fft=args.n_fft, hop_length=args.hop, use_hann_window=args.window == "hann", f_min_hz=args.f_min,
                       f_max_hz=args.f_max, points_per_octave=args.points_per_octave,
                       noise_tail_fraction=args.noise_tail_fraction, floor_db=args.floor_db,
                       min_fit_points=args.min_fit_points, with_relief=not args.no_relief)


def main(argv: Optional[Sequence[str]] = None) -> None:
    M.run_cli(build_parser(), argv, settings_from_args, analyse_edr_files, analyse_edr_bundle, summarise_edr_text,
              edr_results_to_json)


if __name__ == "__main__":
    main()
