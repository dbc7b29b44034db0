"""
Early reflections per channel: where are the discrete reflections of an impulse response -- their delays after the direct
sound, levels and polarities -- with the energy-time curve (ETC) they are read from, the initial time delay gap (ITDG) and
the direct-to-reverberant ratio (DRR).

energy.py, lundeby.py, multislope.py and sti.py integrate energy, echo.py judges the audibility of one late echo and
echodensity.py reports when the response stops being discrete; report.py plots an "Early reflections" image.  Nothing
computes what that image shows, and the reference has no such function: this module replaces nothing.

For a channel x (float32) of L samples at rate fs; o its broadband onset as in energy.py and echodensity.py
(eng.onset_index(batch, rel_energy), onset_db = -20 by default).  Every count below is max(1, floor(ms * fs / 1000 + 0.5))
in float64 unless stated:

  d    = max(1, floor(smooth_ms * fs / 2000 + 0.5))   W = 2 d + 1     smooth_ms 1.0       d <= REFL_MAX_HALF 512
  w[k] = 0.5 - 0.5 cos(2 pi (k + 1) / (W + 1)) (hann) | 1 (rect)      float64, built ON THE HOST (echodensity.window_weights)
  D    = direct_search_ms samples (2.5)                               D <= REFL_MAX_DIRECT 1024
  Dw   = direct_window_ms samples (2.5)       half width of the direct window of the DRR
  G    = guard_ms samples (1.0)   S = separation_ms samples (0.5)     G >= S, S <= 1024
  B    = background_ms samples (5.0)                                  S < B <= REFL_MAX_BG 2048
  Tn   = ceil(max_time_ms * fs / 1000) (200 ms; None: unbounded)
  rel  = 10^(min_level_db / 10) (-40)    prom = 10^(prominence_db / 10) (6, >= 0 dB)    keep = max_reflections (16, 1..64)

Envelope (the energy-time curve).  h2[i] = float64(x[i])^2 (exact), 0 outside [0, L);
  e[n] = sum_{k = 0 .. W-1} w[k] * h2[n - d + k],  from 0.0, k ASCENDING, one rounding per multiply and per add.
The device stores the row erow[j] = e[o + j], j < R = min(L - o, Rmax), Rmax = D + Tn + B (L for an unbounded Tn).  The
host sizes the row for onset 0 (min(L, Rmax) doubles): the onset never returns to the host first; entries from R on are
NaN.  With the defaults that is about 10 k doubles per channel, whatever its length.

Direct sound.  n0 = the first index of the maximum of e over [o, min(L, o + D)) (a NaN never wins);  Ed = e[n0].

Candidates.  n in [n0 + G, min(L, n0 + Tn + 1)) for which ALL of these hold, compared in float64:
  1. e[n] >  e[m] for m in [n - S, n)                       (m >= o always: G >= S)
  2. e[n] >= e[m] for m in (n, min(n + S, L - 1)]           (the earlier index wins a tie)
  3. e[n] >= Ed * rel
  4. e[n] * float64(cnt) >= prom * Bsum,  Bsum = the sum of e[m] over [max(n - B, n0 + G), n - S) and then (n + S,
     min(n + B, L - 1)], added SEQUENTIALLY with m ascending from 0.0, cnt = its number of terms; cnt == 0 or Bsum == 0
     passes (the prominence is +inf).  The direct sound is kept out of the background on purpose: with it inside, a -6 dB
     reflection 3 ms behind the direct sound is missed.
Two candidates lie more than S samples apart, so a range of N samples holds at most ceil(N / (S + 1)): this sizes the
candidate scratch on the host (engine.refl_scratch_doubles).

Selection.  Of the M candidates the device keeps the min(M, keep) of largest e (the earlier index on equal e) and writes
them in ascending time, 6 doubles each: n, e[n], Bsum, cnt, m = the first index of max |x| over [max(n - d, 0), min(n + d,
L - 1)], float64(x[m]).  Unused rows hold -1 in the index and count fields and NaN in the others.

Per channel a record of 8 doubles: [0] n0, [1] Ed, [2] M, [3] the number kept, [4] the first candidate in time (-1: none;
independent of the selection), [5] Edir = sum of h2 over [max(n0 - Dw, 0), min(n0 + Dw, L - 1)], [6] Erest = sum of h2 over
(n0 + Dw, L), [7] the non-finite values among erow[0 .. R).  The two energy sums are float64 in an order that depends on
(L, n0, Dw) alone, without atomics.  A channel with L <= o (an empty one) has n0 = o, Ed = NaN, zeros and -1.
Every output of a channel is bit-identical whatever the batch, the channel's place in it or its alignment.

On the host: delay_ms = 1000 (n - n0) / fs, level_db = 10 log10(e / Ed), prominence_db = 10 log10(e cnt / Bsum) (+inf for
cnt == 0 or Bsum == 0), polarity = sign(x[m]), path_difference_m = speed_of_sound (343.0) * (n - n0) / fs, itdg_ms from
[4] (NaN: no candidate), drr_db = 10 log10(Edir / Erest) (+inf for Erest == 0), direct_seconds = n0 / fs,
candidates_found = M, and the curve 10 log10(erow[j Sc] / Ed), j Sc < R, Sc = curve_step_ms samples (1.0), float32,
decimated on the host from the fetched row (--no-curve: the row is not fetched).

No paper was consulted for the settings: a 1 ms Hann smoothing, a 2.5 ms direct window, a 6 dB prominence over +-5 ms and
a -40 dB floor over 200 ms are conventions of measurement practice, defaults of a settings object, not constants of the
kernel.

Per-channel status (bit flags; a channel with a non-zero status has NaN in every value and an empty list, the batch carries
on): 1 silent (|x[peak]| == 0), 2 too short (n0 + G >= L), 4 non-finite (record [7] > 0).

Command line (no plots): python -m analyse.reflections --input A.wav [B.wav ...] | --bundle DIR [--mono] [--smooth-ms 1]
  [--window hann|rect] [--direct-search-ms 2.5] [--direct-window-ms 2.5] [--guard-ms 1] [--separation-ms 0.5]
  [--background-ms 5] [--min-level-db -40] [--prominence-db 6] [--max-time-ms 200|none] [--max-reflections 16] [--onset-db -20]
  [--speed-of-sound 343] [--curve-step-ms 1] [--no-curve] [--expected-sample-rate 48000] [--json OUT.json]
"""
from __future__ import annotations

import argparse
import math
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _measure as M
from ..engine import (REFL_DOUBLES, REFL_FIELDS, REFL_MAX_BG, REFL_MAX_DIRECT, REFL_MAX_HALF, REFL_MAX_KEEP, REFL_MAX_SEP,
                      REFL_UNBOUNDED, refl_row_room)
from ._measure import MAX_BATCH_CHANNELS  # noqa: F401  (part of this module's surface)
from .echodensity import WINDOWS, window_weights
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ

STATUS_SILENT = 1
STATUS_TOO_SHORT = 2
STATUS_NON_FINITE = 4
_STATUS_WORDS = ((STATUS_SILENT, "silent"), (STATUS_TOO_SHORT, "too short"), (STATUS_NON_FINITE, "non-finite"))

MAX_HALF_SAMPLES = REFL_MAX_HALF
MAX_DIRECT_SAMPLES = REFL_MAX_DIRECT
MAX_BACKGROUND_SAMPLES = REFL_MAX_BG
MAX_SEPARATION_SAMPLES = REFL_MAX_SEP
MAX_REFLECTIONS = REFL_MAX_KEEP
UNBOUNDED = REFL_UNBOUNDED          # Tn when max_time_ms is None


def _positive(name: str, v) -> float:
    v = float(v)
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"{name} must be positive and finite, got {v}")
    return v


@dataclass(frozen=True)
class ReflectionSettings:
    smooth_ms: float = 1.0
    window: str = "hann"
    direct_search_ms: float = 2.5
    direct_window_ms: float = 2.5
    guard_ms: float = 1.0
    separation_ms: float = 0.5
    background_ms: float = 5.0
    min_level_db: float = -40.0
    prominence_db: float = 6.0
    max_time_ms: Optional[float] = 200.0           # search up to this time after the direct sound; None: the whole channel
    max_reflections: int = 16
    onset_db: float = -20.0
    speed_of_sound: float = 343.0
    curve_step_ms: float = 1.0
    use_mono_downmix_for_stereo: bool = False

    def __post_init__(self):
        vals = {k: _positive(k, getattr(self, k)) for k in ("smooth_ms", "direct_search_ms", "direct_window_ms", "guard_ms",
                                                            "separation_ms", "background_ms", "speed_of_sound",
                                                            "curve_step_ms")}
        if self.window not in WINDOWS:
            raise ValueError(f"window must be one of {WINDOWS}, got {self.window!r}")
        if vals["guard_ms"] < vals["separation_ms"]:
            raise ValueError(f"guard_ms must be at least separation_ms ({self.separation_ms}), got {self.guard_ms}")
        if vals["background_ms"] <= vals["separation_ms"]:
            raise ValueError(f"background_ms must be more than separation_ms ({self.separation_ms}), got {self.background_ms}")
        level, prominence, onset = float(self.min_level_db), float(self.prominence_db), float(self.onset_db)
        if not math.isfinite(level) or level > 0.0:
            raise ValueError(f"min_level_db must be a finite level <= 0 dB relative to the direct sound, got {self.min_level_db}")
        if not math.isfinite(prominence) or prominence < 0.0:
            raise ValueError(f"prominence_db must be finite and >= 0 dB, got {self.prominence_db}")
        tmax = self.max_time_ms
        if tmax is not None:
            tmax = float(tmax)
            if not (math.isfinite(tmax) and tmax >= 0.0):
                raise ValueError(f"max_time_ms must be finite and >= 0, or None, got {self.max_time_ms}")
        keep = self.max_reflections
        if isinstance(keep, bool) or int(keep) != keep or not 1 <= int(keep) <= MAX_REFLECTIONS:
            raise ValueError(f"max_reflections must be an integer 1..{MAX_REFLECTIONS}, got {self.max_reflections}")
        if not math.isfinite(onset) or onset > 0.0:
            raise ValueError(f"onset_db must be a finite level <= 0 dB relative to the peak, got {self.onset_db}")
        vals.update(min_level_db=level, prominence_db=prominence, max_time_ms=tmax, max_reflections=int(keep), onset_db=onset)
        for k, v in vals.items():
            object.__setattr__(self, k, v)

    @property
    def rel_energy(self) -> float:
        return 10.0 ** (self.onset_db / 10.0)

    @property
    def rel(self) -> float:
        return 10.0 ** (self.min_level_db / 10.0)

    @property
    def prom(self) -> float:
        return 10.0 ** (self.prominence_db / 10.0)


@dataclass(frozen=True)
class SampleCounts:
    """The settings in samples at one rate: d, D, Dw, G, S, B, Tn (UNBOUNDED: none), the curve's step Sc."""
    half: int
    direct: int
    direct_window: int
    guard: int
    separation: int
    background: int
    tn: int
    curve_step: int


@dataclass(frozen=True)
class Reflection:
    sample_index: int                              # n
    peak_sample_index: int                         # m: the largest |x| within the smoothing window of n
    delay_ms: float                                # from the direct sound
    level_db: float                                # 10 log10(e[n] / Ed)
    prominence_db: float                           # over the mean of the background; +inf: the background is silent
    polarity: int                                  # sign of x[m]: 1, -1 or 0
    path_difference_m: float


@dataclass(frozen=True, eq=False)
class ReflectionChannelResult:
    channel_name: str
    sample_rate_hz: int
    onset_samples: int
    onset_seconds: float
    status: int
    smooth_ms: float
    window: str
    window_samples: int                            # W
    direct_samples: int                            # n0; -1 for a channel with a status
    direct_seconds: float
    itdg_ms: float                                 # NaN: no candidate
    drr_db: float
    candidates_found: int                          # M
    reflections: Tuple[Reflection, ...]
    curve_step_seconds: float
    curve: Optional[np.ndarray] = None             # float32: 10 log10(e / Ed) per curve step from the onset; None: not kept


@dataclass
class ReflectionRecords:
    """What reflections_device leaves on the host: per channel the length, the onset, |x[peak]|, the kernel's record
    [n0, Ed, M, kept, first candidate, Edir, Erest, non-finite row entries], the kept list (keep rows of n, e, Bsum, cnt,
    peak index, peak sample) and the energy-time rows (float64, the first R values of each; None: not fetched)."""
    settings: ReflectionSettings
    counts: SampleCounts
    length: np.ndarray                             # int64 (nch,)
    onset: np.ndarray                              # int64 (nch,)
    peak_abs: np.ndarray                           # float32 (nch,)
    records: np.ndarray                            # float64 (nch, 8)
    lists: np.ndarray                              # float64 (nch, keep, 6)
    erow: Optional[np.ndarray]                     # float64, flat
    erow_off: np.ndarray                           # int64 (nch,)


def samples_of(ms: float, sample_rate_hz: float) -> int:
    """max(1, floor(ms * fs / 1000 + 0.5)) samples, float64 in exactly that order."""
    return max(1, int(math.floor(float(ms) * float(sample_rate_hz) / 1000.0 + 0.5)))


def half_window_samples(smooth_ms: float, sample_rate_hz: float) -> int:
    """d = max(1, floor(smooth_ms * fs / 2000 + 0.5)) samples (1 ms: 11 / 22 / 24 / 48 at 22.05 / 44.1 / 48 / 96 kHz);
    W = 2 d + 1."""
    return max(1, int(math.floor(float(smooth_ms) * float(sample_rate_hz) / 2000.0 + 0.5)))


def search_samples(max_time_ms: Optional[float], sample_rate_hz: float) -> int:
    """Tn = ceil(max_time_ms * fs / 1000); None: UNBOUNDED."""
    if max_time_ms is None:
        return UNBOUNDED
    return min(UNBOUNDED, int(math.ceil(float(max_time_ms) * float(sample_rate_hz) / 1000.0)))


def sample_counts(settings: ReflectionSettings, sample_rate_hz: float) -> SampleCounts:
    """The settings in samples; ValueError where a count leaves the kernel's bounds at this rate."""
    fs = float(sample_rate_hz)
    c = SampleCounts(half=half_window_samples(settings.smooth_ms, fs), direct=samples_of(settings.direct_search_ms, fs),
                     direct_window=samples_of(settings.direct_window_ms, fs), guard=samples_of(settings.guard_ms, fs),
                     separation=samples_of(settings.separation_ms, fs), background=samples_of(settings.background_ms, fs),
                     tn=search_samples(settings.max_time_ms, fs), curve_step=samples_of(settings.curve_step_ms, fs))
    if c.half > MAX_HALF_SAMPLES:
        raise ValueError(f"smooth_ms {settings.smooth_ms:g} is {2 * c.half + 1} samples at {fs:g} Hz: at most "
                         f"{2 * MAX_HALF_SAMPLES + 1}")
    if c.direct > MAX_DIRECT_SAMPLES:
        raise ValueError(f"direct_search_ms {settings.direct_search_ms:g} is {c.direct} samples at {fs:g} Hz: at most "
                         f"{MAX_DIRECT_SAMPLES}")
    if c.separation > MAX_SEPARATION_SAMPLES:
        raise ValueError(f"separation_ms {settings.separation_ms:g} is {c.separation} samples at {fs:g} Hz: at most "
                         f"{MAX_SEPARATION_SAMPLES}")
    if c.guard < c.separation:
        raise ValueError(f"guard_ms {settings.guard_ms:g} ({c.guard} samples) must be at least separation_ms "
                         f"({c.separation} samples)")
    if not c.separation < c.background <= MAX_BACKGROUND_SAMPLES:
        raise ValueError(f"background_ms {settings.background_ms:g} is {c.background} samples at {fs:g} Hz: more than the "
                         f"separation ({c.separation}) and at most {MAX_BACKGROUND_SAMPLES}")
    if c.direct_window >= 1 << 31 or c.guard >= 1 << 31:
        raise ValueError("direct_window_ms and guard_ms must stay below 2^31 samples")
    return c


def status_text(status: int) -> str:
    return M.status_text(status, _STATUS_WORDS)


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def reflections_device(eng, batch, sample_rate_hz: int, settings: Optional[ReflectionSettings] = None,
                       keep_curve: bool = True) -> ReflectionRecords:
    """Onset, energy-time row, kept reflections and record of every channel of a device batch, in ONE ira_reflections
    call.  keep_curve False: the rows stay on the device."""
    settings = settings or ReflectionSettings()
    c = sample_counts(settings, sample_rate_hz)
    nch, keep = batch.count, settings.max_reflections
    onset_dev, _, peak_abs_dev = eng.onset_index(batch, settings.rel_energy)
    erow = None
    if nch:
        erow_dev, erow_off, list_dev, rec_dev = eng.reflections(
            batch.x, batch.off, batch.length, onset_dev, window_weights(c.half, settings.window), c.half, c.direct,
            c.direct_window, c.guard, c.separation, c.background, c.tn, settings.rel, settings.prom, keep)
        records = rec_dev.cpu().numpy().reshape(nch, REFL_DOUBLES)
        lists = list_dev.cpu().numpy().reshape(nch, keep, REFL_FIELDS)
        if keep_curve:
            erow = erow_dev.cpu().numpy().reshape(-1)
    else:
        records, lists, erow_off = np.zeros((0, REFL_DOUBLES)), np.zeros((0, keep, REFL_FIELDS)), np.zeros(0, np.int64)
        if keep_curve:
            erow = np.zeros(0)
    return ReflectionRecords(settings=settings, counts=c, length=batch.length.astype(np.int64).copy(),
                             onset=onset_dev.cpu().numpy().copy(), peak_abs=peak_abs_dev.cpu().numpy().copy(),
                             records=records, lists=lists, erow=erow, erow_off=np.asarray(erow_off, dtype=np.int64))


# ---------------------------------------------------------------------------------------------------
# host: records -> results
# ---------------------------------------------------------------------------------------------------


def _db(num: float, den: float) -> float:
    """10 log10(num / den) for non-negative energies: +inf for den == 0 < num, -inf for num == 0 < den, NaN for 0 / 0."""
    num, den = float(num), float(den)
    if math.isnan(num) or math.isnan(den) or (num == 0.0 and den == 0.0) or (math.isinf(num) and math.isinf(den)):
        return float("nan")
    if den == 0.0 or math.isinf(num):
        return float("inf")
    if num == 0.0 or math.isinf(den):
        return float("-inf")
    return 10.0 * math.log10(num / den)


def reflection_results(res: ReflectionRecords, sample_rate_hz: int, channel_names: Sequence[str],
                       keep_curve: bool = True) -> List[ReflectionChannelResult]:
    fs = float(sample_rate_hz)
    st, c = res.settings, res.counts
    nan = float("nan")
    out = []
    for ch, name in enumerate(channel_names):
        rec = res.records[ch]
        onset, length, n0 = int(res.onset[ch]), int(res.length[ch]), int(rec[0])
        rows_held = int(refl_row_room(max(length - onset, 0), c.direct, c.tn, c.background))      # R
        status = 0
        if float(res.peak_abs[ch]) == 0.0:
            status |= STATUS_SILENT
        if n0 + c.guard >= length:
            status |= STATUS_TOO_SHORT
        if rec[7] > 0:
            status |= STATUS_NON_FINITE
        curve = None
        if keep_curve and res.erow is not None:
            a = int(res.erow_off[ch])
            if status:
                curve = np.full(len(range(0, rows_held, c.curve_step)), np.nan, dtype=np.float32)
            else:
                with np.errstate(divide="ignore", invalid="ignore"):
                    curve = (10.0 * np.log10(res.erow[a : a + rows_held : c.curve_step] / rec[1])).astype(np.float32)
        if status:
            direct, direct_s, itdg, drr, found, rows = -1, nan, nan, nan, 0, ()
        else:
            ed = float(rec[1])
            direct, direct_s, found = n0, n0 / fs, int(rec[2])
            itdg = 1000.0 * (float(rec[4]) - n0) / fs if rec[4] >= 0 else nan
            drr = _db(rec[5], rec[6])
            rows = []
            for n, e, bsum, cnt, m, xm in res.lists[ch][: max(int(rec[3]), 0)]:
                delay = (float(n) - n0) / fs
                prominence = float("inf") if cnt == 0 or bsum == 0.0 else _db(float(e) * float(cnt), bsum)
                rows.append(Reflection(sample_index=int(n), peak_sample_index=int(m), delay_ms=1000.0 * delay,
                                       level_db=_db(e, ed), prominence_db=prominence,
                                       polarity=int(xm > 0.0) - int(xm < 0.0), path_difference_m=st.speed_of_sound * delay))
            rows = tuple(rows)
        out.append(ReflectionChannelResult(
            channel_name=str(name), sample_rate_hz=int(sample_rate_hz), onset_samples=onset, onset_seconds=onset / fs,
            status=status, smooth_ms=st.smooth_ms, window=st.window, window_samples=2 * c.half + 1, direct_samples=direct,
            direct_seconds=direct_s, itdg_ms=itdg, drr_db=drr, candidates_found=found, reflections=rows,
            curve_step_seconds=c.curve_step / fs, curve=curve))
    return out


# ---------------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------------


def _results_of_batch(eng, batch, sample_rate_hz, names, settings, keep_curve: bool = True) -> List[ReflectionChannelResult]:
    return reflection_results(reflections_device(eng, batch, sample_rate_hz, settings, keep_curve), sample_rate_hz, names,
                              keep_curve)


def _results_without_curve(eng, batch, sample_rate_hz, names, settings) -> List[ReflectionChannelResult]:
    return _results_of_batch(eng, batch, sample_rate_hz, names, settings, keep_curve=False)


def analyse_reflections_batch(
    channels: Sequence[np.ndarray],
    sample_rate_hz: int,
    channel_names: Sequence[str],
    settings: Optional[ReflectionSettings] = None,
    keep_curve: bool = True,
) -> List[ReflectionChannelResult]:
    """Every channel through the device in batches of at most MAX_BATCH_CHANNELS channels."""
    return M.analyse_channel_batches(channels, sample_rate_hz, channel_names, settings or ReflectionSettings(),
                                     _results_of_batch if keep_curve else _results_without_curve)


def analyse_reflections_from_wav_file(
    input_wav_file_path: str | Path,
    settings: Optional[ReflectionSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
    keep_curve: bool = True,
) -> List[ReflectionChannelResult]:
    """One WAV file (mono or stereo, rate checked against expected_sample_rate_hz); channels named as by
    get_analysis_channels ("mono", "left", "right")."""
    return M.analyse_wav_file_channels(input_wav_file_path, settings or ReflectionSettings(), expected_sample_rate_hz,
                                       lambda c, fs, n, s: analyse_reflections_batch(c, fs, n, s, keep_curve))


def analyse_reflections_files(
    paths: Sequence[str | Path],
    settings: Optional[ReflectionSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
    keep_curve: bool = True,
) -> List[ReflectionChannelResult]:
    """Every channel of every file in one device batch per MAX_BATCH_CHANNELS channels; channels named
    "<file name>:<channel>"."""
    return M.analyse_file_channels(paths, settings or ReflectionSettings(), expected_sample_rate_hz,
                                   lambda c, fs, n, s: analyse_reflections_batch(c, fs, n, s, keep_curve))


def analyse_reflections_bundle(
    bundle_root: str | Path,
    settings: Optional[ReflectionSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
    keep_curve: bool = True,
) -> List[ReflectionChannelResult]:
    """The taps a bundle's meta.json lists (taps/<name>.wav), read by the native ingest (ingest.TapSet) a group at a
    time; channels named "<tap>:<channel>"."""
    return M.analyse_bundle_channels(bundle_root, settings or ReflectionSettings(), expected_sample_rate_hz,
                                     _results_of_batch if keep_curve else _results_without_curve)


# ---------------------------------------------------------------------------------------------------
# text, Markdown, JSON
# ---------------------------------------------------------------------------------------------------

_POLARITY = {1: "+", -1: "-", 0: "0"}


def _rows(r: ReflectionChannelResult) -> List[List[str]]:
    return [[str(i + 1), M.fmt(q.delay_ms, 3), M.fmt(q.level_db, 2), M.fmt(q.prominence_db, 2), _POLARITY[q.polarity],
             M.fmt(q.path_difference_m, 3)] for i, q in enumerate(r.reflections)]


def _head(r: ReflectionChannelResult, sep: str, end: str) -> str:
    direct = "NA" if r.direct_samples < 0 else f"{r.direct_samples} samples ({1000.0 * r.direct_seconds:.3f} ms)"
    return (f"Onset: {r.onset_samples} samples ({1000.0 * r.onset_seconds:.3f} ms){sep}Direct: {direct}{sep}"
            f"Status: {status_text(r.status)}{sep}Window: {r.window} {r.smooth_ms:g} ms ({r.window_samples} samples){end}")


def _tail(r: ReflectionChannelResult, sep: str, end: str) -> List[str]:
    return [f"ITDG: {M.fmt(r.itdg_ms, 3)} ms{sep}DRR: {M.fmt(r.drr_db, 2)} dB{sep}found {r.candidates_found}, "
            f"kept {len(r.reflections)}{end}"]


_COLUMNS = ["delay_ms", "level_dB", "prominence_dB", "polarity", "path_m"]


def summarise_reflections_text(channel_results: List[ReflectionChannelResult]) -> str:
    """
    Fixed text format, one block per channel followed by an empty line:
        [<channel name>]
        Onset: <o> samples (<ms, 3 decimals> ms)  Direct: <n0> samples (<ms, 3 decimals> ms) | NA  Status: ok | <flags> (<words>)  Window: <kind> <ms> ms (<W> samples)
        #  delay_ms  level_dB  prominence_dB  polarity  path_m
        <1, 2, ..>  <ms after the direct sound, 3 decimals>  <2 decimals>  <2 decimals | +inf>  <+ | - | 0>  <metres, 3 decimals>
        ITDG: <ms, 3 decimals> ms  DRR: <2 decimals> dB  found <M>, kept <K>
    Cells are separated by two spaces; NaN (no candidate, or a channel with a status) is "NA".
    """
    return M.join_blocks(M.text_block(r.channel_name, _head(r, "  ", ""), _COLUMNS, _rows(r), tail=_tail(r, "  ", ""),
                                      first="#") for r in channel_results)


def summarise_reflections_markdown(channel_results: List[ReflectionChannelResult]) -> str:
    """The same values as a Markdown section per channel: a '### <channel name>' heading, an onset / direct / status /
    window line, a table with a row per kept reflection and the ITDG / DRR line."""
    cols = ["delay (ms)", "level (dB)", "prominence (dB)", "polarity", "path (m)"]
    return M.join_blocks(M.markdown_block(r.channel_name, _head(r, ". ", "."), cols, _rows(r), tail=_tail(r, ". ", "."),
                                          first="#") for r in channel_results)


def reflections_results_to_json(channel_results: List[ReflectionChannelResult], with_curve: bool = True) -> Dict:
    """Plain JSON: NaN is null, an infinity "+inf" / "-inf".  The curve is written for the channels that kept one unless
    with_curve is False."""
    rows = []
    for r in channel_results:
        d = {"channel_name": r.channel_name, "sample_rate_hz": r.sample_rate_hz, "onset_samples": r.onset_samples,
             "onset_seconds": r.onset_seconds, "status": r.status, "smooth_ms": r.smooth_ms, "window": r.window,
             "window_samples": r.window_samples, "direct_samples": r.direct_samples,
             "direct_seconds": M.json_num(r.direct_seconds), "itdg_ms": M.json_num(r.itdg_ms), "drr_db": M.json_num(r.drr_db),
             "candidates_found": r.candidates_found,
             "reflections": [{"sample_index": q.sample_index, "peak_sample_index": q.peak_sample_index,
                              "delay_ms": M.json_num(q.delay_ms), "level_db": M.json_num(q.level_db),
                              "prominence_db": M.json_num(q.prominence_db), "polarity": q.polarity,
                              "path_difference_m": M.json_num(q.path_difference_m)} for q in r.reflections],
             "curve_step_seconds": r.curve_step_seconds}
        if with_curve and r.curve is not None:
            d["curve"] = [M.json_num(float(v)) for v in r.curve]
        rows.append(d)
    return {"reflections": rows}


def reflections_results_from_json(doc: Dict) -> List[ReflectionChannelResult]:
    return [ReflectionChannelResult(
        channel_name=d["channel_name"], sample_rate_hz=int(d["sample_rate_hz"]), onset_samples=int(d["onset_samples"]),
        onset_seconds=float(d["onset_seconds"]), status=int(d["status"]), smooth_ms=float(d["smooth_ms"]),
        window=str(d["window"]), window_samples=int(d["window_samples"]), direct_samples=int(d["direct_samples"]),
        direct_seconds=M.num_json(d["direct_seconds"]), itdg_ms=M.num_json(d["itdg_ms"]), drr_db=M.num_json(d["drr_db"]),
        candidates_found=int(d["candidates_found"]),
        reflections=tuple(Reflection(sample_index=int(q["sample_index"]), peak_sample_index=int(q["peak_sample_index"]),
                                     delay_ms=M.num_json(q["delay_ms"]), level_db=M.num_json(q["level_db"]),
                                     prominence_db=M.num_json(q["prominence_db"]), polarity=int(q["polarity"]),
                                     path_difference_m=M.num_json(q["path_difference_m"])) for q in d["reflections"]),
        curve_step_seconds=float(d["curve_step_seconds"]),
        curve=np.asarray([M.num_json(v) for v in d["curve"]], dtype=np.float32) if "curve" in d else None)
        for d in doc["reflections"]]


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def _time_or_none(text: str) -> Optional[float]:
    return None if text.strip().lower() == "none" else float(text)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.reflections",
        description="Early reflections per channel: the discrete reflections after the direct sound (delay, level, "
                    "prominence, polarity, path difference), the initial time delay gap and the direct-to-reverberant "
                    "ratio, read from a smoothed energy-time curve.")
    M.add_source_arguments(p)
    p.add_argument("--smooth-ms", type=float, default=1.0, help="length of the smoothing window of the curve (default: 1 ms)")
    p.add_argument("--window", choices=WINDOWS, default="hann", help="smoothing weights (default: hann)")
    p.add_argument("--direct-search-ms", type=float, default=2.5,
                   help="the direct sound is the curve's maximum within this time of the onset (default: 2.5 ms)")
    p.add_argument("--direct-window-ms", type=float, default=2.5,
                   help="half width of the direct sound's window of the direct-to-reverberant ratio (default: 2.5 ms)")
    p.add_argument("--guard-ms", type=float, default=1.0, help="no reflection within this time of the direct sound (default: 1 ms)")
    p.add_argument("--separation-ms", type=float, default=0.5,
                   help="a reflection is the curve's maximum within this time on both sides (default: 0.5 ms)")
    p.add_argument("--background-ms", type=float, default=5.0,
                   help="the background a reflection stands out of reaches this far on both sides (default: 5 ms)")
    p.add_argument("--min-level-db", type=float, default=-40.0,
                   help="lowest level of a reflection relative to the direct sound (default: -40 dB)")
    p.add_argument("--prominence-db", type=float, default=6.0,
                   help="a reflection exceeds the mean of its background by this much (default: 6 dB)")
    p.add_argument("--max-time-ms", type=_time_or_none, default=200.0, metavar="MS|none",
                   help="search up to this time after the direct sound (default: 200 ms; none: the whole channel)")
    p.add_argument("--max-reflections", type=int, default=16,
                   help=f"keep the strongest 1 to {MAX_REFLECTIONS} reflections (default: 16)")
    p.add_argument("--onset-db", type=float, default=-20.0,
                   help="onset: first sample within this level of the peak (default: -20 dB, ISO 3382-1)")
    p.add_argument("--speed-of-sound", type=float, default=343.0, help="metres per second, for the path difference (default: 343)")
    p.add_argument("--curve-step-ms", type=float, default=1.0, help="distance of the curve's points in the JSON (default: 1 ms)")
    p.add_argument("--no-curve", action="store_true", help="leave the energy-time curve out of the JSON")
    M.add_output_arguments(p)
    return p


def settings_from_args(args) -> ReflectionSettings:
    return ReflectionSettings(smooth_ms=args.smooth_ms, window=args.window, direct_search_ms=args.direct_search_ms,
                              direct_window_ms=args.direct_window_ms, guard_ms=args.guard_ms,
                              separation_ms=args.separation_ms, background_ms=args.background_ms,
                              min_level_db=args.min_level_db, prominence_db=args.prominence_db, max_time_ms=args.max_time_ms,
                              max_reflections=args.max_reflections, onset_db=args.onset_db,
                              speed_of_sound=args.speed_of_sound, curve_step_ms=args.curve_step_ms,
                              use_mono_downmix_for_stereo=bool(args.mono))


def main(argv: Optional[Sequence[str]] = None) -> None:
    parser = build_parser()
    curve = not bool(parser.parse_args(argv).no_curve)
    M.run_cli(parser, argv, settings_from_args,
              lambda paths, st, fs: analyse_reflections_files(paths, st, fs, keep_curve=curve),
              lambda root, st, fs: analyse_reflections_bundle(root, st, fs, keep_curve=curve),
              summarise_reflections_text, lambda results: reflections_results_to_json(results, curve))


if __name__ == "__main__":
    main()
