"""
Burst decay per channel: a constant-Q map of level over frequency and TIME IN PERIODS, every frequency seen through a
window a fixed number of CYCLES long that is moved along the channel from the direct sound on.  spectrogram.py and
waterfall.py use one n_fft for every frequency; fdw.py has constant-Q windows, but at one instant.  The map shows which
modes ring and for how many cycles, whether a driver stores energy, and (with a negative start) pre-ringing.

For a channel x (float32) of L samples at the sample rate fs:

  grid     f_j, rho_j = f_j / fs and the half width H_j exactly by fdw.fdw_grid's rules (fdw.py states them)
           (defaults: cycles 8, 24 points per octave, 20 Hz .. 20 kHz, window reach 0 .. 500 ms: at 48 kHz 240 points,
           H 9600 .. 10)
  centre   p = the peak (first index of max |x|) or the onset as in energy.py (eng.onset_index(batch, rel_energy),
           onset_db = -20 by default).  It is read on the device and comes to the host only for the result.
  axis     t_m = start + m * step (float64), m = 0 .. M - 1, M = floor((stop - start) / step + 1e-9) + 1
           axis "periods" (default): start 0, stop 30, step 0.5 (M = 61);  delta[j, m] = rint(t_m * fs / f_j)
           axis "ms":                start 0, stop 300, step 2 (M = 151);  delta[j, m] = rint(t_m * fs / 1000), every j alike
           float64 in exactly the order written, stored as int32.  start may be negative: pre-ringing.
  wavelet  g_j(k) = w(k) e^{-2 pi i r(k)}, k = -H_j .. H_j, w and r exactly as include/ira.h states them for
           ira_fdw_response: hann as sinpi((H + 1 - |k|) / (2 H + 2))^2, rect = 1; the turn count k rho reduced with the
           fma split, then sincospi(2 r)                                            (ira_burst_table, float64, made once)
  cell     c = p + delta[j, m];  S[j, m] = sum over k of g_j(k) * float64(x[c + k]);  a term with c + k outside [0, L)
           contributes nothing and is not read.  The phase is relative to the cell's own centre.      (ira_burst_decay)

From S, in float64 NumPy on the host (burst_arithmetic; exactly restatable):

  N            max(0, min(c + H, L - 1) - max(c - H, 0) + 1), the terms inside the channel (no device output needed)
  clipped      N < 2 H + 1
  level_db     10 log10(max(|S|^2, 10^(magnitude_floor_db / 10))),  |S|^2 = Re^2 + Im^2
  relative_db  level_db - (the channel's largest finite level_db)
  phase_deg    atan2(Im S, Re S) in degrees
  A cell is NaN where S == 0 (nothing inside the window, digital silence) or a part of S is not finite (a NaN or an
  infinity inside the window).  No other cell is touched.
  decay[j]     over the cells of row j that have a value: from the row's maximum (its first occurrence) on, the first
               cell whose level is at least decay_db (default 30) below that maximum; the axis position is interpolated
               linearly in dB between that cell and the cell with a value before it.  NaN if the row never gets there (or
               has no value).  Reported in periods and in seconds: seconds = periods / f_j.

A unit impulse at p gives S[j, m] = g_j(-delta[j, m]): at t = 0 the level is 0 dB at every frequency, which is why there is
no further normalisation.  The defaults are conventions of measurement tools ("burst decay", "wavelet"), not citations
(PAPERS.md).

Command line (no plots): python -m analyse.burstdecay --input A.wav [B.wav ...] | --bundle DIR [--mono] [--cycles 8]
  [--points-per-octave 24] [--f-min 20] [--f-max 20000] [--window hann|rect] [--min-window-ms 0] [--max-window-ms 500]
  [--axis periods|ms] [--start S] [--stop E] [--step D] [--centre peak|onset] [--onset-db -20] [--decay-db 30] [--no-map]
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
from ..engine import BURST_MAX_DELTA, BURST_MAX_STEPS
from ._measure import MAX_BATCH_CHANNELS  # noqa: F401  (part of this module's surface)
from .fdw import CENTRES, WINDOWS, FdwSettings, fdw_grid
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ

AXES = ("periods", "ms")
AXIS_DEFAULTS = {"periods": (0.0, 30.0, 0.5), "ms": (0.0, 300.0, 2.0)}         # start, stop, step
MAX_STEPS = BURST_MAX_STEPS
MAX_DELTA_SAMPLES = BURST_MAX_DELTA
_POINT_CURVES = ("frequencies_hz", "half_samples", "peak_level_db", "peak_position", "decay_periods", "decay_seconds")
_MAPS = ("level_db", "relative_db", "phase_deg", "clipped")


@dataclass(frozen=True)
class BurstDecaySettings:
    cycles: float = 8.0
    points_per_octave: int = 24
    f_min_hz: float = 20.0
    f_max_hz: float = 20000.0                      # clipped to the Nyquist frequency of the channel
    window: str = "hann"
    min_window_ms: float = 0.0                     # bounds of the half width, the window's reach to either side
    max_window_ms: float = 500.0
    centre: str = "peak"
    onset_db: float = -20.0
    axis: str = "periods"
    start: Optional[float] = None                  # None: the axis's default (AXIS_DEFAULTS)
    stop: Optional[float] = None
    step: Optional[float] = None
    decay_db: float = 30.0
    magnitude_floor_db: float = -120.0
    use_mono_downmix_for_stereo: bool = False

    def __post_init__(self):
        def number(name, positive=False):
            try:
                v = float(getattr(self, name))
            except (TypeError, ValueError):
                raise ValueError(f"{name} must be a number, got {getattr(self, name)!r}") from None
            if not math.isfinite(v) or (positive and v <= 0.0):
                raise ValueError(f"{name} must be finite{' and > 0' if positive else ''}, got {getattr(self, name)}")
            return v

        self.grid_settings                                                  # the grid's own fields, by FdwSettings' rules
        if self.axis not in AXES:
            raise ValueError(f"axis must be one of {AXES}, got {self.axis!r}")
        decay, floor = number("decay_db", True), number("magnitude_floor_db")
        values = {k: (None if getattr(self, k) is None else number(k, k == "step")) for k in ("start", "stop", "step")}
        for k, v in (("cycles", float(self.cycles)), ("points_per_octave", int(self.points_per_octave)),
                     ("f_min_hz", float(self.f_min_hz)), ("f_max_hz", float(self.f_max_hz)),
                     ("min_window_ms", float(self.min_window_ms)), ("max_window_ms", float(self.max_window_ms)),
                     ("onset_db", float(self.onset_db)), ("decay_db", decay), ("magnitude_floor_db", floor), *values.items()):
            object.__setattr__(self, k, v)
        start, stop, step = self.axis_range
        if stop < start:
            raise ValueError(f"stop must be at least start, got {start:g} .. {stop:g}")
        if self.steps > MAX_STEPS:
            raise ValueError(f"{self.steps} steps, at most {MAX_STEPS}: raise step or shorten start .. stop")

    @property
    def grid_settings(self) -> FdwSettings:
        """The fields fdw.fdw_grid reads, validated as FdwSettings validates them."""
        return FdwSettings(cycles=self.cycles, points_per_octave=self.points_per_octave, f_min_hz=self.f_min_hz,
                           f_max_hz=self.f_max_hz, window=self.window, min_window_ms=self.min_window_ms,
                           max_window_ms=self.max_window_ms, centre=self.centre, onset_db=self.onset_db)

    @property
    def rel_energy(self) -> float:
        return 10.0 ** (self.onset_db / 10.0)

    @property
    def axis_range(self) -> Tuple[float, float, float]:
        """(start, stop, step) with the axis's defaults where a field is None."""
        return tuple(d if v is None else v for v, d in zip((self.start, self.stop, self.step), AXIS_DEFAULTS[self.axis]))

    @property
    def steps(self) -> int:
        start, stop, step = self.axis_range
        return int(math.floor((stop - start) / step + 1e-9)) + 1


@dataclass(frozen=True, eq=False)
class BurstDecayChannelResult:
    channel_name: str
    sample_rate_hz: int
    centre: str                                    # "peak" | "onset"
    centre_samples: int
    centre_seconds: float
    cycles: float
    window: str
    points_per_octave: int
    axis: str                                      # "periods" | "ms"
    decay_db: float
    axis_values: np.ndarray                        # float64 (M,): t_m in periods or milliseconds
    # per frequency point
    frequencies_hz: np.ndarray
    half_samples: np.ndarray                       # int64: H
    peak_level_db: np.ndarray                      # the row's maximum (NaN: no cell of the row has a value)
    peak_position: np.ndarray                      # its axis position
    decay_periods: np.ndarray
    decay_seconds: np.ndarray
    # per (point, step); None: not kept (a JSON written with --no-map)
    level_db: Optional[np.ndarray] = None
    relative_db: Optional[np.ndarray] = None
    phase_deg: Optional[np.ndarray] = None
    clipped: Optional[np.ndarray] = None           # bool


@dataclass
class BurstDecayRecords:
    """What burst_decay_device leaves on the host: the grid and the axis, per channel the length and the centre, and the
    kernel's (Re S, Im S) per (channel, point, step)."""
    settings: BurstDecaySettings
    frequencies_hz: np.ndarray                     # float64 (J,)
    rho: np.ndarray                                # float64 (J,)
    half: np.ndarray                               # int32 (J,)
    axis_values: np.ndarray                        # float64 (M,)
    delta: np.ndarray                              # int32 (J, M)
    length: np.ndarray                             # int64 (nch,)
    centre: np.ndarray                             # int64 (nch,)
    sums: np.ndarray                               # float64 (nch, J, M, 2)


def burst_grid(settings: BurstDecaySettings, sample_rate_hz: float):
    """(f_j, rho_j, H_j, t_m, delta[j, m]) of the settings at a sample rate: float64 (J,), float64 (J,), int32 (J,), float64
    (M,), int32 (J, M).  The first three are fdw.fdw_grid's; t_m = start + m * step; delta = rint(t_m * fs / f_j) on the
    periods axis, rint(t_m * fs / 1000) on the ms axis."""
    f, rho, half = fdw_grid(settings.grid_settings, sample_rate_hz)
    fs = float(sample_rate_hz)
    start, _, step = settings.axis_range
    t = start + np.arange(settings.steps, dtype=np.float64) * step
    if settings.axis == "periods":
        delta = np.rint(t[None, :] * fs / f[:, None])
    else:
        delta = np.broadcast_to(np.rint(t * fs / 1000.0)[None, :], (f.size, t.size))
    if np.abs(delta).max() > MAX_DELTA_SAMPLES:
        raise ValueError(f"a step {int(np.abs(delta).max())} samples from the centre, at most {MAX_DELTA_SAMPLES}: shorten "
                         f"start .. stop or raise f_min_hz")
    return f, rho, half, t, np.ascontiguousarray(delta, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def burst_decay_device(eng, batch, sample_rate_hz: int, settings: Optional[BurstDecaySettings] = None) -> BurstDecayRecords:
    """Centre and S of every (channel, point, step) of a device batch: ONE ira_burst_table call and one ira_burst_decay
    call (more only where the map of the batch exceeds engine.BURST_MAX_OUT_BYTES)."""
    settings = settings or BurstDecaySettings()
    f, rho, half, t, delta = burst_grid(settings, sample_rate_hz)
    nch = batch.count
    onset_dev, peak_dev, _ = eng.onset_index(batch, settings.rel_energy)
    centre_dev = peak_dev if settings.centre == "peak" else onset_dev
    if nch:
        table = eng.burst_table(rho, half, settings.window)
        parts = eng.burst_decay(batch.x, batch.off, batch.length, centre_dev, table, delta)
        sums = np.concatenate([p.cpu().numpy().reshape(-1, f.size, t.size, 2) for p in parts], axis=0)
    else:
        sums = np.zeros((0, f.size, t.size, 2))
    return BurstDecayRecords(settings=settings, frequencies_hz=f, rho=rho, half=half, axis_values=t, delta=delta,
                             length=batch.length.astype(np.int64).copy(),
                             centre=centre_dev.cpu().numpy().astype(np.int64).copy(), sums=sums)


# ---------------------------------------------------------------------------------------------------
# host: sums -> results
# ---------------------------------------------------------------------------------------------------


def terms_inside(centre: int, delta: np.ndarray, half: np.ndarray, length: int) -> np.ndarray:
    """N[j, m] = max(0, min(c + H, L - 1) - max(c - H, 0) + 1), c = p + delta[j, m] (int64)."""
    c = int(centre) + np.asarray(delta, dtype=np.int64)
    h = np.asarray(half, dtype=np.int64).reshape(-1, 1)
    return np.maximum(0, np.minimum(c + h, int(length) - 1) - np.maximum(c - h, 0) + 1)


def burst_arithmetic(sums: np.ndarray, half: np.ndarray, delta: np.ndarray, frequencies_hz: np.ndarray,
                     axis_values: np.ndarray, axis: str, centre: int, length: int, decay_db: float = 30.0,
                     magnitude_floor_db: float = -120.0) -> Dict:
    """The maps and the per-point values of one channel from its (J, M, 2) sums, float64 NumPy (the module's docstring
    states each line): level_db, relative_db, phase_deg, clipped (J, M); peak_level_db, peak_position, decay_periods,
    decay_seconds (J,)."""
    s = np.asarray(sums, dtype=np.float64)
    re, im = s[..., 0], s[..., 1]
    f = np.asarray(frequencies_hz, dtype=np.float64).reshape(-1)
    t = np.asarray(axis_values, dtype=np.float64).reshape(-1)
    if axis not in AXES:
        raise ValueError(f"axis must be one of {AXES}, got {axis!r}")
    n = terms_inside(centre, delta, half, length)
    ok = np.isfinite(re) & np.isfinite(im) & ((re != 0.0) | (im != 0.0))
    nan = np.full(re.shape, np.nan)
    with np.errstate(all="ignore"):
        power = re * re + im * im
        level = np.where(ok, 10.0 * np.log10(np.maximum(power, 10.0 ** (float(magnitude_floor_db) / 10.0))), nan)
        phase = np.where(ok, np.degrees(np.arctan2(im, re)), nan)
    top = float(np.max(level[ok])) if ok.any() else float("nan")
    peak_level, peak_pos, decay = (np.full(f.size, np.nan) for _ in range(3))
    for j in range(f.size):
        cells = np.flatnonzero(ok[j])
        if cells.size == 0:
            continue
        row = level[j, cells]
        first = int(np.argmax(row))                                          # the first occurrence of the maximum
        peak_level[j], peak_pos[j] = row[first], t[cells[first]]
        below = np.flatnonzero(row[first + 1:] <= row[first] - float(decay_db))
        if below.size:
            b = first + 1 + int(below[0])
            a = b - 1
            ta, tb = t[cells[a]], t[cells[b]]
            decay[j] = ta + (row[first] - float(decay_db) - row[a]) / (row[b] - row[a]) * (tb - ta)
    if axis == "periods":
        periods, seconds = decay, decay / f
    else:
        seconds = decay / 1000.0
        periods = seconds * f
    return dict(level_db=level, relative_db=level - top, phase_deg=phase,
                clipped=n < 2 * np.asarray(half, dtype=np.int64).reshape(-1, 1) + 1, peak_level_db=peak_level,
                peak_position=peak_pos, decay_periods=periods, decay_seconds=seconds)


def burst_decay_results(res: BurstDecayRecords, sample_rate_hz: int, channel_names: Sequence[str],
                        keep_map: bool = True) -> List[BurstDecayChannelResult]:
    fs = float(sample_rate_hz)
    st = res.settings
    out = []
    for ch, name in enumerate(channel_names):
        p = int(res.centre[ch])
        values = burst_arithmetic(res.sums[ch], res.half, res.delta, res.frequencies_hz, res.axis_values, st.axis, p,
                                  int(res.length[ch]), st.decay_db, st.magnitude_floor_db)
        if not keep_map:
            for k in _MAPS:
                values.pop(k)
        out.append(BurstDecayChannelResult(
            channel_name=str(name), sample_rate_hz=int(sample_rate_hz), centre=st.centre, centre_samples=p,
            centre_seconds=p / fs, cycles=st.cycles, window=st.window, points_per_octave=st.points_per_octave, axis=st.axis,
            decay_db=st.decay_db, axis_values=res.axis_values.copy(), frequencies_hz=res.frequencies_hz.copy(),
            half_samples=res.half.astype(np.int64), **values))
    return out


# ---------------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------------


def _results_of_batch(eng, batch, sample_rate_hz, names, settings) -> List[BurstDecayChannelResult]:
    return burst_decay_results(burst_decay_device(eng, batch, sample_rate_hz, settings), sample_rate_hz, names)


def analyse_burst_decay_batch(
    channels: Sequence[np.ndarray],
    sample_rate_hz: int,
    channel_names: Sequence[str],
    settings: Optional[BurstDecaySettings] = None,
) -> List[BurstDecayChannelResult]:
    """Every channel through the device in batches of at most MAX_BATCH_CHANNELS channels."""
    return M.analyse_channel_batches(channels, sample_rate_hz, channel_names, settings or BurstDecaySettings(),
                                     _results_of_batch)


def analyse_burst_decay_for_channel(
    samples: np.ndarray,
    sample_rate_hz: int,
    channel_name: str,
    settings: Optional[BurstDecaySettings] = None,
) -> BurstDecayChannelResult:
    return analyse_burst_decay_batch([samples], sample_rate_hz, [channel_name], settings)[0]


def analyse_burst_decay_from_wav_file(
    input_wav_file_path: str | Path,
    settings: Optional[BurstDecaySettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[BurstDecayChannelResult]:
    """One WAV file (mono or stereo, rate checked against expected_sample_rate_hz); channels named as by
    get_analysis_channels ("mono", "left", "right")."""
    return M.analyse_wav_file_channels(input_wav_file_path, settings or BurstDecaySettings(), expected_sample_rate_hz,
                                       analyse_burst_decay_batch)


def analyse_burst_decay_files(
    paths: Sequence[str | Path],
    settings: Optional[BurstDecaySettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[BurstDecayChannelResult]:
    """Every channel of every file in one device batch per MAX_BATCH_CHANNELS channels; channels named
    "<file name>:<channel>"."""
    return M.analyse_file_channels(paths, settings or BurstDecaySettings(), expected_sample_rate_hz, analyse_burst_decay_batch)


def analyse_burst_decay_bundle(
    bundle_root: str | Path,
    settings: Optional[BurstDecaySettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[BurstDecayChannelResult]:
    """The taps a bundle's meta.json lists (taps/<name>.wav), read by the native ingest (ingest.TapSet) a group at a
    time; channels named "<tap>:<channel>"."""
    return M.analyse_bundle_channels(bundle_root, settings or BurstDecaySettings(), expected_sample_rate_hz, _results_of_batch)


# ---------------------------------------------------------------------------------------------------
# text, JSON
# ---------------------------------------------------------------------------------------------------

_COLUMNS = ["window_ms", "peak_dB", "peak_at", "decay_periods", "decay_ms", "clipped_cells"]


def _rows(r: BurstDecayChannelResult) -> List[List[str]]:
    """One row per octave from the first grid point (every points_per_octave-th point)."""
    rows = []
    for j in range(0, len(r.frequencies_hz), r.points_per_octave):
        clipped = "NA" if r.clipped is None else str(int(np.count_nonzero(r.clipped[j])))
        rows.append([f"{r.frequencies_hz[j]:.1f}", M.fmt(1000.0 * (2.0 * float(r.half_samples[j]) + 1.0) / r.sample_rate_hz, 3),
                     M.fmt(float(r.peak_level_db[j]), 2), M.fmt(float(r.peak_position[j]), 2),
                     M.fmt(float(r.decay_periods[j]), 2), M.fmt(1000.0 * float(r.decay_seconds[j]), 3), clipped])
    return rows


def summarise_burst_decay_text(channel_results: List[BurstDecayChannelResult]) -> str:
    """
    Fixed text format, one block per channel followed by an empty line:
        [<channel name>]
        Centre: <kind> at <p> samples (<ms, 3 decimals> ms)  Window: <kind> <cycles> cycles  Points: <J> (<ppo> per octave)  Axis: <kind> <first> .. <last>, <M> steps  Decay: -<decay_db> dB
        freq_Hz  window_ms  peak_dB  peak_at  decay_periods  decay_ms  clipped_cells
        <f, 1 decimal>  <3 decimals>  <2 decimals>  <2 decimals>  <2 decimals>  <3 decimals>  <count | NA>   (one row per octave)
        points that reach the decay: <count> of <J>
    Cells are separated by two spaces; NaN is "NA".  peak_at is the axis position of the row's maximum.
    """
    blocks = []
    for r in channel_results:
        t = r.axis_values
        head = (f"Centre: {r.centre} at {r.centre_samples} samples ({1000.0 * r.centre_seconds:.3f} ms)  Window: {r.window} "
                f"{r.cycles:g} cycles  Points: {len(r.frequencies_hz)} ({r.points_per_octave} per octave)  Axis: {r.axis} "
                f"{t[0]:g} .. {t[-1]:g}, {len(t)} steps  Decay: -{r.decay_db:g} dB")
        tail = [f"points that reach the decay: {int(np.count_nonzero(~np.isnan(r.decay_periods)))} of {len(r.frequencies_hz)}"]
        blocks.append(M.text_block(r.channel_name, head, _COLUMNS, _rows(r), tail=tail, first="freq_Hz"))
    return M.join_blocks(blocks)


def burst_decay_results_to_json(channel_results: List[BurstDecayChannelResult], with_map: bool = True) -> Dict:
    """Plain JSON: NaN is null.  The maps are written for the channels that kept them unless with_map is False."""
    rows = []
    for r in channel_results:
        d = {"channel_name": r.channel_name, "sample_rate_hz": r.sample_rate_hz, "centre": r.centre,
             "centre_samples": r.centre_samples, "centre_seconds": r.centre_seconds, "cycles": r.cycles, "window": r.window,
             "points_per_octave": r.points_per_octave, "axis": r.axis, "decay_db": r.decay_db,
             "axis_values": [float(v) for v in r.axis_values]}
        for name in _POINT_CURVES:
            v = getattr(r, name)
            d[name] = [int(h) for h in v] if name == "half_samples" else [M.json_num(float(x)) for x in v]
        if with_map and r.level_db is not None:
            for name in _MAPS:
                v = getattr(r, name)
                d[name] = [[bool(b) for b in row] for row in v] if name == "clipped" else \
                    [[M.json_num(float(x)) for x in row] for row in v]
        rows.append(d)
    return {"burst_decay": rows}


def burst_decay_results_from_json(doc: Dict) -> List[BurstDecayChannelResult]:
    out = []
    for d in doc["burst_decay"]:
        values = {}
        for name in _POINT_CURVES:
            values[name] = np.asarray(d[name], dtype=np.int64) if name == "half_samples" else \
                np.asarray([M.num_json(v) for v in d[name]], dtype=np.float64)
        if "level_db" in d:
            shape = (len(d["frequencies_hz"]), len(d["axis_values"]))
            for name in _MAPS:
                values[name] = np.asarray(d[name], dtype=bool).reshape(shape) if name == "clipped" else \
                    np.asarray([[M.num_json(v) for v in row] for row in d[name]], dtype=np.float64).reshape(shape)
        out.append(BurstDecayChannelResult(
            channel_name=d["channel_name"], sample_rate_hz=int(d["sample_rate_hz"]), centre=str(d["centre"]),
            centre_samples=int(d["centre_samples"]), centre_seconds=float(d["centre_seconds"]), cycles=float(d["cycles"]),
            window=str(d["window"]), points_per_octave=int(d["points_per_octave"]), axis=str(d["axis"]),
            decay_db=float(d["decay_db"]), axis_values=np.asarray(d["axis_values"], dtype=np.float64), **values))
    return out


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.burstdecay",
        description="Burst decay per channel: level over frequency and time in periods, every frequency through a window "
                    "a fixed number of cycles long that moves along the channel from the direct sound on.")
    M.add_source_arguments(p)
    p.add_argument("--cycles", type=float, default=8.0, help="window length in cycles of each frequency (default: 8)")
    p.add_argument("--points-per-octave", type=int, default=24, help="grid density (default: 24)")
    p.add_argument("--f-min", type=float, default=20.0, help="first grid frequency in Hz (default: 20)")
    p.add_argument("--f-max", type=float, default=20000.0,
                   help="the grid ends at or below this frequency and the Nyquist frequency (default: 20000)")
    p.add_argument("--window", choices=WINDOWS, default="hann", help="window weights (default: hann)")
    p.add_argument("--min-window-ms", type=float, default=0.0,
                   help="shortest reach of a window to either side of its centre (default: 0)")
    p.add_argument("--max-window-ms", type=float, default=500.0,
                   help="longest reach of a window to either side of its centre (default: 500 ms)")
    p.add_argument("--axis", choices=AXES, default="periods",
                   help="time axis: periods of each frequency, or milliseconds (default: periods)")
    p.add_argument("--start", type=float, default=None, help="first axis position; may be negative (default: 0)")
    p.add_argument("--stop", type=float, default=None, help="last axis position (default: 30 periods | 300 ms)")
    p.add_argument("--step", type=float, default=None, help="distance between axis positions (default: 0.5 periods | 2 ms)")
    p.add_argument("--centre", choices=CENTRES, default="peak", help="t = 0: the peak or the onset (default: peak)")
    p.add_argument("--onset-db", type=float, default=-20.0,
                   help="onset: first sample within this level of the peak (default: -20 dB, ISO 3382-1)")
    p.add_argument("--decay-db", type=float, default=30.0,
                   help="the decay of a frequency: where its level has fallen this far below its maximum (default: 30 dB)")
    p.add_argument("--no-map", action="store_true", help="leave the per-cell maps out of the JSON")
    M.add_output_arguments(p)
    return p


def settings_from_args(args) -> BurstDecaySettings:
    return BurstDecaySettings(cycles=args.cycles, points_per_octave=args.points_per_octave, f_min_hz=args.f_min,
                              f_max_hz=args.f_max, window=args.window, min_window_ms=args.min_window_ms,
                              max_window_ms=args.max_window_ms, centre=args.centre, onset_db=args.onset_db, axis=args.axis,
                              start=args.start, stop=args.stop, step=args.step, decay_db=args.decay_db,
                              use_mono_downmix_for_stereo=bool(args.mono))


def main(argv: Optional[Sequence[str]] = None) -> None:
    parser = build_parser()
    no_map = bool(parser.parse_args(argv).no_map)
    M.run_cli(parser, argv, settings_from_args, analyse_burst_decay_files, analyse_burst_decay_bundle,
              summarise_burst_decay_text, lambda results: burst_decay_results_to_json(results, not no_map))


if __name__ == "__main__":
    main()
