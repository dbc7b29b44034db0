"""
Frequency-dependent-window (FDW) response per channel: level, phase and group delay on a logarithmic frequency grid,
each point seen through a window a fixed number of CYCLES long around the direct sound -- many milliseconds at 30 Hz, so
that room modes are resolved, a fraction of a millisecond at 10 kHz, so that reflections are gated out and the
loudspeaker's own response remains.  frequency_response.py and filterplot.py use one window for all frequencies.

For a channel x (float32) of L samples at the sample rate fs:

  grid     f_j = f_min * 2^(j / points_per_octave), j = 0, 1, .. while f_j <= min(f_max, fs / 2)  (float64)
           rho_j = f_j / fs
           H_j = clip(rint(cycles * fs / (2 f_j)), rint(min_window_ms * fs / 1000), rint(max_window_ms * fs / 1000)),
           at least 1: the HALF width in samples.  The window of point j is the 2 H_j + 1 samples centred on p; the two
           millisecond limits bound the half width, the reach of the window to either side of the centre.
           (defaults: cycles 15, 48 points per octave, 20 Hz .. 20 kHz, 0 .. 500 ms: 479 points, H 18000 .. 18 at 48 kHz)
  centre   p = the peak (first index of max |x|) or the onset as in energy.py (eng.onset_index(batch, rel_energy),
           onset_db = -20 by default).  It is read on the device and comes to the host only for the result.
  terms    k = -H .. H, i = p + k; a term with i outside [0, L) contributes nothing
  weight   hann: w(k) = 0.5 + 0.5 cospi(k / (H + 1)) (no zero end points; 1 at the centre)  |  rect: w = 1
  phasor   e^{-2 pi i k rho}, the turn count k rho reduced exactly before the sine and cosine (include/ira.h)
  sums     v = w(k) float64(x[i]):  S0 = sum v e^{-2 pi i k rho},  S1 = sum k v e^{-2 pi i k rho},  A = sum |v|,
           N = the number of terms inside the channel                          (ira_fdw_response, float64)

From the six fields, in float64 NumPy on the host (fdw_arithmetic; exactly restatable):

  level_db             10 log10(max(|S0|^2, 10^(magnitude_floor_db / 10))),  |S0|^2 = Re^2 + Im^2
  phase_deg            atan2(Im S0, Re S0) in degrees.  k counts from the centre, so the phase is relative to it: the bulk
                       delay of the measurement is already gone.
  unwrapped_phase_deg  numpy.unwrap along the grid over the points that have a value
  group_delay_seconds  Re(S1 conj(S0)) / |S0|^2 / fs, relative to the centre.  This is the analytic derivative -d(phase) /
                       d(omega) of the sum AT FIXED WINDOW, not a finite difference along the grid (whose neighbouring
                       points have different windows).
  window_ms            1000 (2 H + 1) / fs
  clipped              N < 2 H + 1: the window reaches past an end of the channel
  cancellation         |S0| / A in [0, 1]: how much of the summed magnitude survives; a small value says the level is
                       the difference of large terms
  Every value of a point is NaN where S0 == 0 (nothing inside the window, digital silence) or a sum is not finite (a NaN
  or an infinity inside the window; no other point is touched).

The defaults are conventions of measurement tools ("frequency-dependent window, N cycles"), not citations.

Command line (no plots): python -m analyse.fdw --input A.wav [B.wav ...] | --bundle DIR [--mono] [--cycles 15]
  [--points-per-octave 48] [--f-min 20] [--f-max 20000] [--window hann|rect] [--min-window-ms 0] [--max-window-ms 500]
  [--centre peak|onset] [--onset-db -20] [--no-curve] [--expected-sample-rate 48000] [--json OUT.json]
"""
from __future__ import annotations

import argparse
import math
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _measure as M
from ..engine import FDW_FIELDS, FDW_MAX_HALF, FDW_MAX_POINTS, FDW_WINDOWS
from ._measure import MAX_BATCH_CHANNELS  # noqa: F401  (part of this module's surface)
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ

WINDOWS = FDW_WINDOWS
CENTRES = ("peak", "onset")
MAX_POINTS = FDW_MAX_POINTS
MAX_HALF_SAMPLES = FDW_MAX_HALF
_CURVES = ("frequencies_hz", "half_samples", "window_ms", "level_db", "phase_deg", "unwrapped_phase_deg",
           "group_delay_seconds", "cancellation", "clipped")


@dataclass(frozen=True)
class FdwSettings:
    cycles: float = 15.0
    points_per_octave: int = 48
    f_min_hz: float = 20.0
    f_max_hz: float = 20000.0                      # clipped to the Nyquist frequency of the channel
    window: str = "hann"
    min_window_ms: float = 0.0                     # bounds of the half width, the window's reach to either side
    max_window_ms: float = 500.0
    centre: str = "peak"
    onset_db: float = -20.0
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

        cycles, f_min, f_max = number("cycles", True), number("f_min_hz", True), number("f_max_hz", True)
        w_min, w_max, onset, floor = (number("min_window_ms"), number("max_window_ms", True), number("onset_db"),
                                      number("magnitude_floor_db"))
        ppo = self.points_per_octave
        if isinstance(ppo, bool) or not isinstance(ppo, (int, np.integer)) or ppo < 1:
            raise ValueError(f"points_per_octave must be a whole number >= 1, got {ppo!r}")
        if f_max < f_min:
            raise ValueError(f"f_max_hz must be at least f_min_hz, got {self.f_min_hz} .. {self.f_max_hz}")
        if self.window not in WINDOWS:
            raise ValueError(f"window must be one of {WINDOWS}, got {self.window!r}")
        if w_min < 0.0 or w_max < w_min:
            raise ValueError(f"min_window_ms must be >= 0 and at most max_window_ms, got {self.min_window_ms} .. "
                             f"{self.max_window_ms}")
        if self.centre not in CENTRES:
            raise ValueError(f"centre must be one of {CENTRES}, got {self.centre!r}")
        if onset > 0.0:
            raise ValueError(f"onset_db must be a finite level <= 0 dB relative to the peak, got {self.onset_db}")
        for k, v in (("cycles", cycles), ("points_per_octave", int(ppo)), ("f_min_hz", f_min), ("f_max_hz", f_max),
                     ("min_window_ms", w_min), ("max_window_ms", w_max), ("onset_db", onset), ("magnitude_floor_db", floor)):
            object.__setattr__(self, k, v)

    @property
    def rel_energy(self) -> float:
        return 10.0 ** (self.onset_db / 10.0)


@dataclass(frozen=True, eq=False)
class FdwChannelResult:
    channel_name: str
    sample_rate_hz: int
    centre: str                                    # "peak" | "onset"
    centre_samples: int
    centre_seconds: float
    cycles: float
    window: str
    points_per_octave: int
    # per frequency point; None: not kept (a JSON written with --no-curve)
    frequencies_hz: Optional[np.ndarray] = None
    half_samples: Optional[np.ndarray] = None      # int64: H
    window_ms: Optional[np.ndarray] = None
    level_db: Optional[np.ndarray] = None
    phase_deg: Optional[np.ndarray] = None
    unwrapped_phase_deg: Optional[np.ndarray] = None
    group_delay_seconds: Optional[np.ndarray] = None
    cancellation: Optional[np.ndarray] = None
    clipped: Optional[np.ndarray] = None           # bool


@dataclass
class FdwRecords:
    """What fdw_device leaves on the host: the grid, per channel the length and the centre, and the kernel's six fields
    per (channel, point): Re S0, Im S0, Re S1, Im S1, A, N."""
    settings: FdwSettings
    frequencies_hz: np.ndarray                     # float64 (J,)
    rho: np.ndarray                                # float64 (J,)
    half: np.ndarray                               # int32 (J,)
    length: np.ndarray                             # int64 (nch,)
    centre: np.ndarray                             # int64 (nch,)
    sums: np.ndarray                               # float64 (nch, J, 6)


def fdw_grid(settings: FdwSettings, sample_rate_hz: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(f_j, rho_j = f_j / fs, H_j) of the settings at a sample rate: float64, float64, int32.  f_j = f_min 2^(j / ppo)
    while f_j <= min(f_max, fs / 2); H_j = rint(cycles fs / (2 f_j)) clipped to the two limits in samples, at least 1."""
    fs = float(sample_rate_hz)
    if not (math.isfinite(fs) and fs > 0.0):
        raise ValueError(f"the sample rate must be positive, got {sample_rate_hz}")
    top = min(settings.f_max_hz, fs / 2.0)
    count = 0 if settings.f_min_hz > top else int(math.floor(math.log2(top / settings.f_min_hz) * settings.points_per_octave)) + 2
    f = settings.f_min_hz * 2.0 ** (np.arange(count, dtype=np.float64) / float(settings.points_per_octave))
    f = f[f <= top]
    if f.size == 0:
        raise ValueError(f"no frequency point: f_min_hz {settings.f_min_hz:g} lies above min(f_max_hz, fs / 2) = {top:g}")
    if f.size > MAX_POINTS:
        raise ValueError(f"{f.size} frequency points, at most {MAX_POINTS}")
    lo = max(1.0, float(np.rint(settings.min_window_ms * fs / 1000.0)))
    hi = max(lo, float(np.rint(settings.max_window_ms * fs / 1000.0)))
    half = np.clip(np.rint(settings.cycles * fs / (2.0 * f)), lo, hi)
    if half.max() > MAX_HALF_SAMPLES:
        raise ValueError(f"a half width of {int(half.max())} samples, at most {MAX_HALF_SAMPLES}: lower cycles or "
                         f"max_window_ms, or raise f_min_hz")
    return f, f / fs, half.astype(np.int32)


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def fdw_device(eng, batch, sample_rate_hz: int, settings: Optional[FdwSettings] = None) -> FdwRecords:
    """Centre and the six sums of every (channel, point) of a device batch, in ONE ira_fdw_response call."""
    settings = settings or FdwSettings()
    f, rho, half = fdw_grid(settings, sample_rate_hz)
    nch = batch.count
    onset_dev, peak_dev, _ = eng.onset_index(batch, settings.rel_energy)
    centre_dev = peak_dev if settings.centre == "peak" else onset_dev
    if nch:
        sums = eng.fdw_response(batch.x, batch.off, batch.length, centre_dev, rho, half, settings.window)
        sums = sums.cpu().numpy().reshape(nch, f.size, FDW_FIELDS)
    else:
        sums = np.zeros((0, f.size, FDW_FIELDS))
    return FdwRecords(settings=settings, frequencies_hz=f, rho=rho, half=half,
                      length=batch.length.astype(np.int64).copy(), centre=centre_dev.cpu().numpy().astype(np.int64).copy(),
                      sums=sums)


# ---------------------------------------------------------------------------------------------------
# host: sums -> results
# ---------------------------------------------------------------------------------------------------


def fdw_arithmetic(sums: np.ndarray, half: np.ndarray, sample_rate_hz: float, magnitude_floor_db: float = -120.0) -> Dict:
    """The curves of one channel from its (J, 6) sums and the half widths, float64 NumPy (the module's docstring states
    each line): level_db, phase_deg, unwrapped_phase_deg, group_delay_seconds, window_ms, clipped, cancellation."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, FDW_FIELDS)
    half = np.asarray(half, dtype=np.int64).reshape(-1)
    fs = float(sample_rate_hz)
    re0, im0, re1, im1, a, n = (s[:, q] for q in range(FDW_FIELDS))
    ok = np.all(np.isfinite(s[:, :5]), axis=1) & ((re0 != 0.0) | (im0 != 0.0))
    nan = np.full(s.shape[0], np.nan)
    with np.errstate(all="ignore"):
        power = re0 * re0 + im0 * im0
        level = np.where(ok, 10.0 * np.log10(np.maximum(power, 10.0 ** (float(magnitude_floor_db) / 10.0))), nan)
        phase = np.where(ok, np.degrees(np.arctan2(im0, re0)), nan)
        unwrapped = nan.copy()
        unwrapped[ok] = np.degrees(np.unwrap(np.arctan2(im0[ok], re0[ok])))
        delay = np.where(ok, (re1 * re0 + im1 * im0) / power / fs, nan)
        cancellation = np.where(ok, np.hypot(re0, im0) / a, nan)
    return dict(level_db=level, phase_deg=phase, unwrapped_phase_deg=unwrapped, group_delay_seconds=delay,
                window_ms=1000.0 * (2.0 * half + 1.0) / fs, clipped=n < 2 * half + 1, cancellation=cancellation)


def fdw_results(res: FdwRecords, sample_rate_hz: int, channel_names: Sequence[str], keep_curve: bool = True) -> List["FdwChannelResult"]:
    fs = float(sample_rate_hz)
    st = res.settings
    out = []
    for ch, name in enumerate(channel_names):
        curves = {}
        if keep_curve:
            curves = fdw_arithmetic(res.sums[ch], res.half, fs, st.magnitude_floor_db)
            curves.update(frequencies_hz=res.frequencies_hz.copy(), half_samples=res.half.astype(np.int64))
        p = int(res.centre[ch])
        out.append(FdwChannelResult(channel_name=str(name), sample_rate_hz=int(sample_rate_hz), centre=st.centre,
                                    centre_samples=p, centre_seconds=p / fs, cycles=st.cycles, window=st.window,
                                    points_per_octave=st.points_per_octave, **curves))
    return out


# ---------------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------------


def _results_of_batch(eng, batch, sample_rate_hz, names, settings) -> List[FdwChannelResult]:
    return fdw_results(fdw_device(eng, batch, sample_rate_hz, settings), sample_rate_hz, names)


def analyse_fdw_batch(
    channels: Sequence[np.ndarray],
    sample_rate_hz: int,
    channel_names: Sequence[str],
    settings: Optional[FdwSettings] = None,
) -> List[FdwChannelResult]:
    """Every channel through the device in batches of at most MAX_BATCH_CHANNELS channels."""
    return M.analyse_channel_batches(channels, sample_rate_hz, channel_names, settings or FdwSettings(), _results_of_batch)


def analyse_fdw_for_channel(
    samples: np.ndarray,
    sample_rate_hz: int,
    channel_name: str,
    settings: Optional[FdwSettings] = None,
) -> FdwChannelResult:
    return analyse_fdw_batch([samples], sample_rate_hz, [channel_name], settings)[0]


def analyse_fdw_from_wav_file(
    input_wav_file_path: str | Path,
    settings: Optional[FdwSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[FdwChannelResult]:
    """One WAV file (mono or stereo, rate checked against expected_sample_rate_hz); channels named as by
    get_analysis_channels ("mono", "left", "right")."""
    return M.analyse_wav_file_channels(input_wav_file_path, settings or FdwSettings(), expected_sample_rate_hz,
                                       analyse_fdw_batch)


def analyse_fdw_files(
    paths: Sequence[str | Path],
    settings: Optional[FdwSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[FdwChannelResult]:
    """Every channel of every file in one device batch per MAX_BATCH_CHANNELS channels; channels named
    "<file name>:<channel>"."""
    return M.analyse_file_channels(paths, settings or FdwSettings(), expected_sample_rate_hz, analyse_fdw_batch)


def analyse_fdw_bundle(
    bundle_root: str | Path,
    settings: Optional[FdwSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[FdwChannelResult]:
    """The taps a bundle's meta.json lists (taps/<name>.wav), read by the native ingest (ingest.TapSet) a group at a
    time; channels named "<tap>:<channel>"."""
    return M.analyse_bundle_channels(bundle_root, settings or FdwSettings(), expected_sample_rate_hz, _results_of_batch)


# ---------------------------------------------------------------------------------------------------
# text, Markdown, JSON
# ---------------------------------------------------------------------------------------------------


def _rows(r: FdwChannelResult) -> List[List[str]]:
    """One row per octave from the first grid point (every points_per_octave-th point); none without the curve."""
    if r.frequencies_hz is None:
        return []
    return [[f"{r.frequencies_hz[j]:.1f}", M.fmt(float(r.window_ms[j]), 3), M.fmt(float(r.level_db[j]), 2),
             M.fmt(float(r.phase_deg[j]), 1), M.fmt(1000.0 * float(r.group_delay_seconds[j]), 3),
             M.fmt(float(r.cancellation[j]), 4), "yes" if r.clipped[j] else "no"]
            for j in range(0, len(r.frequencies_hz), r.points_per_octave)]


def _head(r: FdwChannelResult, sep: str, end: str) -> str:
    points = "NA" if r.frequencies_hz is None else str(len(r.frequencies_hz))
    return (f"Centre: {r.centre} at {r.centre_samples} samples ({1000.0 * r.centre_seconds:.3f} ms){sep}"
            f"Window: {r.window} {r.cycles:g} cycles{sep}Points: {points} ({r.points_per_octave} per octave){end}")


def _tail(r: FdwChannelResult, end: str) -> List[str]:
    if r.frequencies_hz is None:
        return []
    return [f"clipped points: {int(np.count_nonzero(r.clipped))}, without a value: "
            f"{int(np.count_nonzero(np.isnan(r.level_db)))}{end}"]


_COLUMNS = ["window_ms", "level_dB", "phase_deg", "group_delay_ms", "cancellation", "clipped"]
_MD_COLUMNS = ["window (ms)", "level (dB)", "phase (deg)", "group delay (ms)", "cancellation", "clipped"]


def summarise_fdw_text(channel_results: List[FdwChannelResult]) -> str:
    """
    Fixed text format, one block per channel followed by an empty line:
        [<channel name>]
        Centre: <kind> at <p> samples (<p / fs in ms, 3 decimals> ms)  Window: <kind> <cycles> cycles  Points: <J> (<ppo> per octave)
        freq_Hz  window_ms  level_dB  phase_deg  group_delay_ms  cancellation  clipped
        <f, 1 decimal>  <3 decimals>  <2 decimals>  <1 decimal>  <3 decimals>  <4 decimals>  yes | no      (one row per octave)
        clipped points: <count>, without a value: <count>
    Cells are separated by two spaces; NaN is "NA".  The group delay is relative to the centre.
    """
    return M.join_blocks(M.text_block(r.channel_name, _head(r, "  ", ""), _COLUMNS, _rows(r), tail=_tail(r, ""),
                                      first="freq_Hz") for r in channel_results)


def summarise_fdw_markdown(channel_results: List[FdwChannelResult]) -> str:
    """The same values as a Markdown section per channel: a '### <channel name>' heading, the centre / window / points
    line, a table with a row per octave and the counts line."""
    return M.join_blocks(M.markdown_block(r.channel_name, _head(r, ". ", "."), _MD_COLUMNS, _rows(r), tail=_tail(r, "."),
                                          first="freq (Hz)") for r in channel_results)


def fdw_results_to_json(channel_results: List[FdwChannelResult], with_curve: bool = True) -> Dict:
    """Plain JSON: NaN is null.  The curves are written for the channels that kept them unless with_curve is False."""
    rows = []
    for r in channel_results:
        d = {"channel_name": r.channel_name, "sample_rate_hz": r.sample_rate_hz, "centre": r.centre,
             "centre_samples": r.centre_samples, "centre_seconds": r.centre_seconds, "cycles": r.cycles, "window": r.window,
             "points_per_octave": r.points_per_octave}
        if with_curve and r.frequencies_hz is not None:
            for name in _CURVES:
                v = getattr(r, name)
                if name == "clipped":
                    d[name] = [bool(b) for b in v]
                elif name == "half_samples":
                    d[name] = [int(h) for h in v]
                else:
                    d[name] = [M.json_num(float(x)) for x in v]
        rows.append(d)
    return {"fdw": rows}


def fdw_results_from_json(doc: Dict) -> List[FdwChannelResult]:
    out = []
    for d in doc["fdw"]:
        curves = {}
        if "frequencies_hz" in d:
            for name in _CURVES:
                if name == "clipped":
                    curves[name] = np.asarray(d[name], dtype=bool)
                elif name == "half_samples":
                    curves[name] = np.asarray(d[name], dtype=np.int64)
                else:
                    curves[name] = np.asarray([M.num_json(v) for v in d[name]], dtype=np.float64)
        out.append(FdwChannelResult(
            channel_name=d["channel_name"], sample_rate_hz=int(d["sample_rate_hz"]), centre=str(d["centre"]),
            centre_samples=int(d["centre_samples"]), centre_seconds=float(d["centre_seconds"]), cycles=float(d["cycles"]),
            window=str(d["window"]), points_per_octave=int(d["points_per_octave"]), **curves))
    return out


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.fdw",
        description="Frequency-dependent-window response per channel: level, phase and group delay on a logarithmic "
                    "grid, each point through a window a fixed number of cycles long around the direct sound.")
    M.add_source_arguments(p)
    p.add_argument("--cycles", type=float, default=15.0, help="window length in cycles of each frequency (default: 15)")
    p.add_argument("--points-per-octave", type=int, default=48, help="grid density (default: 48)")
    p.add_argument("--f-min", type=float, default=20.0, help="first grid frequency in Hz (default: 20)")
    p.add_argument("--f-max", type=float, default=20000.0,
                   help="the grid ends at or below this frequency and the Nyquist frequency (default: 20000)")
    p.add_argument("--window", choices=WINDOWS, default="hann", help="window weights (default: hann)")
    p.add_argument("--min-window-ms", type=float, default=0.0,
                   help="shortest reach of a window to either side of the centre (default: 0)")
    p.add_argument("--max-window-ms", type=float, default=500.0,
                   help="longest reach of a window to either side of the centre (default: 500 ms)")
    p.add_argument("--centre", choices=CENTRES, default="peak", help="window centre: the peak or the onset (default: peak)")
    p.add_argument("--onset-db", type=float, default=-20.0,
                   help="onset: first sample within this level of the peak (default: -20 dB, ISO 3382-1)")
    p.add_argument("--no-curve", action="store_true", help="leave the per-frequency curves out of the JSON")
    M.add_output_arguments(p)
    return p


def settings_from_args(args) -> FdwSettings:
    return FdwSettings(cycles=args.cycles, points_per_octave=args.points_per_octave, f_min_hz=args.f_min,
                       f_max_hz=args.f_max, window=args.window, min_window_ms=args.min_window_ms,
                       max_window_ms=args.max_window_ms, centre=args.centre, onset_db=args.onset_db,
                       use_mono_downmix_for_stereo=bool(args.mono))


def main(argv: Optional[Sequence[str]] = None) -> None:
    parser = build_parser()
    no_curve = bool(parser.parse_args(argv).no_curve)
    M.run_cli(parser, argv, settings_from_args, analyse_fdw_files, analyse_fdw_bundle, summarise_fdw_text,
              lambda results: fdw_results_to_json(results, not no_curve))


if __name__ == "__main__":
    main()
