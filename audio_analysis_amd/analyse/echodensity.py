"""
Normalized echo density (NED) per channel and the mixing time read from it: when does an impulse response stop being a
set of discrete reflections and become a dense, Gaussian-like tail.

diffusion.py mirrors the reference's "echo density proxy", a float32 count over hard 50 ms windows against a user
threshold, and echo.py / energy.py / lundeby.py are built on energy: none of them sees texture.  The accepted measure is
the normalized echo density of Abel & Huang (AES 121st Convention, 2006): the weighted fraction of the
samples of a sliding window that lie outside the window's own standard deviation, over the value a Gaussian signal
gives, erfc(1 / sqrt 2).  The mixing time is the first time the profile reaches 1 (the definition Lindau, Kosanke &
Weinzierl use, JAES 2012).

For a channel x (float32) of L samples; o its broadband onset as in energy.py and echo.py (eng.onset_index(batch,
rel_energy), onset_db = -20 by default); fs the sample rate:

  delta  = max(1, floor(window_ms * fs / 2000.0 + 0.5))     W = 2 delta + 1 samples   (window_ms default 20)
  w[k]   = 0.5 - 0.5 cos(2 pi (k + 1) / (W + 1))  (hann, no zero end points)  |  1.0 (rect)     k = 0 .. W-1, float64,
           built ON THE HOST
  S      = max(1, floor(step_ms * fs / 1000.0 + 0.5))  samples        (step_ms default 1; 0 means S = 1)
  K      = 0 if L <= o else min(floor((L - 1 - o) / S) + 1, Kmax)
  Kmax   = 1 + floor(ceil(max_time_ms * fs / 1000) / S), unbounded for None (default None)
  centre c_j = o + j S,  j = 0 .. K-1;  window indices i = c_j - delta .. c_j + delta clipped to [0, L)  (k = i - (c_j - delta))
  h2[i]  = float64(x[i])^2                      (exact: a float32 squared fits a float64)
  A_j    = sum w[k]           B_j = sum w[k] h2[i]               over the clipped window, k ascending
  in[i]  = h2[i] A_j  >  B_j (1 + 2^-32)                          ("|x| exceeds sigma": no sqrt, no division)
  C_j    = sum w[k] over the clipped window where in[i], k ascending
  eta_j  = (C_j / A_j) / 0.31731050786291415                      (erfc(1 / sqrt 2) as that float64 literal)
  eta_j  = NaN where B_j == 0 (digital silence in the window) or B_j is not finite
  profile[j] = float32(eta_j)

Edge windows are renormalised by A_j, not zero-extended: the profile starts at the onset even when the onset is sample 0.
The guard factor 1 + 2^-32 makes the natural exact ties deterministic -- a constant-magnitude signal and a window of one
sample, where h2 A == B in exact arithmetic and the rounding of B would otherwise decide each comparison: such a signal
gives eta = 0 everywhere.  The guard moves sigma by about 1 part in 10^10, which has no acoustic meaning.

All of it is formed on the device (ira_echo_density), K from the onset included: the onset never returns to the host
first, so a channel's profile row is sized for onset 0 and only its first K values are the profile.  The two NaN kinds
are told apart in the float32 profile as stored by their payload (engine.NED_NAN_SILENT, engine.NED_NAN_NONFINITE).

Per channel the device also reduces, FROM THE FLOAT32 PROFILE AS STORED (a user who reads both sees consistent numbers),
a record of 8 doubles: [0] K, [1] positions with B == 0, [2] positions with B not finite, [3] the maximum of the finite
profile values (NaN if none), [4] its first index (-1 if none), [5..7] the first j with profile[j] >= thresholds[t] for
up to 3 thresholds (-1 for no crossing and for unused slots; NaN never crosses).  On the host
mixing_time_seconds[t] = j S / fs, measured from the onset (NaN: no crossing), eta_max, tau_max_seconds = (index of the
maximum) S / fs, onset_samples and the profile with step_seconds = S / fs.

No copy of either paper was at hand, so the window length (20 ms), its kind (Hann) and the threshold (1.0) are the
defaults of a settings object, not constants of the kernel.

Per-channel status (bit flags; a channel with a non-zero status has NaN in every value, the batch carries on): 1 silent
(|x[peak]| == 0), 2 too short (L - o < W: not one full window), 4 non-finite (record [2] > 0).

Command line (no plots): python -m analyse.echodensity --input A.wav [B.wav ...] | --bundle DIR [--mono] [--window-ms 20]
  [--window hann|rect] [--step-ms 1] [--max-time-ms T] [--thresholds 1.0 ...] [--onset-db -20] [--no-profile]
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
from ..engine import NED_DOUBLES, NED_MAX_DELTA, NED_MAX_THRESHOLDS, ned_positions
from ._measure import MAX_BATCH_CHANNELS  # noqa: F401  (part of this module's surface)
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ

STATUS_SILENT = 1
STATUS_TOO_SHORT = 2
STATUS_NON_FINITE = 4
_STATUS_WORDS = ((STATUS_SILENT, "silent"), (STATUS_TOO_SHORT, "too short"), (STATUS_NON_FINITE, "non-finite"))

WINDOWS = ("hann", "rect")
MAX_THRESHOLDS = NED_MAX_THRESHOLDS
MAX_DELTA_SAMPLES = NED_MAX_DELTA   # IRA_NED_MAX_DELTA: W <= 4097; 20 ms at 192 kHz is 3841
UNBOUNDED = 1 << 31                 # Kmax when max_time_ms is None: no channel has as many positions
GAUSSIAN_FRACTION = 0.31731050786291415   # erfc(1 / sqrt 2)


@dataclass(frozen=True)
class EchoDensitySettings:
    window_ms: float = 20.0
    window: str = "hann"
    step_ms: float = 1.0                           # 0: one sample
    max_time_ms: Optional[float] = None            # evaluate up to this time after the onset; None: the whole channel
    thresholds: Tuple[float, ...] = (1.0,)
    onset_db: float = -20.0
    use_mono_downmix_for_stereo: bool = False

    def __post_init__(self):
        win_ms, step = float(self.window_ms), float(self.step_ms)
        if not (math.isfinite(win_ms) and win_ms > 0.0):
            raise ValueError(f"window_ms must be positive and finite, got {self.window_ms}")
        if self.window not in WINDOWS:
            raise ValueError(f"window must be one of {WINDOWS}, got {self.window!r}")
        if not (math.isfinite(step) and step >= 0.0):
            raise ValueError(f"step_ms must be finite and >= 0 (0: one sample), got {self.step_ms}")
        tmax = self.max_time_ms
        if tmax is not None:
            tmax = float(tmax)
            if not (math.isfinite(tmax) and tmax >= 0.0):
                raise ValueError(f"max_time_ms must be finite and >= 0, or None, got {self.max_time_ms}")
        try:
            thr = tuple(float(v) for v in self.thresholds)
        except (TypeError, ValueError):
            raise ValueError(f"thresholds must be a sequence of 1 to {MAX_THRESHOLDS} numbers") from None
        if not 1 <= len(thr) <= MAX_THRESHOLDS:
            raise ValueError(f"thresholds needs 1 to {MAX_THRESHOLDS} entries, got {len(thr)}")
        if not all(math.isfinite(v) and v > 0.0 for v in thr):
            raise ValueError(f"thresholds must be finite and > 0, got {thr}")
        if any(b <= a for a, b in zip(thr, thr[1:])):
            raise ValueError(f"thresholds must ascend, got {thr}")
        onset = float(self.onset_db)
        if not math.isfinite(onset) or onset > 0.0:
            raise ValueError(f"onset_db must be a finite level <= 0 dB relative to the peak, got {self.onset_db}")
        for k, v in (("window_ms", win_ms), ("step_ms", step), ("max_time_ms", tmax), ("thresholds", thr),
                     ("onset_db", onset)):
            object.__setattr__(self, k, v)

    @property
    def rel_energy(self) -> float:
        return 10.0 ** (self.onset_db / 10.0)


@dataclass(frozen=True, eq=False)
class EchoDensityChannelResult:
    channel_name: str
    sample_rate_hz: int
    onset_samples: int
    onset_seconds: float
    status: int
    window_ms: float
    window: str
    window_samples: int                            # W
    step_seconds: float                            # S / fs
    thresholds: Tuple[float, ...]
    mixing_time_seconds: Tuple[float, ...]         # per threshold, from the onset; NaN: the profile never reaches it
    eta_max: float
    tau_max_seconds: float
    profile: Optional[np.ndarray] = None           # float32 (K,): eta per step from the onset, as stored; None: not kept


@dataclass
class EchoDensityRecords:
    """What echo_density_device leaves on the host: per channel the length, the onset, |x[peak]|, the kernel's record
    [K, positions of digital silence, positions with a non-finite sum, max eta, its first index, first index at or
    above each threshold (-1: none)] and the profile rows (float32, the first K values of each)."""
    settings: EchoDensitySettings
    length: np.ndarray                             # int64 (nch,)
    onset: np.ndarray                              # int64 (nch,)
    peak_abs: np.ndarray                           # float32 (nch,)
    records: np.ndarray                            # float64 (nch, 8)
    profile: np.ndarray                            # float32, flat
    profile_off: np.ndarray                        # int64 (nch,)
    delta: int
    step: int


def half_window_samples(window_ms: float, sample_rate_hz: float) -> int:
    """delta = max(1, floor(window_ms * fs / 2000 + 0.5)) samples, float64 in exactly that order (20 ms: 221 / 441 / 480 /
    960 at 22.05 / 44.1 / 48 / 96 kHz); W = 2 delta + 1."""
    return max(1, int(math.floor(float(window_ms) * float(sample_rate_hz) / 2000.0 + 0.5)))


def step_samples(step_ms: float, sample_rate_hz: float) -> int:
    """S = max(1, floor(step_ms * fs / 1000 + 0.5)) samples; step_ms = 0 means one sample."""
    return max(1, int(math.floor(float(step_ms) * float(sample_rate_hz) / 1000.0 + 0.5)))


def max_positions(max_time_ms: Optional[float], sample_rate_hz: float, step: int) -> int:
    """Kmax = 1 + floor(ceil(max_time_ms * fs / 1000) / S): the profile reaches max_time_ms; None: unbounded."""
    if max_time_ms is None:
        return UNBOUNDED
    return min(UNBOUNDED, 1 + int(math.ceil(float(max_time_ms) * float(sample_rate_hz) / 1000.0)) // int(step))


def position_count(length: int, onset: int, step: int, kmax: int) -> int:
    """K = 0 if L <= o else min(floor((L - 1 - o) / S) + 1, Kmax)."""
    return int(ned_positions(length, onset, step, kmax))


def window_weights(delta: int, window: str) -> np.ndarray:
    """The W = 2 delta + 1 float64 weights: hann without its zero end points, 0.5 - 0.5 cos(2 pi (k + 1) / (W + 1)), or
    ones."""
    if window not in WINDOWS:
        raise ValueError(f"window must be one of {WINDOWS}, got {window!r}")
    w = 2 * int(delta) + 1
    if window == "rect":
        return np.ones(w, dtype=np.float64)
    k = np.arange(w, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (k + 1.0) / (w + 1.0))


def status_text(status: int) -> str:
    return M.status_text(status, _STATUS_WORDS)


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def echo_density_device(eng, batch, sample_rate_hz: int, settings: Optional[EchoDensitySettings] = None) -> EchoDensityRecords:
    """Onset, profile and record of every channel of a device batch, in ONE ira_echo_density call."""
    settings = settings or EchoDensitySettings()
    delta = half_window_samples(settings.window_ms, sample_rate_hz)
    if delta > MAX_DELTA_SAMPLES:
        raise ValueError(f"window_ms {settings.window_ms:g} is {2 * delta + 1} samples at {sample_rate_hz:g} Hz: at most "
                         f"{2 * MAX_DELTA_SAMPLES + 1}")
    step = step_samples(settings.step_ms, sample_rate_hz)
    kmax = max_positions(settings.max_time_ms, sample_rate_hz, step)
    nch = batch.count
    onset_dev, _, peak_abs_dev = eng.onset_index(batch, settings.rel_energy)
    if nch:
        prof_dev, prof_off, rec_dev = eng.echo_density(batch.x, batch.off, batch.length, onset_dev,
                                                       window_weights(delta, settings.window), delta, step, kmax,
                                                       settings.thresholds)
        records, profile = rec_dev.cpu().numpy().reshape(nch, NED_DOUBLES), prof_dev.cpu().numpy().reshape(-1)
    else:
        records, profile, prof_off = np.zeros((0, NED_DOUBLES)), np.zeros(0, np.float32), np.zeros(0, np.int64)
    return EchoDensityRecords(settings=settings, length=batch.length.astype(np.int64).copy(),
                              onset=onset_dev.cpu().numpy().copy(), peak_abs=peak_abs_dev.cpu().numpy().copy(),
                              records=records, profile=profile, profile_off=np.asarray(prof_off, dtype=np.int64),
                              delta=delta, step=step)


# ---------------------------------------------------------------------------------------------------
# host: records -> results
# ---------------------------------------------------------------------------------------------------


def echo_density_results(res: EchoDensityRecords, sample_rate_hz: int, channel_names: Sequence[str],
                         keep_profile: bool = True) -> List[EchoDensityChannelResult]:
    fs = float(sample_rate_hz)
    st = res.settings
    w = 2 * res.delta + 1
    nan = float("nan")
    out = []
    for ch, name in enumerate(channel_names):
        rec = res.records[ch]
        onset, k = int(res.onset[ch]), max(int(rec[0]), 0)
        status = 0
        if float(res.peak_abs[ch]) == 0.0:
            status |= STATUS_SILENT
        if int(res.length[ch]) - onset < w:
            status |= STATUS_TOO_SHORT
        if rec[2] > 0:
            status |= STATUS_NON_FINITE
        if status:
            mixing, eta_max, tau_max = tuple([nan] * len(st.thresholds)), nan, nan
            profile = np.full(k, np.nan, dtype=np.float32)
        else:
            mixing = tuple(float(j) * res.step / fs if j >= 0 else nan for j in rec[5 : 5 + len(st.thresholds)])
            eta_max, tau_max = float(rec[3]), (float(rec[4]) * res.step / fs if rec[4] >= 0 else nan)
            a = int(res.profile_off[ch])
            profile = res.profile[a : a + k].copy()
        out.append(EchoDensityChannelResult(
            channel_name=str(name), sample_rate_hz=int(sample_rate_hz), onset_samples=onset, onset_seconds=onset / fs,
            status=status, window_ms=st.window_ms, window=st.window, window_samples=w, step_seconds=res.step / fs,
            thresholds=st.thresholds, mixing_time_seconds=mixing, eta_max=eta_max, tau_max_seconds=tau_max,
            profile=profile if keep_profile else None))
    return out


# ---------------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------------


def _results_of_batch(eng, batch, sample_rate_hz, names, settings) -> List[EchoDensityChannelResult]:
    return echo_density_results(echo_density_device(eng, batch, sample_rate_hz, settings), sample_rate_hz, names)


def analyse_echo_density_batch(
    channels: Sequence[np.ndarray],
    sample_rate_hz: int,
    channel_names: Sequence[str],
    settings: Optional[EchoDensitySettings] = None,
) -> List[EchoDensityChannelResult]:
    """Every channel through the device in batches of at most MAX_BATCH_CHANNELS channels."""
    return M.analyse_channel_batches(channels, sample_rate_hz, channel_names, settings or EchoDensitySettings(),
                                     _results_of_batch)


def analyse_echo_density_from_wav_file(
    input_wav_file_path: str | Path,
    settings: Optional[EchoDensitySettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[EchoDensityChannelResult]:
    """One WAV file (mono or stereo, rate checked against expected_sample_rate_hz); channels named as by
    get_analysis_channels ("mono", "left", "right")."""
    return M.analyse_wav_file_channels(input_wav_file_path, settings or EchoDensitySettings(), expected_sample_rate_hz,
                                       analyse_echo_density_batch)


def analyse_echo_density_files(
    paths: Sequence[str | Path],
    settings: Optional[EchoDensitySettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[EchoDensityChannelResult]:
    """Every channel of every file in one device batch per MAX_BATCH_CHANNELS channels; channels named
    "<file name>:<channel>"."""
    return M.analyse_file_channels(paths, settings or EchoDensitySettings(), expected_sample_rate_hz,
                                   analyse_echo_density_batch)


def analyse_echo_density_bundle(
    bundle_root: str | Path,
    settings: Optional[EchoDensitySettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[EchoDensityChannelResult]:
    """The taps a bundle's meta.json lists (taps/<name>.wav), read by the native ingest (ingest.TapSet) a group at a
    time; channels named "<tap>:<channel>"."""
    return M.analyse_bundle_channels(bundle_root, settings or EchoDensitySettings(), expected_sample_rate_hz,
                                     _results_of_batch)


# ---------------------------------------------------------------------------------------------------
# text, Markdown, JSON
# ---------------------------------------------------------------------------------------------------


def _rows(r: EchoDensityChannelResult) -> List[List[str]]:
    return [[f"{thr:g}", M.fmt(1000.0 * t, 2)] for thr, t in zip(r.thresholds, r.mixing_time_seconds)]


def _head(r: EchoDensityChannelResult, sep: str, end: str) -> str:
    return (f"Onset: {r.onset_samples} samples ({1000.0 * r.onset_seconds:.3f} ms){sep}Status: {status_text(r.status)}{sep}"
            f"Window: {r.window} {r.window_ms:g} ms ({r.window_samples} samples){sep}Step: {1000.0 * r.step_seconds:.3f} ms{end}")


def _tail(r: EchoDensityChannelResult, end: str) -> List[str]:
    return [f"eta_max: {M.fmt(r.eta_max, 3)} at {M.fmt(1000.0 * r.tau_max_seconds, 2)} ms{end}"]


def summarise_echo_density_text(channel_results: List[EchoDensityChannelResult]) -> str:
    """
    Fixed text format, one block per channel followed by an empty line:
        [<channel name>]
        Onset: <o> samples (<o / fs in ms, 3 decimals> ms)  Status: ok | <flags> (<words>)  Window: <kind> <ms> ms (<W> samples)  Step: <ms, 3 decimals> ms
        Threshold  mixing_time_ms
        <threshold>  <ms from the onset, 2 decimals>
        eta_max: <3 decimals> at <ms, 2 decimals> ms
    Cells are separated by two spaces; NaN (no crossing, or a channel with a status) is "NA".
    """
    return M.join_blocks(M.text_block(r.channel_name, _head(r, "  ", ""), ["mixing_time_ms"], _rows(r), tail=_tail(r, ""),
                                      first="Threshold") for r in channel_results)


def summarise_echo_density_markdown(channel_results: List[EchoDensityChannelResult]) -> str:
    """The same values as a Markdown section per channel: a '### <channel name>' heading, an onset / status / window line,
    a table with a row per threshold and the eta_max line."""
    return M.join_blocks(M.markdown_block(r.channel_name, _head(r, ". ", "."), ["mixing time (ms)"], _rows(r),
                                          tail=_tail(r, "."), first="Threshold") for r in channel_results)


def echo_density_results_to_json(channel_results: List[EchoDensityChannelResult], with_profile: bool = True) -> Dict:
    """Plain JSON: NaN is null.  The profile is written for the channels that kept one unless with_profile is False."""
    rows = []
    for r in channel_results:
        d = {"channel_name": r.channel_name, "sample_rate_hz": r.sample_rate_hz, "onset_samples": r.onset_samples,
             "onset_seconds": r.onset_seconds, "status": r.status, "window_ms": r.window_ms, "window": r.window,
             "window_samples": r.window_samples, "step_seconds": r.step_seconds, "thresholds": list(r.thresholds),
             "mixing_time_seconds": [M.json_num(v) for v in r.mixing_time_seconds], "eta_max": M.json_num(r.eta_max),
             "tau_max_seconds": M.json_num(r.tau_max_seconds)}
        if with_profile and r.profile is not None:
            d["profile"] = [M.json_num(float(v)) for v in r.profile]
        rows.append(d)
    return {"echo_density": rows}


def echo_density_results_from_json(doc: Dict) -> List[EchoDensityChannelResult]:
    return [EchoDensityChannelResult(
        channel_name=d["channel_name"], sample_rate_hz=int(d["sample_rate_hz"]), onset_samples=int(d["onset_samples"]),
        onset_seconds=float(d["onset_seconds"]), status=int(d["status"]), window_ms=float(d["window_ms"]),
        window=str(d["window"]), window_samples=int(d["window_samples"]), step_seconds=float(d["step_seconds"]),
        thresholds=tuple(float(v) for v in d["thresholds"]),
        mixing_time_seconds=tuple(M.num_json(v) for v in d["mixing_time_seconds"]), eta_max=M.num_json(d["eta_max"]),
        tau_max_seconds=M.num_json(d["tau_max_seconds"]),
        profile=np.asarray([M.num_json(v) for v in d["profile"]], dtype=np.float32) if "profile" in d else None)
        for d in doc["echo_density"]]


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.echodensity",
        description="Normalized echo density (Abel & Huang) per channel: the profile from the onset, its maximum and the "
                    "mixing time, the first time the profile reaches a threshold.")
    M.add_source_arguments(p)
    p.add_argument("--window-ms", type=float, default=20.0, help="length of the sliding window (default: 20 ms)")
    p.add_argument("--window", choices=WINDOWS, default="hann", help="window weights (default: hann)")
    p.add_argument("--step-ms", type=float, default=1.0,
                   help="distance of neighbouring positions (default: 1 ms; 0: one sample)")
    p.add_argument("--max-time-ms", type=float, default=None,
                   help="evaluate up to this time after the onset (default: the whole channel)")
    p.add_argument("--thresholds", nargs="+", type=float, default=[1.0],
                   help=f"1 to {MAX_THRESHOLDS} ascending levels whose first crossing is a mixing time (default: 1.0)")
    p.add_argument("--onset-db", type=float, default=-20.0,
                   help="onset: first sample within this level of the peak (default: -20 dB, ISO 3382-1)")
    p.add_argument("--no-profile", action="store_true", help="leave the profile out of the JSON")
    M.add_output_arguments(p)
    return p


def settings_from_args(args) -> EchoDensitySettings:
    return EchoDensitySettings(window_ms=args.window_ms, window=args.window, step_ms=args.step_ms,
                               max_time_ms=args.max_time_ms, thresholds=tuple(args.thresholds), onset_db=args.onset_db,
                               use_mono_downmix_for_stereo=bool(args.mono))


def main(argv: Optional[Sequence[str]] = None) -> None:
    parser = build_parser()
    no_profile = bool(parser.parse_args(argv).no_profile)
    M.run_cli(parser, argv, settings_from_args, analyse_echo_density_files, analyse_echo_density_bundle,
              summarise_echo_density_text, lambda results: echo_density_results_to_json(results, not no_profile))


if __name__ == "__main__":
    main()
