"""
ISO 3382-1 energy-ratio parameters per channel and band: clarity C_k, definition D and centre time Ts.

The reference reports decay times only; this module adds the numbers an impulse-response analyser reports beside them.
For a float32 channel x (after the usual channel policy) at sample rate fs, with e[n] = float64(x[n])**2:

  peak     p = argmax |x|, the first maximum (ira_peak_index).
  onset    o = the smallest n <= p with e[n] >= e[p] * 10**(onset_db / 10) (ISO 3382-1 A.3.4: the first point within
           20 dB of the maximum for the default onset_db = -20); the factor is formed on the host in float64, the compare
           is float64 (ira_onset_index, on the device: the peak never returns to the host in between).
  windows  every early limit (1 to 4 of them, ascending, in ms) becomes N_k = math.ceil(limit_ms * fs / 1000.0) samples.
  sums     over s = e[o:], L = len(x) - o samples: P_0 = sum s[0:N_1], ..., P_K = sum s[N_K:L] and S1 = sum n s[n], all
           float64 (ira_energy_windows).  Late energy is its own partition sum, never total - early, so that C stays accurate
           when the tail is 60 dB down.
  C_k      10 log10((P_0 + ... + P_{k-1}) / (P_k + ... + P_K)) dB; +inf when the late sum is 0 and the early sum is not.
  D        early(50 ms) / total when 50 ms is one of the limits, else early(first limit) / total, named by that limit.
  Ts       S1 / (fs * total) seconds.

Bands are the rt60bands filter bank (Rt60BandsAnalysisSettings: three / octave / third bands) made by the same engine calls
as rt60_bands_device: circular irfft(rfft(x) * mask) over the FULL file.  The masks are real, so the band filters are
zero-phase and every band signal uses its channel's broadband onset o and the same N_k.  Pre-ringing of a band filter that
wraps around to the end of the file counts as late energy, exactly as it shapes the band decay in rt60bands.

Per-channel status (bit flags; a channel with a non-zero status has NaN in every output, the batch carries on):
  1 silent (e[p] == 0), 2 too short (L <= N_K), 4 non-finite (total or S1 of the broadband channel not finite).

Command line (no plots): python -m analyse.energy --input A.wav [B.wav ...] | --bundle DIR [--mono]
  [--bands {none,three,octave,third}] [--onset-db -20] [--limits-ms 50 80] [--expected-sample-rate 48000] [--json OUT.json]
"""
from __future__ import annotations

import argparse
import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _measure as M
from ._common import band_row_offsets
from ._measure import BAND_MODES, MAX_BATCH_CHANNELS  # noqa: F401  (both are part of this module's surface)
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ
from .rt60bands import BandDefinition, Rt60BandsAnalysisSettings, band_signals_device

STATUS_SILENT = 1
STATUS_TOO_SHORT = 2
STATUS_NON_FINITE = 4
_STATUS_WORDS = ((STATUS_SILENT, "silent"), (STATUS_TOO_SHORT, "too short"), (STATUS_NON_FINITE, "non-finite"))

MAX_LIMITS = 4


@dataclass(frozen=True)
class EnergyParameterSettings:
    onset_db: float = -20.0
    early_limits_ms: Tuple[float, ...] = (50.0, 80.0)
    bands: Optional[Rt60BandsAnalysisSettings] = field(default_factory=lambda: Rt60BandsAnalysisSettings(band_mode="octave"))
    use_mono_downmix_for_stereo: bool = False

    def __post_init__(self):
        onset = float(self.onset_db)
        if not math.isfinite(onset) or onset > 0.0:
            raise ValueError(f"onset_db must be a finite level <= 0 dB relative to the peak, got {self.onset_db}")
        try:
            limits = tuple(float(v) for v in self.early_limits_ms)
        except TypeError:
            raise ValueError("early_limits_ms must be a sequence of 1 to 4 limits in ms") from None
        if not 1 <= len(limits) <= MAX_LIMITS:
            raise ValueError(f"early_limits_ms needs 1 to {MAX_LIMITS} limits, got {len(limits)}")
        if not all(math.isfinite(v) and v > 0.0 for v in limits):
            raise ValueError(f"early_limits_ms must be positive and finite, got {limits}")
        if any(b <= a for a, b in zip(limits, limits[1:])):
            raise ValueError(f"early_limits_ms must be strictly ascending, got {limits}")
        if self.bands is not None:
            if not isinstance(self.bands, Rt60BandsAnalysisSettings):
                raise ValueError("bands must be an Rt60BandsAnalysisSettings or None")
            if str(self.bands.band_mode).lower() not in BAND_MODES:
                raise ValueError(f"Unknown band_mode: {self.bands.band_mode} (expected one of {', '.join(BAND_MODES)})")
        object.__setattr__(self, "onset_db", onset)
        object.__setattr__(self, "early_limits_ms", limits)

    @property
    def rel_energy(self) -> float:
        return 10.0 ** (self.onset_db / 10.0)

    @property
    def definition_limit_ms(self) -> float:
        return 50.0 if 50.0 in self.early_limits_ms else self.early_limits_ms[0]


@dataclass(frozen=True)
class EnergyParameters:
    clarity_db: Tuple[float, ...]          # C_k, one per early limit
    definition: float                      # D at definition_limit_ms
    centre_time_seconds: float             # Ts


@dataclass(frozen=True)
class EnergyParametersChannelResult:
    channel_name: str
    sample_rate_hz: int
    early_limits_ms: Tuple[float, ...]
    definition_limit_ms: float
    onset_samples: int
    onset_seconds: float
    status: int
    broadband: EnergyParameters
    band_definitions: List[BandDefinition]
    band_parameters_by_name: Dict[str, EnergyParameters]


@dataclass
class EnergySums:
    """What energy_parameters_device leaves on the host: per channel the onset, |x[peak]| and the window sums of the
    broadband signal (band 0) and of every band (1 ..), each row P_0 .. P_K, S1."""
    bands: List[BandDefinition]
    length: np.ndarray                     # int64 (nch,) channel lengths
    onset: np.ndarray                      # int64 (nch,)
    peak_abs: np.ndarray                   # float32 (nch,)
    sums: np.ndarray                       # float64 (nch, 1 + nbands, K + 2)
    limits: np.ndarray                     # int64 (K,) window limits in samples


def window_samples(early_limits_ms: Sequence[float], sample_rate_hz: float) -> List[int]:
    """N_k = ceil(limit_ms * fs / 1000) samples, float64 in exactly that order (2400 / 3840 at 48 kHz for 50 / 80 ms)."""
    return [int(math.ceil(float(v) * float(sample_rate_hz) / 1000.0)) for v in early_limits_ms]


def status_text(status: int) -> str:
    return M.status_text(status, _STATUS_WORDS)


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def energy_parameters_device(eng, batch, sample_rate_hz: int, settings: Optional[EnergyParameterSettings] = None,
                             band_signals=None) -> EnergySums:
    """
    Onset and window sums of every channel of a device batch, broadband and per band, in ONE ira_energy_windows launch.
    band_signals = (bands, y device, y_off (nch, nbands)) as band_signals_device returns them lets a caller that already
    built the band signals skip the filter bank; otherwise settings.bands decides which are built (None: broadband only).
    """
    settings = settings or EnergyParameterSettings()
    nch = batch.count
    limits = np.asarray(window_samples(settings.early_limits_ms, sample_rate_hz), dtype=np.int64)
    nlim = int(limits.size)
    onset_dev, _, peak_abs_dev = eng.onset_index(batch, settings.rel_energy)
    if band_signals is None and settings.bands is not None:
        band_signals = band_signals_device(eng, batch, sample_rate_hz, settings.bands)
    bands = band_signals[0] if band_signals is not None else []
    nb = len(bands)
    # segment rows: channel c's broadband signal, then its bands (row c * (1 + nb) + b)
    base, seg_off = band_row_offsets(batch, band_signals)
    seg_len = np.repeat(batch.length.astype(np.int64), 1 + nb)
    chan = np.repeat(np.arange(nch, dtype=np.int32), 1 + nb)
    if nch:
        out = eng.energy_windows(base, seg_off, seg_len, chan, onset_dev, np.tile(limits, (seg_off.size, 1)))
        sums = out.cpu().numpy().reshape(nch, 1 + nb, nlim + 2)
    else:
        sums = np.zeros((0, 1 + nb, nlim + 2))
    return EnergySums(bands=list(bands), length=batch.length.astype(np.int64).copy(), onset=onset_dev.cpu().numpy().copy(), peak_abs=peak_abs_dev.cpu().numpy().copy(),
                      sums=sums, limits=limits)


# ---------------------------------------------------------------------------------------------------
# host: sums -> parameters
# ---------------------------------------------------------------------------------------------------


def parameters_from_sums(sums: np.ndarray, sample_rate_hz: float, d_index: int):
    """(C (..., K) dB, D (...), Ts (...) s) from window sums (..., K + 2) = P_0 .. P_K, S1, float64.  d_index: the limit
    (0-based) D is taken at.  Early sums add P_0, P_1, ... in ascending order; late sums add P_k .. P_K ascending."""
    s = np.asarray(sums, dtype=np.float64)
    k = s.shape[-1] - 2
    parts = [s[..., i] for i in range(k + 1)]
    total = parts[0].copy()
    for p in parts[1:]:
        total = total + p
    early, late = [], []
    acc = np.zeros_like(total)
    for i in range(1, k + 1):
        acc = acc + parts[i - 1]
        early.append(acc)
        tail = parts[i].copy()
        for p in parts[i + 1:]:
            tail = tail + p
        late.append(tail)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.stack([10.0 * np.log10(e / l) for e, l in zip(early, late)], axis=-1)
        d = early[d_index] / total
        ts = s[..., k + 1] / (float(sample_rate_hz) * total)
    return c, d, ts


def energy_parameters_results(res: EnergySums, sample_rate_hz: int, channel_names: Sequence[str],
                              settings: EnergyParameterSettings) -> List[EnergyParametersChannelResult]:
    limits_ms = settings.early_limits_ms
    d_ms = settings.definition_limit_ms
    d_index = limits_ms.index(d_ms)
    c, d, ts = parameters_from_sums(res.sums, sample_rate_hz, d_index)
    out = []
    for ch, name in enumerate(channel_names):
        onset = int(res.onset[ch])
        total = float(np.sum(res.sums[ch, 0, :-1]))
        s1 = float(res.sums[ch, 0, -1])
        status = 0
        if float(res.peak_abs[ch]) == 0.0:
            status |= STATUS_SILENT
        if int(res.length[ch]) - onset <= int(res.limits[-1]):
            status |= STATUS_TOO_SHORT
        if not (math.isfinite(total) and math.isfinite(s1)):
            status |= STATUS_NON_FINITE

        def params(row):
            if status:
                return EnergyParameters(tuple(float("nan") for _ in limits_ms), float("nan"), float("nan"))
            return EnergyParameters(tuple(float(v) for v in c[ch, row]), float(d[ch, row]), float(ts[ch, row]))

        out.append(EnergyParametersChannelResult(
            channel_name=str(name), sample_rate_hz=int(sample_rate_hz), early_limits_ms=tuple(limits_ms),
            definition_limit_ms=float(d_ms), onset_samples=onset, onset_seconds=onset / float(sample_rate_hz),
            status=status, broadband=params(0), band_definitions=list(res.bands),
            band_parameters_by_name={b.name: params(1 + i) for i, b in enumerate(res.bands)}))
    return out


# ---------------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------------


def _results_of_batch(eng, batch, sample_rate_hz, names, settings) -> List[EnergyParametersChannelResult]:
    res = energy_parameters_device(eng, batch, sample_rate_hz, settings)
    return energy_parameters_results(res, sample_rate_hz, names, settings)


def analyse_energy_parameters_batch(
    channels: Sequence[np.ndarray],
    sample_rate_hz: int,
    channel_names: Sequence[str],
    settings: Optional[EnergyParameterSettings] = None,
) -> List[EnergyParametersChannelResult]:
    """Every channel through the device in batches of at most MAX_BATCH_CHANNELS channels."""
    return M.analyse_channel_batches(channels, sample_rate_hz, channel_names, settings or EnergyParameterSettings(),
                                     _results_of_batch)


def analyse_energy_parameters_from_wav_file(
    input_wav_file_path: str | Path,
    settings: Optional[EnergyParameterSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[EnergyParametersChannelResult]:
    """One WAV file (mono or stereo, rate checked against expected_sample_rate_hz); channels named as by
    get_analysis_channels ("mono", "left", "right")."""
    return M.analyse_wav_file_channels(input_wav_file_path, settings or EnergyParameterSettings(), expected_sample_rate_hz,
                                       analyse_energy_parameters_batch)


def analyse_energy_parameters_files(
    paths: Sequence[str | Path],
    settings: Optional[EnergyParameterSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[EnergyParametersChannelResult]:
    """Every channel of every file in one device batch per MAX_BATCH_CHANNELS channels; channels named
    "<file name>:<channel>"."""
    return M.analyse_file_channels(paths, settings or EnergyParameterSettings(), expected_sample_rate_hz,
                                   analyse_energy_parameters_batch)


def analyse_energy_parameters_bundle(
    bundle_root: str | Path,
    settings: Optional[EnergyParameterSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[EnergyParametersChannelResult]:
    """The taps a bundle's meta.json lists (taps/<name>.wav), read by the native ingest (ingest.TapSet) a group at a
    time (at most MAX_BATCH_CHANNELS channels per group); channels named "<tap>:<channel>"."""
    return M.analyse_bundle_channels(bundle_root, settings or EnergyParameterSettings(), expected_sample_rate_hz,
                                     _results_of_batch)


# ---------------------------------------------------------------------------------------------------
# text, Markdown, JSON
# ---------------------------------------------------------------------------------------------------


def _columns(r: EnergyParametersChannelResult) -> List[str]:
    return [f"C{v:g}_dB" for v in r.early_limits_ms] + [f"D{r.definition_limit_ms:g}", "Ts_ms"]


def _cells(p: EnergyParameters) -> List[str]:
    return [M.fmt(v, 2) for v in p.clarity_db] + [M.fmt(p.definition, 3), M.fmt(1000.0 * p.centre_time_seconds, 2)]


def _rows(r: EnergyParametersChannelResult) -> List[List[str]]:
    return [[name] + _cells(p) for name, p in M.band_rows(r, r.band_parameters_by_name)]


def summarise_energy_parameters_text(channel_results: List[EnergyParametersChannelResult]) -> str:
    """
    Fixed text format, one block per channel followed by an empty line:
        [<channel name>]
        Onset: <o> samples (<o / fs in ms, 3 decimals> ms)  Status: ok | <flags> (<words>)
        Band  C50_dB  C80_dB  D50  Ts_ms
        Broadband  <C, 2 decimals>  ...  <D, 3 decimals>  <Ts in ms, 2 decimals>
        <band name>  ...                       (one row per band, ascending)
    Cells are separated by two spaces; NaN is "NA", an infinite clarity "+inf" / "-inf".
    """
    return M.join_blocks(M.text_block(
        r.channel_name, f"Onset: {r.onset_samples} samples ({1000.0 * r.onset_seconds:.3f} ms)  Status: {status_text(r.status)}",
        _columns(r), _rows(r)) for r in channel_results)


def summarise_energy_parameters_markdown(channel_results: List[EnergyParametersChannelResult]) -> str:
    """The same values as a Markdown section per channel: a '### <channel name>' heading, an onset / status line and a
    table with a column per parameter (C in dB, D, Ts in ms), rows Broadband then the bands."""
    return M.join_blocks(M.markdown_block(
        r.channel_name, f"Onset: {r.onset_samples} samples ({1000.0 * r.onset_seconds:.3f} ms). Status: {status_text(r.status)}.",
        [f"C{v:g} (dB)" for v in r.early_limits_ms] + [f"D{r.definition_limit_ms:g}", "Ts (ms)"], _rows(r))
        for r in channel_results)


def _params_json(p: EnergyParameters) -> Dict:
    return {"clarity_db": [M.json_num(v) for v in p.clarity_db], "definition": M.json_num(p.definition),
            "centre_time_seconds": M.json_num(p.centre_time_seconds)}


def _params_from_json(d: Dict) -> EnergyParameters:
    return EnergyParameters(tuple(M.num_json(v) for v in d["clarity_db"]), M.num_json(d["definition"]),
                            M.num_json(d["centre_time_seconds"]))


def energy_results_to_json(channel_results: List[EnergyParametersChannelResult]) -> Dict:
    """Plain JSON: NaN is null, an infinite clarity the string "+inf" / "-inf"."""
    rows = []
    for r in channel_results:
        rows.append({
            "channel_name": r.channel_name, "sample_rate_hz": r.sample_rate_hz, "early_limits_ms": list(r.early_limits_ms),
            "definition_limit_ms": r.definition_limit_ms, "onset_samples": r.onset_samples,
            "onset_seconds": r.onset_seconds, "status": r.status, "broadband": _params_json(r.broadband),
            "bands": [M.band_to_json(b, _params_json(r.band_parameters_by_name[b.name])) for b in r.band_definitions],
        })
    return {"energy_parameters": rows}


def energy_results_from_json(doc: Dict) -> List[EnergyParametersChannelResult]:
    out = []
    for d in doc["energy_parameters"]:
        out.append(EnergyParametersChannelResult(
            channel_name=d["channel_name"], sample_rate_hz=int(d["sample_rate_hz"]),
            early_limits_ms=tuple(float(v) for v in d["early_limits_ms"]),
            definition_limit_ms=float(d["definition_limit_ms"]), onset_samples=int(d["onset_samples"]),
            onset_seconds=float(d["onset_seconds"]), status=int(d["status"]), broadband=_params_from_json(d["broadband"]),
            band_definitions=M.bands_from_json(d["bands"]),
            band_parameters_by_name={b["name"]: _params_from_json(b) for b in d["bands"]}))
    return out


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.energy",
        description="ISO 3382-1 clarity (C), definition (D) and centre time (Ts) per channel and band.")
    M.add_source_arguments(p)
    M.add_bands_argument(p)
    p.add_argument("--onset-db", type=float, default=-20.0,
                   help="onset: first sample within this level of the peak (default: -20 dB, ISO 3382-1)")
    p.add_argument("--limits-ms", nargs="+", type=float, default=[50.0, 80.0],
                   help="early/late limits in ms, 1 to 4, ascending (default: 50 80)")
    M.add_output_arguments(p)
    return p


def settings_from_args(args) -> EnergyParameterSettings:
    bands = None if args.bands == "none" else Rt60BandsAnalysisSettings(band_mode=args.bands)
    return EnergyParameterSettings(onset_db=args.onset_db, early_limits_ms=tuple(args.limits_ms), bands=bands,
                                   use_mono_downmix_for_stereo=bool(args.mono))


def main(argv: Optional[Sequence[str]] = None) -> None:
    M.run_cli(build_parser(), argv, settings_from_args, analyse_energy_parameters_files, analyse_energy_parameters_bundle,
              summarise_energy_parameters_text, energy_results_to_json)


if __name__ == "__main__":
    main()
