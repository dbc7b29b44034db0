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
import json
import math
import sys
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..engine import get_engine
from ._common import wav_channels
from .frequency_response import rfft_bin_step
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ
from .rt60bands import BandDefinition, Rt60BandsAnalysisSettings, _build_band_definitions, band_mask_record

STATUS_SILENT = 1
STATUS_TOO_SHORT = 2
STATUS_NON_FINITE = 4
_STATUS_WORDS = ((STATUS_SILENT, "silent"), (STATUS_TOO_SHORT, "too short"), (STATUS_NON_FINITE, "non-finite"))

MAX_LIMITS = 4
MAX_BATCH_CHANNELS = 256          # channels per device batch (the CLI's chunk)
BAND_MODES = ("three", "octave", "third")


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
    if status == 0:
        return "ok"
    return f"{status} (" + ", ".join(w for bit, w in _STATUS_WORDS if status & bit) + ")"


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def band_signals_device(eng, batch, sample_rate_hz: int, band_settings: Rt60BandsAnalysisSettings):
    """The rt60bands filter bank for a device batch, by the engine calls of rt60_bands_device: one forward float64 rFFT of
    every full file, masked inverse transforms per band.  Returns (bands, y float32 device, y_off (nch, nbands) int64):
    band b of channel c is batch.length[c] samples at y_off[c, b]."""
    t = eng.torch
    nch = batch.count
    n64 = batch.length.astype(np.int64)
    if np.any(n64 < 8):
        raise ValueError("Not enough samples for band analysis.")
    bands = _build_band_definitions(band_settings, sample_rate_hz)
    nb = len(bands)
    if nb == 0:
        return bands, None, np.zeros((nch, 0), dtype=np.int64)
    nyq = 0.5 * float(sample_rate_hz)
    records = np.stack([band_mask_record(b, band_settings.transition_width_octaves, nyq) for b in bands])
    spec, spec_off = eng.rfft_any(batch.x, batch.off, n64, use_hann=False)
    per_entry = np.repeat(n64, nb)
    y_off = (np.cumsum(per_entry) - per_entry).reshape(nch, nb)
    y = eng.empty(int(per_entry.sum()), t.float32)
    fv_of = {int(v): rfft_bin_step(int(v), sample_rate_hz) for v in np.unique(n64)}
    fv = np.array([fv_of[int(v)] for v in n64], dtype=np.float64)
    eng.band_irfft(spec, np.repeat(np.asarray(spec_off, dtype=np.int64), nb), per_entry.astype(np.int32),
                   np.tile(records, (nch, 1)), np.repeat(fv, nb), y, y_off.reshape(-1))
    return bands, y, y_off


def _common_base(tensors):
    """One base pointer for float32 device buffers that one launch reads: the lowest of them, and every buffer's offset
    from it in elements (the kernels address segments as base + offset in the device's flat address space)."""
    ptrs = [int(x.data_ptr()) for x in tensors]
    lo = int(np.argmin(ptrs))
    if any((p - ptrs[lo]) % 4 for p in ptrs):
        raise ValueError("float32 buffers of one launch must be 4-byte aligned to each other")
    return tensors[lo], [(p - ptrs[lo]) // 4 for p in ptrs]


def energy_parameters_device(eng, batch, sample_rate_hz: int, settings: Optional[EnergyParameterSettings] = None,
                             band_signals=None) -> EnergySums:
    """
    Onset and window sums of every channel of a device batch, broadband and per band, in ONE ira_energy_windows launch.
    band_signals = (bands, y device, y_off (nch, nbands)) as band_signals_device returns them lets a caller that already
    built the band signals skip the filter bank; otherwise settings.bands decides which are built (None: broadband only).
    """
    settings = settings or EnergyParameterSettings()
    t = eng.torch
    nch = batch.count
    limits = np.asarray(window_samples(settings.early_limits_ms, sample_rate_hz), dtype=np.int64)
    nlim = int(limits.size)
    onset_dev, _, peak_abs_dev = eng.onset_index(batch, settings.rel_energy)
    if band_signals is None and settings.bands is not None:
        band_signals = band_signals_device(eng, batch, sample_rate_hz, settings.bands)
    bands, y, y_off = band_signals if band_signals is not None else ([], None, np.zeros((nch, 0), dtype=np.int64))
    nb = len(bands)
    y_off = np.asarray(y_off, dtype=np.int64).reshape(nch, nb)
    # segment rows: channel c's broadband signal, then its bands (row c * (1 + nb) + b)
    if nb:
        base, (dx, dy) = _common_base([batch.x, y])
        seg_off = np.concatenate([(batch.off + dx)[:, None], y_off + dy], axis=1).reshape(-1)
    else:
        base, seg_off = batch.x, batch.off.copy()
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


def analyse_energy_parameters_batch(
    channels: Sequence[np.ndarray],
    sample_rate_hz: int,
    channel_names: Sequence[str],
    settings: Optional[EnergyParameterSettings] = None,
) -> List[EnergyParametersChannelResult]:
    """Every channel through the device in batches of at most MAX_BATCH_CHANNELS channels."""
    settings = settings or EnergyParameterSettings()
    if len(channels) != len(channel_names):
        raise ValueError("one name per channel")
    eng = get_engine()
    out: List[EnergyParametersChannelResult] = []
    for a in range(0, len(channels), MAX_BATCH_CHANNELS):
        chans = [np.asarray(c, dtype=np.float32).reshape(-1) for c in channels[a : a + MAX_BATCH_CHANNELS]]
        batch = eng.upload(chans)
        out += _results_of_batch(eng, batch, sample_rate_hz, channel_names[a : a + MAX_BATCH_CHANNELS], settings)
    return out


def _results_of_batch(eng, batch, sample_rate_hz, names, settings) -> List[EnergyParametersChannelResult]:
    res = energy_parameters_device(eng, batch, sample_rate_hz, settings)
    return energy_parameters_results(res, sample_rate_hz, names, settings)


def analyse_energy_parameters_from_wav_file(
    input_wav_file_path: str | Path,
    settings: Optional[EnergyParameterSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[EnergyParametersChannelResult]:
    """One WAV file (mono or stereo, rate checked against expected_sample_rate_hz); channels named as by
    get_analysis_channels ("mono", "left", "right")."""
    settings = settings or EnergyParameterSettings()
    loaded, chans = wav_channels(input_wav_file_path, settings.use_mono_downmix_for_stereo,
                                 expected_sample_rate_hz=expected_sample_rate_hz)
    return analyse_energy_parameters_batch([c for _, c in chans], loaded.sample_rate_hz, [n for n, _ in chans], settings)


def analyse_energy_parameters_files(
    paths: Sequence[str | Path],
    settings: Optional[EnergyParameterSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[EnergyParametersChannelResult]:
    """Every channel of every file in one device batch per MAX_BATCH_CHANNELS channels; channels named
    "<file name>:<channel>"."""
    settings = settings or EnergyParameterSettings()
    chans, names = [], []
    for p in paths:
        _, cs = wav_channels(p, settings.use_mono_downmix_for_stereo, expected_sample_rate_hz=expected_sample_rate_hz)
        for n, c in cs:
            chans.append(c)
            names.append(f"{Path(p).name}:{n}")
    return analyse_energy_parameters_batch(chans, int(expected_sample_rate_hz), names, settings)


def analyse_energy_parameters_bundle(
    bundle_root: str | Path,
    settings: Optional[EnergyParameterSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[EnergyParametersChannelResult]:
    """The taps a bundle's meta.json lists (taps/<name>.wav), read by the native ingest (ingest.TapSet) a group at a
    time (at most MAX_BATCH_CHANNELS channels per group); channels named "<tap>:<channel>"."""
    from ..ingest import TapSet

    settings = settings or EnergyParameterSettings()
    root = Path(bundle_root)
    taps: List[str] = list(json.loads((root / "meta.json").read_text()).get("taps", []))
    eng = get_engine()
    out: List[EnergyParametersChannelResult] = []
    step = MAX_BATCH_CHANNELS // 2                        # a tap has one or two channels
    for a in range(0, len(taps), step):
        group = taps[a : a + step]
        ts = TapSet(eng, [root / "taps" / f"{t}.wav" for t in group], expected_sample_rate_hz)
        batch, labels = ts.view(settings.use_mono_downmix_for_stereo)
        names = [f"{group[i]}:{ch}" for i, ch in labels]
        out += _results_of_batch(eng, batch, int(expected_sample_rate_hz), names, settings)
    return out


# ---------------------------------------------------------------------------------------------------
# text, Markdown, JSON
# ---------------------------------------------------------------------------------------------------


def _fmt(v: float, digits: int) -> str:
    if math.isnan(v):
        return "NA"
    if math.isinf(v):
        return "+inf" if v > 0 else "-inf"
    return f"{v:.{digits}f}"


def _columns(r: EnergyParametersChannelResult) -> List[str]:
    return [f"C{v:g}_dB" for v in r.early_limits_ms] + [f"D{r.definition_limit_ms:g}", "Ts_ms"]


def _cells(p: EnergyParameters) -> List[str]:
    return [_fmt(v, 2) for v in p.clarity_db] + [_fmt(p.definition, 3), _fmt(1000.0 * p.centre_time_seconds, 2)]


def _rows(r: EnergyParametersChannelResult) -> List[Tuple[str, EnergyParameters]]:
    return [("Broadband", r.broadband)] + [(b.name, r.band_parameters_by_name[b.name]) for b in r.band_definitions]


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
    lines: List[str] = []
    for r in channel_results:
        lines.append(f"[{r.channel_name}]")
        lines.append(f"Onset: {r.onset_samples} samples ({1000.0 * r.onset_seconds:.3f} ms)  Status: {status_text(r.status)}")
        lines.append("  ".join(["Band"] + _columns(r)))
        for name, p in _rows(r):
            lines.append("  ".join([name] + _cells(p)))
        lines.append("")
    return "\n".join(lines) + ("\n" if lines else "")


def summarise_energy_parameters_markdown(channel_results: List[EnergyParametersChannelResult]) -> str:
    """The same values as a Markdown section per channel: a '### <channel name>' heading, an onset / status line and a
    table with a column per parameter (C in dB, D, Ts in ms), rows Broadband then the bands."""
    lines: List[str] = []
    for r in channel_results:
        cols = [f"C{v:g} (dB)" for v in r.early_limits_ms] + [f"D{r.definition_limit_ms:g}", "Ts (ms)"]
        lines.append(f"### {r.channel_name}")
        lines.append("")
        lines.append(f"Onset: {r.onset_samples} samples ({1000.0 * r.onset_seconds:.3f} ms). Status: {status_text(r.status)}.")
        lines.append("")
        lines.append("| Band | " + " | ".join(cols) + " |")
        lines.append("|---|" + "---:|" * len(cols))
        for name, p in _rows(r):
            lines.append("| " + " | ".join([name] + _cells(p)) + " |")
        lines.append("")
    return "\n".join(lines) + ("\n" if lines else "")


def _json_num(v: float):
    if math.isnan(v):
        return None
    if math.isinf(v):
        return "+inf" if v > 0 else "-inf"
    return float(v)


def _num_json(v) -> float:
    return float("nan") if v is None else float(v)          # float("+inf") parses the infinite clarity


def _params_json(p: EnergyParameters) -> Dict:
    return {"clarity_db": [_json_num(v) for v in p.clarity_db], "definition": _json_num(p.definition),
            "centre_time_seconds": _json_num(p.centre_time_seconds)}


def _params_from_json(d: Dict) -> EnergyParameters:
    return EnergyParameters(tuple(_num_json(v) for v in d["clarity_db"]), _num_json(d["definition"]),
                            _num_json(d["centre_time_seconds"]))


def energy_results_to_json(channel_results: List[EnergyParametersChannelResult]) -> Dict:
    """Plain JSON: NaN is null, an infinite clarity the string "+inf" / "-inf"."""
    rows = []
    for r in channel_results:
        rows.append({
            "channel_name": r.channel_name, "sample_rate_hz": r.sample_rate_hz, "early_limits_ms": list(r.early_limits_ms),
            "definition_limit_ms": r.definition_limit_ms, "onset_samples": r.onset_samples,
            "onset_seconds": r.onset_seconds, "status": r.status, "broadband": _params_json(r.broadband),
            "bands": [dict(name=b.name, centre_hz=b.centre_hz, kind=b.kind, low_edge_hz=b.low_edge_hz,
                           high_edge_hz=b.high_edge_hz, **_params_json(r.band_parameters_by_name[b.name]))
                      for b in r.band_definitions],
        })
    return {"energy_parameters": rows}


def energy_results_from_json(doc: Dict) -> List[EnergyParametersChannelResult]:
    out = []
    for d in doc["energy_parameters"]:
        bands = [BandDefinition(b["name"], b["centre_hz"], b["kind"], b["low_edge_hz"], b["high_edge_hz"])
                 for b in d["bands"]]
        out.append(EnergyParametersChannelResult(
            channel_name=d["channel_name"], sample_rate_hz=int(d["sample_rate_hz"]),
            early_limits_ms=tuple(float(v) for v in d["early_limits_ms"]),
            definition_limit_ms=float(d["definition_limit_ms"]), onset_samples=int(d["onset_samples"]),
            onset_seconds=float(d["onset_seconds"]), status=int(d["status"]), broadband=_params_from_json(d["broadband"]),
            band_definitions=bands, band_parameters_by_name={b["name"]: _params_from_json(b) for b in d["bands"]}))
    return out


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.energy",
        description="ISO 3382-1 clarity (C), definition (D) and centre time (Ts) per channel and band.")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--input", nargs="+", type=Path, help="WAV files (every channel of every file is analysed)")
    src.add_argument("--bundle", type=Path, help="bundle directory: meta.json + taps/<name>.wav")
    p.add_argument("--mono", action="store_true", help="analyse stereo files as their mono downmix 0.5 * (L + R)")
    p.add_argument("--bands", choices=["none", *BAND_MODES], default="octave", help="filter bank (default: octave)")
    p.add_argument("--onset-db", type=float, default=-20.0,
                   help="onset: first sample within this level of the peak (default: -20 dB, ISO 3382-1)")
    p.add_argument("--limits-ms", nargs="+", type=float, default=[50.0, 80.0],
                   help="early/late limits in ms, 1 to 4, ascending (default: 50 80)")
    p.add_argument("--expected-sample-rate", type=int, default=DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
                   help="every file must have this sample rate (default: 48000)")
    p.add_argument("--json", type=Path, default=None, help="also write the results as JSON to this file")
    return p


def settings_from_args(args) -> EnergyParameterSettings:
    bands = None if args.bands == "none" else Rt60BandsAnalysisSettings(band_mode=args.bands)
    return EnergyParameterSettings(onset_db=args.onset_db, early_limits_ms=tuple(args.limits_ms), bands=bands,
                                   use_mono_downmix_for_stereo=bool(args.mono))


def main(argv: Optional[Sequence[str]] = None) -> None:
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        settings = settings_from_args(args)
    except ValueError as e:
        parser.error(str(e))
    if args.input:
        results = analyse_energy_parameters_files(args.input, settings, args.expected_sample_rate)
    else:
        results = analyse_energy_parameters_bundle(args.bundle, settings, args.expected_sample_rate)
    sys.stdout.write(summarise_energy_parameters_text(results))
    sys.stdout.flush()
    if args.json is not None:
        args.json.write_text(json.dumps(energy_results_to_json(results), indent=2) + "\n")


if __name__ == "__main__":
    main()
