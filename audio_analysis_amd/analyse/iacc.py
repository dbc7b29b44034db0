"""
ISO 3382-1 Annex B inter-aural (here: inter-channel) cross-correlation coefficients per stereo pair and band: IACC_E
(early), IACC_L (late), IACC_A (whole response), each with the lag tau_IACC at which the maximum falls.

The reference reports nothing of the kind (its diffusion block has a short-time, float32, mean-removed series for a plot);
this module adds the parameter.  A stereo pair is two float32 channels l, r of equal length N at sample rate fs.  Every
product and sum is float64 on the exact float32 samples.

  onset    o = min(o_l, o_r), each the channel's ISO 3382-1 onset (ira_onset_index with rel_energy = 10**(onset_db / 10),
           default onset_db = -20 as in analyse.energy); the minimum is taken on the device.  Every band signal of the
           pair uses this broadband o.  L = N - o.
  lags     T = floor(max_lag_ms * fs / 1000) samples (default max_lag_ms = 1.0: T = 48 at 48 kHz); tau runs over -T .. +T
           inclusive.  1 <= T <= 128 (IRA_XCORR_MAX_LAG).
  limits   1 to 4 ascending early limits in ms, default (80.0,); N_k = energy.window_samples (ceil(limit_ms * fs / 1000)).
           Partitions P_0 = [0, N_1), ..., P_K = [N_K, L), counted from o.
  sums     per partition j = [a, b), 2T + 3 doubles (ira_xcorr_windows):
             C_j(tau) = sum_{n=a}^{b-1} l[o + n] * r[o + n + tau], r[m] = 0 for m < 0 or m >= N: the right channel is read
                        across partition boundaries and in front of the onset, never wrapped;
             El_j = sum l[o + n]**2, Er_j = sum r[o + n]**2, both over the same unshifted [a, b).
  host     (float64) for limit k: early = P_0 + ... + P_{k-1}, late = P_k + ... + P_K, all = every partition, always added in
           ascending order (as energy.parameters_from_sums does).  IACF(tau) = C(tau) / sqrt(El * Er);
           IACC = max_tau |IACF(tau)|; tau_samples = the first maximiser in the order -T .. +T (tau > 0: the right channel
           lags); tau_seconds = tau_samples / fs.  If El * Er is 0 or not finite, that cell's IACC and tau are NaN and no
           flag is set.
  IACC_E3  the mean of the early IACC at the first limit over the 500 Hz, 1000 Hz and 2000 Hz bands; reported only when the
           bank is the octave bank, otherwise NaN.
  bands    the rt60bands filter bank (rt60bands.band_signals_device): none, three, octave (default) or third.  Each
           channel of the pair is filtered separately, with the same zero-phase circular filter as everywhere else.

Per-pair status (bit flags; when any is set every output is NaN, the batch carries on):
  1 either channel silent, 2 too short (L <= N_K), 4 non-finite (broadband El, Er or any C of the whole response),
  8 not a stereo pair (a mono file or tap in a file list or bundle).

Command line (no plots): python -m analyse.iacc --input A.wav [B.wav ...] | --bundle DIR
  [--bands {none,three,octave,third}] [--onset-db -20] [--limits-ms 80] [--max-lag-ms 1.0] [--expected-sample-rate 48000]
  [--json OUT.json]
"""
from __future__ import annotations

import argparse
import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..engine import get_engine
from . import _measure as M
from ._common import band_row_offsets
from ._measure import BAND_MODES
from .energy import MAX_LIMITS, window_samples
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ
from .rt60bands import BandDefinition, Rt60BandsAnalysisSettings, _build_band_definitions, band_signals_device

STATUS_SILENT = 1
STATUS_TOO_SHORT = 2
STATUS_NON_FINITE = 4
STATUS_NOT_STEREO = 8
_STATUS_WORDS = ((STATUS_SILENT, "silent"), (STATUS_TOO_SHORT, "too short"), (STATUS_NON_FINITE, "non-finite"),
                 (STATUS_NOT_STEREO, "not stereo"))

MAX_LAG_SAMPLES = 128             # IRA_XCORR_MAX_LAG of include/ira.h
E3_BANDS = ("500Hz", "1000Hz", "2000Hz")


@dataclass(frozen=True)
class IaccSettings:
    onset_db: float = -20.0
    early_limits_ms: Tuple[float, ...] = (80.0,)
    max_lag_ms: float = 1.0
    bands: Optional[Rt60BandsAnalysisSettings] = field(default_factory=lambda: Rt60BandsAnalysisSettings(band_mode="octave"))

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
        try:
            lag = float(self.max_lag_ms)
        except (TypeError, ValueError):
            raise ValueError(f"max_lag_ms must be a positive, finite time in ms, got {self.max_lag_ms!r}") from None
        if not (math.isfinite(lag) and lag > 0.0):
            raise ValueError(f"max_lag_ms must be a positive, finite time in ms, got {self.max_lag_ms}")
        if self.bands is not None:
            if not isinstance(self.bands, Rt60BandsAnalysisSettings):
                raise ValueError("bands must be an Rt60BandsAnalysisSettings or None")
            if str(self.bands.band_mode).lower() not in BAND_MODES:
                raise ValueError(f"Unknown band_mode: {self.bands.band_mode} (expected one of {', '.join(BAND_MODES)})")
        object.__setattr__(self, "onset_db", onset)
        object.__setattr__(self, "early_limits_ms", limits)
        object.__setattr__(self, "max_lag_ms", lag)

    @property
    def rel_energy(self) -> float:
        return 10.0 ** (self.onset_db / 10.0)

    @property
    def is_octave_bank(self) -> bool:
        return self.bands is not None and str(self.bands.band_mode).lower() == "octave"


@dataclass(frozen=True)
class IaccValues:
    early: Tuple[float, ...]               # IACC_E, one per early limit
    late: Tuple[float, ...]                # IACC_L, one per early limit
    whole: float                           # IACC_A
    tau_early_seconds: Tuple[float, ...]   # tau_IACC of each of them (tau > 0: the right channel lags)
    tau_late_seconds: Tuple[float, ...]
    tau_whole_seconds: float


@dataclass(frozen=True)
class IaccPairResult:
    pair_name: str
    sample_rate_hz: int
    early_limits_ms: Tuple[float, ...]
    max_lag_samples: int
    onset_samples: int
    onset_seconds: float
    status: int
    broadband: IaccValues
    band_definitions: List[BandDefinition]
    band_values_by_name: Dict[str, IaccValues]
    iacc_e3: float


@dataclass
class IaccSums:
    """What iacc_device leaves on the host: per pair the onset, |x[peak]| of both channels and the partition sums of the
    broadband signals (row 0) and of every band (1 ..), each partition C(-T .. +T), El, Er."""
    bands: List[BandDefinition]
    length: np.ndarray                     # int64 (npairs,)
    onset: np.ndarray                      # int64 (npairs,) min of the two channels' onsets
    peak_abs: np.ndarray                   # float32 (npairs, 2)
    sums: np.ndarray                       # float64 (npairs, 1 + nbands, K + 1, 2T + 3)
    limits: np.ndarray                     # int64 (K,) window limits in samples
    max_lag: int                           # T


def max_lag_samples(max_lag_ms: float, sample_rate_hz: float) -> int:
    """T = floor(max_lag_ms * fs / 1000) samples, float64 in exactly that order (48 at 48 kHz for 1 ms)."""
    return int(math.floor(float(max_lag_ms) * float(sample_rate_hz) / 1000.0))


def status_text(status: int) -> str:
    return M.status_text(status, _STATUS_WORDS)


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def iacc_device(eng, batch, pairs: Sequence[Tuple[int, int]], sample_rate_hz: int, settings: Optional[IaccSettings] = None,
                band_signals=None) -> IaccSums:
    """
    Onsets and partitioned lag sums of every (left, right) pair of channel indices of a device batch, broadband and per
    band, in ONE ira_xcorr_windows launch.  band_signals = (bands, y device, y_off (nch, nbands)) as
    band_signals_device returns them lets a caller that already built the band signals skip the filter bank;
    otherwise settings.bands decides which are built (None: broadband only).
    """
    settings = settings or IaccSettings()
    nch = batch.count
    pr = np.asarray(list(pairs), dtype=np.int64).reshape(-1, 2)
    npairs = int(pr.shape[0])
    if npairs and (pr.min() < 0 or pr.max() >= nch):
        raise ValueError("pairs must hold channel indices of the batch")
    left, right = pr[:, 0], pr[:, 1]
    n64 = batch.length.astype(np.int64)
    if np.any(n64[left] != n64[right]):
        raise ValueError("the two channels of a stereo pair must have the same length")
    tmax = max_lag_samples(settings.max_lag_ms, sample_rate_hz)
    if not 1 <= tmax <= MAX_LAG_SAMPLES:
        raise ValueError(f"max_lag_ms = {settings.max_lag_ms:g} is {tmax} samples at {sample_rate_hz} Hz; "
                         f"1 to {MAX_LAG_SAMPLES} samples are supported")
    limits = np.asarray(window_samples(settings.early_limits_ms, sample_rate_hz), dtype=np.int64)
    nlim = int(limits.size)
    onset_dev, _, peak_abs_dev = eng.onset_index(batch, settings.rel_energy)
    if band_signals is None and settings.bands is not None:
        band_signals = band_signals_device(eng, batch, sample_rate_hz, settings.bands)
    bands = band_signals[0] if band_signals is not None else []
    nb = len(bands)
    # segment rows: pair p's broadband signals, then its bands (row p * (1 + nb) + b)
    base, l_off = band_row_offsets(batch, band_signals, channels=left)
    _, r_off = band_row_offsets(batch, band_signals, channels=right)
    if npairs:
        out = eng.xcorr_windows(base, l_off, r_off, np.repeat(n64[left], 1 + nb), np.repeat(left.astype(np.int32), 1 + nb),
                                np.repeat(right.astype(np.int32), 1 + nb), onset_dev, np.tile(limits, (l_off.size, 1)), tmax)
        sums = out.cpu().numpy().reshape(npairs, 1 + nb, nlim + 1, 2 * tmax + 3)
    else:
        sums = np.zeros((0, 1 + nb, nlim + 1, 2 * tmax + 3))
    onset = onset_dev.cpu().numpy()
    peak_abs = peak_abs_dev.cpu().numpy()
    return IaccSums(bands=list(bands), length=n64[left].copy(), onset=np.minimum(onset[left], onset[right]).astype(np.int64),
                    peak_abs=np.stack([peak_abs[left], peak_abs[right]], axis=1), sums=sums, limits=limits, max_lag=tmax)


# ---------------------------------------------------------------------------------------------------
# host: sums -> coefficients
# ---------------------------------------------------------------------------------------------------


def _coefficient(s: np.ndarray):
    """(IACC (...), tau in samples (...), float64, NaN where undefined) of summed records (..., 2T + 3)."""
    tmax = (s.shape[-1] - 3) // 2
    c, el, er = s[..., : 2 * tmax + 1], s[..., 2 * tmax + 1], s[..., 2 * tmax + 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        prod = el * er
        ok = np.isfinite(prod) & (prod != 0.0)
        iacf = np.abs(c / np.sqrt(np.where(ok, prod, 1.0))[..., None])
    first = np.argmax(iacf, axis=-1)                      # the first maximiser in the order -T .. +T
    iacc = np.take_along_axis(iacf, first[..., None], axis=-1)[..., 0]
    return np.where(ok, iacc, np.nan), np.where(ok, (first - tmax).astype(np.float64), np.nan)


def iacc_from_sums(sums: np.ndarray):
    """
    Partition sums (..., K + 1, 2T + 3) = per partition C(-T .. +T), El, Er, float64 -> a dict of float64 arrays:
    "early", "late" (..., K) and "whole" (...): IACC_E / IACC_L per limit and IACC_A; "tau_early", "tau_late", "tau_whole":
    the lag of each maximum in SAMPLES (NaN where El * Er is 0 or not finite, like the coefficient).  Early sums add
    P_0, P_1, ... in ascending order; late sums add P_k .. P_K ascending; the whole response adds every partition ascending.
    """
    s = np.asarray(sums, dtype=np.float64)
    k = s.shape[-2] - 1
    parts = [s[..., i, :] for i in range(k + 1)]
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
    ce = [_coefficient(v) for v in early]
    cl = [_coefficient(v) for v in late]
    whole, tau_whole = _coefficient(total)
    return {"early": np.stack([v for v, _ in ce], axis=-1), "late": np.stack([v for v, _ in cl], axis=-1), "whole": whole,
            "tau_early": np.stack([t for _, t in ce], axis=-1), "tau_late": np.stack([t for _, t in cl], axis=-1),
            "tau_whole": tau_whole}


def iacc_e3(early_first_limit_by_band: Dict[str, float], octave_bank: bool) -> float:
    """IACC_E3: the mean of the early coefficient (first limit) over the 500 Hz, 1000 Hz and 2000 Hz octave bands; NaN for
    any other bank."""
    if not octave_bank or any(n not in early_first_limit_by_band for n in E3_BANDS):
        return float("nan")
    return float(sum(float(early_first_limit_by_band[n]) for n in E3_BANDS) / 3.0)


def _nan_values(nlim: int) -> IaccValues:
    nan = float("nan")
    return IaccValues((nan,) * nlim, (nan,) * nlim, nan, (nan,) * nlim, (nan,) * nlim, nan)


def not_stereo_result(name: str, sample_rate_hz: int, settings: IaccSettings) -> IaccPairResult:
    """The result of a file or tap that is not a stereo pair: status 8, every value NaN, the bank's rows kept."""
    bands = _build_band_definitions(settings.bands, sample_rate_hz) if settings.bands is not None else []
    nlim = len(settings.early_limits_ms)
    return IaccPairResult(
        pair_name=str(name), sample_rate_hz=int(sample_rate_hz), early_limits_ms=tuple(settings.early_limits_ms),
        max_lag_samples=max_lag_samples(settings.max_lag_ms, sample_rate_hz), onset_samples=0, onset_seconds=0.0,
        status=STATUS_NOT_STEREO, broadband=_nan_values(nlim), band_definitions=list(bands),
        band_values_by_name={b.name: _nan_values(nlim) for b in bands}, iacc_e3=float("nan"))


def iacc_results(res: IaccSums, sample_rate_hz: int, pair_names: Sequence[str], settings: IaccSettings) -> List[IaccPairResult]:
    fs = float(sample_rate_hz)
    nlim = int(res.limits.size)
    v = iacc_from_sums(res.sums) if res.sums.shape[0] else None
    out = []
    for p, name in enumerate(pair_names):
        onset = int(res.onset[p])
        whole = res.sums[p, 0].copy()
        total = whole[0].copy()
        for part in whole[1:]:
            total = total + part
        status = 0
        if float(res.peak_abs[p, 0]) == 0.0 or float(res.peak_abs[p, 1]) == 0.0:
            status |= STATUS_SILENT
        if int(res.length[p]) - onset <= int(res.limits[-1]):
            status |= STATUS_TOO_SHORT
        if not np.all(np.isfinite(total)):
            status |= STATUS_NON_FINITE

        def values(row):
            if status:
                return _nan_values(nlim)
            return IaccValues(tuple(float(x) for x in v["early"][p, row]), tuple(float(x) for x in v["late"][p, row]),
                              float(v["whole"][p, row]), tuple(float(x) / fs for x in v["tau_early"][p, row]),
                              tuple(float(x) / fs for x in v["tau_late"][p, row]), float(v["tau_whole"][p, row]) / fs)

        by_name = {b.name: values(1 + i) for i, b in enumerate(res.bands)}
        out.append(IaccPairResult(
            pair_name=str(name), sample_rate_hz=int(sample_rate_hz), early_limits_ms=tuple(settings.early_limits_ms),
            max_lag_samples=int(res.max_lag), onset_samples=onset, onset_seconds=onset / fs, status=status,
            broadband=values(0), band_definitions=list(res.bands), band_values_by_name=by_name,
            iacc_e3=iacc_e3({n: x.early[0] for n, x in by_name.items()}, settings.is_octave_bank)))
    return out


# ---------------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------------


def _results_of_pairs(eng, batch, pairs, sample_rate_hz, names, settings) -> List[IaccPairResult]:
    res = iacc_device(eng, batch, pairs, sample_rate_hz, settings)
    return iacc_results(res, sample_rate_hz, names, settings)


def _results_of_batch(eng, batch, sample_rate_hz, names, settings) -> List[IaccPairResult]:
    """A batch of interleaved pairs (channels 2 i and 2 i + 1), every channel named by its pair."""
    pairs = [(2 * i, 2 * i + 1) for i in range(batch.count // 2)]
    return _results_of_pairs(eng, batch, pairs, sample_rate_hz, names[::2], settings)


def analyse_iacc_pairs_batch(lefts: Sequence[np.ndarray], rights: Sequence[np.ndarray], sample_rate_hz: int,
                             names: Sequence[str], settings: Optional[IaccSettings] = None) -> List[IaccPairResult]:
    """Every (left, right) pair through the device in batches of at most MAX_BATCH_CHANNELS channels."""
    if not len(lefts) == len(rights) == len(names):
        raise ValueError("one right channel and one name per left channel")
    # left, right, left, ...: MAX_BATCH_CHANNELS is even, so a batch never splits a pair
    chans = [c for pair in zip(lefts, rights) for c in pair]
    return M.analyse_channel_batches(chans, sample_rate_hz, [n for n in names for _ in range(2)], settings or IaccSettings(),
                                     _results_of_batch)


def _merge(names: Sequence[str], stereo: Sequence[bool], pair_results: List[IaccPairResult], sample_rate_hz: int,
           settings: IaccSettings) -> List[IaccPairResult]:
    """Results in the order of the files: the analysed pairs, and a status-8 result for everything that is not a pair."""
    it = iter(pair_results)
    return [next(it) if s else not_stereo_result(n, sample_rate_hz, settings) for n, s in zip(names, stereo)]


def analyse_iacc_from_wav_file(input_wav_file_path: str | Path, settings: Optional[IaccSettings] = None,
                               expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> List[IaccPairResult]:
    """One WAV file (rate checked against expected_sample_rate_hz), named by its file name: one result, status 8 if the
    file is mono."""
    return analyse_iacc_files([input_wav_file_path], settings, expected_sample_rate_hz)


def analyse_iacc_files(paths: Sequence[str | Path], settings: Optional[IaccSettings] = None,
                       expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> List[IaccPairResult]:
    """One result per file, named by the file's name; stereo files share device batches of at most MAX_BATCH_CHANNELS
    channels, a mono file gets status 8."""
    settings = settings or IaccSettings()
    names, stereo, lefts, rights = [], [], [], []
    for p in paths:
        cs = [c for _, c in M.file_channels([p], False, expected_sample_rate_hz)]
        names.append(Path(p).name)
        stereo.append(len(cs) == 2)
        if len(cs) == 2:
            lefts.append(cs[0])
            rights.append(cs[1])
    fs = int(expected_sample_rate_hz)
    res = analyse_iacc_pairs_batch(lefts, rights, fs, [n for n, s in zip(names, stereo) if s], settings)
    return _merge(names, stereo, res, fs, settings)


def analyse_iacc_bundle(bundle_root: str | Path, settings: Optional[IaccSettings] = None,
                        expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> List[IaccPairResult]:
    """The taps a bundle's meta.json lists (taps/<name>.wav), read by the native ingest (ingest.TapSet) a group at a time
    (at most MAX_BATCH_CHANNELS channels per group); one result per tap, named by the tap; a mono tap gets status 8."""
    settings = settings or IaccSettings()
    fs = int(expected_sample_rate_hz)
    out: List[IaccPairResult] = []
    for group, batch, labels in M.bundle_groups(bundle_root, False, expected_sample_rate_hz):
        where: Dict[int, Dict[str, int]] = {}
        for k, (i, ch) in enumerate(labels):
            where.setdefault(i, {})[ch] = k
        stereo = [("left" in where.get(i, {}) and "right" in where.get(i, {})) for i in range(len(group))]
        pairs = [(where[i]["left"], where[i]["right"]) for i in range(len(group)) if stereo[i]]
        names = [g for g, s in zip(group, stereo) if s]
        res = _results_of_pairs(get_engine(), batch, pairs, fs, names, settings) if pairs else []
        out += _merge(group, stereo, res, fs, settings)
    return out


# ---------------------------------------------------------------------------------------------------
# text, Markdown, JSON
# ---------------------------------------------------------------------------------------------------


def _columns(r: IaccPairResult, markdown: bool = False) -> List[str]:
    unit = " (ms)" if markdown else "_ms"
    cols: List[str] = []
    for which in ("E", "L"):
        for v in r.early_limits_ms:
            cols += [f"IACC_{which}{v:g}", f"tau_{which}{v:g}{unit}"]
    return cols + ["IACC_A", f"tau_A{unit}"]


def _cells(v: IaccValues) -> List[str]:
    cells: List[str] = []
    for coeff, tau in ((v.early, v.tau_early_seconds), (v.late, v.tau_late_seconds)):
        for c, t in zip(coeff, tau):
            cells += [M.fmt(c), M.fmt(1000.0 * t)]
    return cells + [M.fmt(v.whole), M.fmt(1000.0 * v.tau_whole_seconds)]


def _rows(r: IaccPairResult) -> List[List[str]]:
    return [[name] + _cells(v) for name, v in M.band_rows(r, r.band_values_by_name)]


def summarise_iacc_text(pair_results: List[IaccPairResult]) -> str:
    """
    Fixed text format, one block per pair followed by an empty line:
        [<pair name>]
        Onset: <o> samples (<o / fs in ms, 3 decimals> ms)  Max lag: <T> samples  Status: ok | <flags> (<words>)
        Band  IACC_E80  tau_E80_ms  IACC_L80  tau_L80_ms  IACC_A  tau_A_ms
        Broadband  <IACC, 3 decimals>  <tau in ms, 3 decimals>  ...
        <band name>  ...                       (one row per band, ascending)
        IACC_E3: <3 decimals>
    The early columns of every limit come first, then the late ones, then the whole response.  Cells are separated by two
    spaces; NaN is "NA".
    """
    return M.join_blocks(M.text_block(
        r.pair_name, f"Onset: {r.onset_samples} samples ({1000.0 * r.onset_seconds:.3f} ms)  "
                     f"Max lag: {r.max_lag_samples} samples  Status: {status_text(r.status)}",
        _columns(r), _rows(r), tail=[f"IACC_E3: {M.fmt(r.iacc_e3)}"]) for r in pair_results)


def summarise_iacc_markdown(pair_results: List[IaccPairResult]) -> str:
    """The same values as a Markdown section per pair: a '### <pair name>' heading, an onset / lag / status line, a table
    with two columns per coefficient (IACC, tau in ms), rows Broadband then the bands, and an IACC_E3 line."""
    return M.join_blocks(M.markdown_block(
        r.pair_name, f"Onset: {r.onset_samples} samples ({1000.0 * r.onset_seconds:.3f} ms). "
                     f"Max lag: {r.max_lag_samples} samples. Status: {status_text(r.status)}.",
        _columns(r, markdown=True), _rows(r), tail=[f"IACC_E3: {M.fmt(r.iacc_e3)}"]) for r in pair_results)


def _values_json(v: IaccValues) -> Dict:
    return {"early": [M.json_num(x) for x in v.early], "late": [M.json_num(x) for x in v.late], "whole": M.json_num(v.whole),
            "tau_early_seconds": [M.json_num(x) for x in v.tau_early_seconds],
            "tau_late_seconds": [M.json_num(x) for x in v.tau_late_seconds],
            "tau_whole_seconds": M.json_num(v.tau_whole_seconds)}


def _values_from_json(d: Dict) -> IaccValues:
    return IaccValues(tuple(M.num_json(x) for x in d["early"]), tuple(M.num_json(x) for x in d["late"]), M.num_json(d["whole"]),
                      tuple(M.num_json(x) for x in d["tau_early_seconds"]), tuple(M.num_json(x) for x in d["tau_late_seconds"]),
                      M.num_json(d["tau_whole_seconds"]))


def iacc_results_to_json(pair_results: List[IaccPairResult]) -> Dict:
    """Plain JSON: NaN is null."""
    rows = []
    for r in pair_results:
        rows.append({
            "pair_name": r.pair_name, "sample_rate_hz": r.sample_rate_hz, "early_limits_ms": list(r.early_limits_ms),
            "max_lag_samples": r.max_lag_samples, "onset_samples": r.onset_samples, "onset_seconds": r.onset_seconds,
            "status": r.status, "iacc_e3": M.json_num(r.iacc_e3), "broadband": _values_json(r.broadband),
            "bands": [M.band_to_json(b, _values_json(r.band_values_by_name[b.name])) for b in r.band_definitions],
        })
    return {"iacc": rows}


def iacc_results_from_json(doc: Dict) -> List[IaccPairResult]:
    out = []
    for d in doc["iacc"]:
        out.append(IaccPairResult(
            pair_name=d["pair_name"], sample_rate_hz=int(d["sample_rate_hz"]),
            early_limits_ms=tuple(float(v) for v in d["early_limits_ms"]), max_lag_samples=int(d["max_lag_samples"]),
            onset_samples=int(d["onset_samples"]), onset_seconds=float(d["onset_seconds"]), status=int(d["status"]),
            broadband=_values_from_json(d["broadband"]), band_definitions=M.bands_from_json(d["bands"]),
            band_values_by_name={b["name"]: _values_from_json(b) for b in d["bands"]}, iacc_e3=M.num_json(d["iacc_e3"])))
    return out


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.iacc",
        description="ISO 3382-1 inter-channel cross-correlation coefficients (IACC early, late, whole) per stereo pair "
                    "and band.")
    M.add_source_arguments(p, "stereo WAV files (one pair per file)", mono=False)
    M.add_bands_argument(p)
    p.add_argument("--onset-db", type=float, default=-20.0,
                   help="onset: first sample within this level of the peak (default: -20 dB, ISO 3382-1)")
    p.add_argument("--limits-ms", nargs="+", type=float, default=[80.0],
                   help="early/late limits in ms, 1 to 4, ascending (default: 80)")
    p.add_argument("--max-lag-ms", type=float, default=1.0, help="largest lag |tau| in ms (default: 1.0, ISO 3382-1)")
    M.add_output_arguments(p)
    return p


def settings_from_args(args) -> IaccSettings:
    bands = None if args.bands == "none" else Rt60BandsAnalysisSettings(band_mode=args.bands)
    return IaccSettings(onset_db=args.onset_db, early_limits_ms=tuple(args.limits_ms), max_lag_ms=args.max_lag_ms,
                        bands=bands)


def _checked_settings_from_args(args) -> IaccSettings:
    """settings_from_args, and the lag limit checked at the expected sample rate: a usage error, not a failure later on."""
    settings = settings_from_args(args)
    tmax = max_lag_samples(settings.max_lag_ms, args.expected_sample_rate)
    if not 1 <= tmax <= MAX_LAG_SAMPLES:
        raise ValueError(f"--max-lag-ms {settings.max_lag_ms:g} is {tmax} samples at {args.expected_sample_rate} Hz; "
                         f"1 to {MAX_LAG_SAMPLES} samples are supported")
    return settings


def main(argv: Optional[Sequence[str]] = None) -> None:
    M.run_cli(build_parser(), argv, _checked_settings_from_args, analyse_iacc_files, analyse_iacc_bundle, summarise_iacc_text,
              iacc_results_to_json)


if __name__ == "__main__":
    main()
