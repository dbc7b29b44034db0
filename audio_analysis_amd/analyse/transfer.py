"""
Dual-channel transfer function and coherence (Welch's method, H1 and H2 estimators) between a reference channel and a
measurement channel.

The reference obtains a response only from the recording of a sweep (deconvolve.py, harmonics.py), and its one spectral
division says nothing about how far the result can be trusted at a frequency.  Dual-channel FFT analysis measures a system
from whatever was played -- noise, music, programme material: the auto- and cross-spectra of the two channels are averaged
over overlapping frames, and the magnitude-squared coherence tells, per frequency, how much of the measurement is
linearly explained by the reference (Welch 1967; Bendat & Piersol).

A pair is (reference row x, measurement row y), float32 rows of one device buffer of Lx and Ly samples, with an integer
delay d in samples, positive when the measurement lags, which may be negative:

  x'[n] = x[n + max(0, -d)]      y'[n] = y[n + max(0, d)]      N = min(Lx - max(0, -d), Ly - max(0, d))

n_fft a power of two 256 .. 8192; hop = max(1, n_fft - floor(overlap * n_fft + 0.5)), overlap in [0, 1); w the engine's
float64 window table of n_fft points (numpy.hanning for "hann", ones for "rect").

  K = 1 + floor((N - n_fft) / hop) frames when N >= n_fft, else 0; frame f starts at f * hop; no padding, no detrending.
  For bins k = 0 .. n_fft / 2, X_f = FFT(w x'_f), Y_f = FFT(w y'_f) in float64:
    Sxx[k] = sum_f |X_f[k]|^2      Syy[k] = sum_f |Y_f[k]|^2      Sxy[k] = sum_f conj(X_f[k]) Y_f[k]
  H1 = Sxy / Sxx     H2 = Syy / conj(Sxy) = Syy Sxy / |Sxy|^2     coherence = min(1, |Sxy|^2 / (Sxx Syy))
  mag_db = 20 log10 |H1| (formed as 10 log10 |H1|^2)     phase = atan2(Im Sxy, Re Sxy) radians
  A quotient whose denominator is 0 is NaN, not an infinity.

All of it is formed on the device (ira_xspec_accumulate, ira_xspec_finish: one launch each per batch).  The host adds, from
the device's sums in float64: the mean coherence over band_hz and the share of that band's bins at or above
coherence_threshold (bins k >= 1 with band_hz[0] <= k fs / n_fft <= band_hz[1]), and rows on a fractional-octave grid:
centres 1000 * 2^(i / points_per_octave) inside band_hz, edges a half step either side, a row's bins those with
low <= k fs / n_fft < high, H = sum Sxy / sum Sxx, coherence = |sum Sxy|^2 / (sum Sxx * sum Syy) over them (NaN for a
row without bins).

delay = "auto" (find_delay_device): the measurement deconvolved with the reference (deconvolve_device, no DC removal, no
peak normalisation, the full transform), the index i of the greatest |h| (Engine.segment_peaks); i >= n/2 of that n-point
circular response is the negative delay i - n.  It inherits that module's limit of 2^21 points.

Per-pair status (bit flags; a pair with a status has NaN in every value, the batch carries on): 1 silent reference (Sxx
is 0 in every bin although there are frames), 2 too short (K < 1), 4 non-finite (any sum is not finite).

Command line (no plots):
  python -m analyse.transfer --measured A.wav [B.wav ...] --reference S.wav [--mono]
                           | --input ST.wav [...] --reference-channel left|right
    [--n-fft 4096] [--overlap 0.5] [--window hann|rect] [--delay auto|SAMPLES] [--points-per-octave 3]
    [--coherence-threshold 0.5] [--expected-sample-rate 48000] [--json OUT.json]
With --measured / --reference the reference file is mixed down to mono (as --sweep of analyse.harmonics) and every
channel of every measured file is a pair; with --input / --reference-channel the other channel of each stereo file is the
measurement.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from ..engine import get_engine, xspec_frames
from . import _measure as M
from ._measure import MAX_BATCH_CHANNELS  # noqa: F401  (part of this module's surface)
from .deconvolve import DeconvolveSettings, _downmix_to_mono_1d, deconvolve_device
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ, load_wav_file

STATUS_SILENT_REFERENCE = 1
STATUS_TOO_SHORT = 2
STATUS_NON_FINITE = 4
_STATUS_WORDS = ((STATUS_SILENT_REFERENCE, "silent reference"), (STATUS_TOO_SHORT, "too short"),
                 (STATUS_NON_FINITE, "non-finite"))

MIN_FFT, MAX_FFT = 256, 8192
WINDOWS = ("hann", "rect")
# rows of the device's output, in order (IRA_XSPEC_ROWS)
ARRAYS = ("sxx", "syy", "sxy_re", "sxy_im", "h1_re", "h1_im", "h2_re", "h2_im", "coherence", "mag_db", "phase_rad")


@dataclass(frozen=True)
class TransferSettings:
    n_fft: int = 4096
    overlap: float = 0.5
    window: str = "hann"
    delay: Union[int, str] = "auto"                 # samples the measurement lags the reference by, or "auto"
    band_hz: Tuple[float, float] = (20.0, 20000.0)  # the summary's band
    coherence_threshold: float = 0.5
    points_per_octave: int = 3
    use_mono_downmix_for_stereo: bool = False

    def __post_init__(self):
        n = self.n_fft
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < MIN_FFT or n > MAX_FFT or n & (n - 1):
            raise ValueError(f"n_fft must be a power of two from {MIN_FFT} to {MAX_FFT}, got {self.n_fft}")
        try:
            ov = float(self.overlap)
        except (TypeError, ValueError):
            raise ValueError(f"overlap must be a number in [0, 1), got {self.overlap}") from None
        if not 0.0 <= ov < 1.0:                     # NaN fails
            raise ValueError(f"overlap must lie in [0, 1), got {self.overlap}")
        if self.window not in WINDOWS:
            raise ValueError(f"window must be one of {WINDOWS}, got {self.window!r}")
        d = self.delay
        if isinstance(d, str):
            if d != "auto":
                raise ValueError(f"delay must be an integer number of samples or 'auto', got {d!r}")
        elif isinstance(d, bool) or not isinstance(d, (int, np.integer)):
            raise ValueError(f"delay must be an integer number of samples or 'auto', got {d!r}")
        else:
            d = int(d)
        try:
            lo, hi = (float(v) for v in self.band_hz)
        except (TypeError, ValueError):
            raise ValueError("band_hz must be (low edge, high edge) in Hz") from None
        if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 <= lo < hi):
            raise ValueError(f"band_hz must be 0 <= low edge < high edge, got {self.band_hz}")
        thr = float(self.coherence_threshold)
        if not 0.0 <= thr <= 1.0:
            raise ValueError(f"coherence_threshold must lie in [0, 1], got {self.coherence_threshold}")
        ppo = self.points_per_octave
        if isinstance(ppo, bool) or not isinstance(ppo, (int, np.integer)) or not 1 <= ppo <= 48:
            raise ValueError(f"points_per_octave must be an integer from 1 to 48, got {self.points_per_octave}")
        for k, v in (("n_fft", int(n)), ("overlap", ov), ("delay", d), ("band_hz", (lo, hi)),
                     ("coherence_threshold", thr), ("points_per_octave", int(ppo)),
                     ("use_mono_downmix_for_stereo", bool(self.use_mono_downmix_for_stereo))):
            object.__setattr__(self, k, v)

    @property
    def hop(self) -> int:
        return max(1, self.n_fft - int(math.floor(self.overlap * self.n_fft + 0.5)))

    @property
    def use_hann(self) -> bool:
        return self.window == "hann"


@dataclass(frozen=True)
class TransferBandRow:
    centre_hz: float
    low_edge_hz: float
    high_edge_hz: float
    bins: int
    mag_db: float
    phase_rad: float
    coherence: float


@dataclass(frozen=True)
class TransferPairResult:
    pair_name: str
    sample_rate_hz: int
    n_fft: int
    hop: int
    window: str
    delay_samples: int
    samples: int                                    # N
    frames: int                                     # K
    status: int
    band_hz: Tuple[float, float]
    coherence_threshold: float
    mean_coherence: float
    coherent_fraction: float
    rows: Tuple[TransferBandRow, ...]
    arrays: Dict[str, np.ndarray]                   # ARRAYS -> float64 (n_fft / 2 + 1,)

    @property
    def frequency_hz(self) -> np.ndarray:
        return np.arange(self.n_fft // 2 + 1, dtype=np.float64) * (float(self.sample_rate_hz) / self.n_fft)


@dataclass
class TransferSums:
    """What transfer_device leaves on the host: per pair the delay, N, K and the device's eleven rows."""
    n_fft: int
    hop: int
    window: str
    delay: np.ndarray                               # int64 (npairs,)
    samples: np.ndarray                             # int64 (npairs,)
    frames: np.ndarray                              # int64 (npairs,)
    out: np.ndarray                                 # float64 (npairs, 11, n_fft / 2 + 1)


def status_text(status: int) -> str:
    return M.status_text(status, _STATUS_WORDS)


def pair_geometry(lx, ly, delay):
    """(x skip, y skip, N) of a pair (elementwise int64): x' starts max(0, -d) into x, y' max(0, d) into y, N the
    samples both still have (never below 0)."""
    lx, ly, d = (np.asarray(v, dtype=np.int64) for v in (lx, ly, delay))
    xs, ys = np.maximum(0, -d), np.maximum(0, d)
    return xs, ys, np.maximum(0, np.minimum(lx - xs, ly - ys))


def frame_count(n, n_fft: int, hop: int):
    """K = 1 + floor((N - n_fft) / hop) when N >= n_fft, else 0."""
    return xspec_frames(n, n_fft, hop)


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def find_delay_device(eng, batch, x_rows: Sequence[int], y_rows: Sequence[int], sample_rate_hz: int) -> np.ndarray:
    """The delay of every pair (int64 samples, positive: the measurement lags): the measurement deconvolved with the
    reference over the full transform, no DC removal, no peak normalisation; the index of the greatest magnitude of that
    circular response, indices in its upper half counting as negative.  ValueError beyond 2^21 points, as that module."""
    x_rows = np.asarray(x_rows, dtype=np.int64).reshape(-1)
    y_rows = np.asarray(y_rows, dtype=np.int64).reshape(-1)
    if x_rows.size == 0:
        return np.zeros(0, dtype=np.int64)
    refs, ref_of_pair = np.unique(x_rows, return_inverse=True)
    st = DeconvolveSettings(normalise_peak=False, remove_dc=False, output_length_mode="full_fft")
    dev = deconvolve_device(eng, eng.subset(batch, y_rows), list(range(y_rows.size)), eng.subset(batch, refs),
                            ref_of_pair.reshape(-1), sample_rate_hz, st)
    n = dev["n_fft"].astype(np.int64)
    _, idx = eng.segment_peaks(dev["h"], dev["off"], n, with_index=True)
    return np.where(idx >= n // 2, idx - n, idx).astype(np.int64)


def transfer_device(eng, batch, x_rows: Sequence[int], y_rows: Sequence[int], sample_rate_hz: int,
                    settings: Optional[TransferSettings] = None, delays: Optional[Sequence[int]] = None) -> TransferSums:
    """The sums and derived values of every pair (x_rows[p], y_rows[p]) of rows of a device batch: one
    ira_xspec_accumulate and one ira_xspec_finish launch.  delays: per pair, instead of settings.delay."""
    settings = settings or TransferSettings()
    x_rows = np.asarray(x_rows, dtype=np.int64).reshape(-1)
    y_rows = np.asarray(y_rows, dtype=np.int64).reshape(-1)
    if x_rows.size != y_rows.size:
        raise ValueError("one reference row per measurement row")
    npairs = int(x_rows.size)
    if npairs and (min(x_rows.min(), y_rows.min()) < 0 or max(x_rows.max(), y_rows.max()) >= batch.count):
        raise ValueError("x_rows and y_rows must index the batch")
    if delays is not None:
        d = np.asarray(delays, dtype=np.int64).reshape(-1)
        if d.size != npairs:
            raise ValueError("one delay per pair")
    elif settings.delay == "auto":
        d = find_delay_device(eng, batch, x_rows, y_rows, sample_rate_hz)
    else:
        d = np.full(npairs, int(settings.delay), dtype=np.int64)
    length = batch.length.astype(np.int64)
    xs, ys, n = pair_geometry(length[x_rows], length[y_rows], d)
    n_fft, hop = settings.n_fft, settings.hop
    nbins = n_fft // 2 + 1
    if npairs:
        out = eng.cross_spectra(batch.x, batch.off[x_rows] + xs, batch.off[y_rows] + ys, n, n_fft, hop,
                                settings.use_hann).cpu().numpy().reshape(npairs, len(ARRAYS), nbins)
    else:
        out = np.zeros((0, len(ARRAYS), nbins))
    return TransferSums(n_fft=n_fft, hop=hop, window=settings.window, delay=d, samples=n,
                        frames=frame_count(n, n_fft, hop), out=out)


# ---------------------------------------------------------------------------------------------------
# host: sums -> results
# ---------------------------------------------------------------------------------------------------


def octave_grid(band_hz: Tuple[float, float], points_per_octave: int) -> List[Tuple[float, float, float]]:
    """(centre, low edge, high edge) of the rows: centres 1000 * 2^(i / points_per_octave) inside band_hz."""
    lo, hi = band_hz
    ppo = int(points_per_octave)
    if hi <= 0.0:
        return []
    i0 = int(math.ceil(ppo * math.log2(max(lo, 1e-6) / 1000.0) - 1e-9))
    i1 = int(math.floor(ppo * math.log2(hi / 1000.0) + 1e-9))
    half = 2.0 ** (0.5 / ppo)
    return [(c, c / half, c * half) for c in (1000.0 * 2.0 ** (i / ppo) for i in range(i0, i1 + 1))]


def pair_status(frames: int, sums: np.ndarray) -> int:
    """sums: the four rows Sxx, Syy, Re Sxy, Im Sxy."""
    status = 0
    if frames < 1:
        status |= STATUS_TOO_SHORT
    elif not np.any(sums[0] != 0.0):
        status |= STATUS_SILENT_REFERENCE
    if not np.all(np.isfinite(sums)):
        status |= STATUS_NON_FINITE
    return status


def transfer_results(res: TransferSums, sample_rate_hz: int, pair_names: Sequence[str],
                     settings: Optional[TransferSettings] = None) -> List[TransferPairResult]:
    settings = settings or TransferSettings()
    fs = float(sample_rate_hz)
    nbins = res.n_fft // 2 + 1
    freq = np.arange(nbins, dtype=np.float64) * (fs / res.n_fft)
    lo, hi = settings.band_hz
    in_band = (freq >= lo) & (freq <= hi) & (np.arange(nbins) >= 1)
    grid = octave_grid(settings.band_hz, settings.points_per_octave)
    nan = float("nan")
    out = []
    for p, name in enumerate(pair_names):
        rows11 = res.out[p]
        status = pair_status(int(res.frames[p]), rows11[:4])
        if status:
            arrays = {k: np.full(nbins, nan) for k in ARRAYS}
            mean_coh = frac = nan
            rows = tuple(TransferBandRow(c, a, b, int(np.count_nonzero((freq >= a) & (freq < b) & (np.arange(nbins) >= 1))),
                                         nan, nan, nan) for c, a, b in grid)
        else:
            arrays = {k: rows11[i].astype(np.float64).copy() for i, k in enumerate(ARRAYS)}
            coh = arrays["coherence"][in_band]
            mean_coh = float(np.mean(coh)) if coh.size else nan
            frac = float(np.count_nonzero(coh >= settings.coherence_threshold)) / coh.size if coh.size else nan
            rows = []
            for c, a, b in grid:
                sel = (freq >= a) & (freq < b) & (np.arange(nbins) >= 1)
                cnt = int(np.count_nonzero(sel))
                sxx, syy = float(np.sum(arrays["sxx"][sel])), float(np.sum(arrays["syy"][sel]))
                sxy = complex(float(np.sum(arrays["sxy_re"][sel])), float(np.sum(arrays["sxy_im"][sel])))
                if cnt == 0 or sxx == 0.0:
                    rows.append(TransferBandRow(c, a, b, cnt, nan, nan, nan))
                    continue
                mag = abs(sxy) / sxx
                rows.append(TransferBandRow(
                    c, a, b, cnt, 20.0 * math.log10(mag) if mag > 0.0 else -math.inf, math.atan2(sxy.imag, sxy.real),
                    min(1.0, abs(sxy) ** 2 / (sxx * syy)) if syy > 0.0 else nan))
            rows = tuple(rows)
        out.append(TransferPairResult(
            pair_name=str(name), sample_rate_hz=int(sample_rate_hz), n_fft=res.n_fft, hop=res.hop, window=res.window,
            delay_samples=int(res.delay[p]), samples=int(res.samples[p]), frames=int(res.frames[p]), status=status,
            band_hz=settings.band_hz, coherence_threshold=settings.coherence_threshold, mean_coherence=mean_coh,
            coherent_fraction=frac, rows=rows, arrays=arrays))
    return out


# ---------------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------------


def analyse_transfer_batch(
    channels: Sequence[np.ndarray],
    pairs: Sequence[Tuple[int, int]],
    sample_rate_hz: int,
    pair_names: Sequence[str],
    settings: Optional[TransferSettings] = None,
) -> List[TransferPairResult]:
    """pairs[p] = (index of the reference, index of the measurement) into channels.  The pairs go through the device in
    batches of at most MAX_BATCH_CHANNELS pairs; each batch uploads the channels its pairs name, once each."""
    settings = settings or TransferSettings()
    if len(pairs) != len(pair_names):
        raise ValueError("one name per pair")
    chans = [np.asarray(c, dtype=np.float32).reshape(-1) for c in channels]
    for x, y in pairs:
        if not (0 <= int(x) < len(chans) and 0 <= int(y) < len(chans)):
            raise ValueError("pairs must index channels")
    out: List[TransferPairResult] = []
    eng = get_engine() if pairs else None
    for a in range(0, len(pairs), MAX_BATCH_CHANNELS):
        chunk = [(int(x), int(y)) for x, y in pairs[a : a + MAX_BATCH_CHANNELS]]
        used = sorted({i for xy in chunk for i in xy})
        row = {c: r for r, c in enumerate(used)}
        batch = eng.upload([chans[c] for c in used])
        res = transfer_device(eng, batch, [row[x] for x, _ in chunk], [row[y] for _, y in chunk], sample_rate_hz, settings)
        out += transfer_results(res, sample_rate_hz, pair_names[a : a + MAX_BATCH_CHANNELS], settings)
    return out


def analyse_transfer_from_wav_file(
    input_wav_file_path: str | Path,
    reference_channel: str = "left",
    settings: Optional[TransferSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[TransferPairResult]:
    """One stereo WAV file: reference_channel ("left" | "right") is the reference, the other channel the measurement."""
    return analyse_transfer_stereo_files([input_wav_file_path], reference_channel, settings, expected_sample_rate_hz)


def analyse_transfer_stereo_files(
    paths: Sequence[str | Path],
    reference_channel: str = "left",
    settings: Optional[TransferSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[TransferPairResult]:
    """Every stereo file a pair: its reference_channel against its other channel, named "<file name>:<measured channel>"."""
    if reference_channel not in ("left", "right"):
        raise ValueError(f"reference_channel must be 'left' or 'right', got {reference_channel!r}")
    chans, pairs, names = [], [], []
    for p in paths:
        loaded = load_wav_file(wav_file_path=p, expected_sample_rate_hz=expected_sample_rate_hz,
                               expected_channel_mode="mono_or_stereo", allow_mono_and_upmix_to_stereo=False)
        if loaded.samples.shape[1] != 2:
            raise ValueError(f"{p} is not a stereo file: --reference-channel needs two channels")
        left, right = (np.ascontiguousarray(loaded.samples[:, k]) for k in (0, 1))
        x, y, measured = (left, right, "right") if reference_channel == "left" else (right, left, "left")
        pairs.append((len(chans), len(chans) + 1))
        chans += [x, y]
        names.append(f"{Path(p).name}:{measured}")
    return analyse_transfer_batch(chans, pairs, int(expected_sample_rate_hz), names, settings)


def analyse_transfer_files(
    measured_paths: Sequence[str | Path],
    reference_path: str | Path,
    settings: Optional[TransferSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[TransferPairResult]:
    """Every channel of every measured file (mono or stereo WAV, rate checked; named "<file name>:<channel>") against the
    reference file, which is mixed down to mono as deconvolve_from_wav_files does."""
    settings = settings or TransferSettings()
    ref = load_wav_file(wav_file_path=reference_path, expected_sample_rate_hz=expected_sample_rate_hz,
                        expected_channel_mode="mono_or_stereo", allow_mono_and_upmix_to_stereo=False)
    named = list(M.file_channels(measured_paths, settings.use_mono_downmix_for_stereo, expected_sample_rate_hz))
    chans = [_downmix_to_mono_1d(ref.samples)] + [c for _, c in named]
    return analyse_transfer_batch(chans, [(0, 1 + i) for i in range(len(named))], int(expected_sample_rate_hz),
                                  [n for n, _ in named], settings)


# ---------------------------------------------------------------------------------------------------
# text, Markdown, JSON
# ---------------------------------------------------------------------------------------------------


def _head(r: TransferPairResult, sep: str, end: str) -> str:
    return (f"Delay: {r.delay_samples} samples ({1000.0 * r.delay_samples / r.sample_rate_hz:.3f} ms){sep}"
            f"Frames: {r.frames} of {r.n_fft} ({r.window}, hop {r.hop}){sep}"
            f"Mean coherence {r.band_hz[0]:g}-{r.band_hz[1]:g} Hz: {M.fmt(r.mean_coherence, 3)}{sep}"
            f"Bins at or above {r.coherence_threshold:g}: {M.fmt(100.0 * r.coherent_fraction, 1)} %{sep}"
            f"Status: {status_text(r.status)}{end}")


def _rows(r: TransferPairResult) -> List[List[str]]:
    return [[f"{b.centre_hz:.1f}", M.fmt(b.mag_db, 2), M.fmt(math.degrees(b.phase_rad), 1), M.fmt(b.coherence, 3),
             str(b.bins)] for b in r.rows]


def summarise_transfer_text(results: List[TransferPairResult]) -> str:
    """
    Fixed text format, one block per pair followed by an empty line:
        [<pair name>]
        Delay: <d> samples (<ms, 3 decimals> ms)  Frames: <K> of <n_fft> (<window>, hop <hop>)  Mean coherence <lo>-<hi> Hz:
          <3 decimals>  Bins at or above <threshold>: <1 decimal> %  Status: ok | <flags> (<words>)      (one line)
        Hz  Mag_dB  Phase_deg  Coherence  Bins
        <centre, 1 decimal>  <2 decimals>  <1 decimal>  <3 decimals>  <bins in the row>
    Cells are separated by two spaces; NaN (a row without bins, or a pair with a status) is "NA".
    """
    return M.join_blocks(M.text_block(r.pair_name, _head(r, "  ", ""), ["Mag_dB", "Phase_deg", "Coherence", "Bins"],
                                      _rows(r), first="Hz") for r in results)


def summarise_transfer_markdown(results: List[TransferPairResult]) -> str:
    """The same values as a Markdown section per pair: a '### <pair name>' heading, the head line and a table with a row
    per fractional-octave row."""
    return M.join_blocks(M.markdown_block(r.pair_name, _head(r, ". ", "."),
                                          ["Mag (dB)", "Phase (deg)", "Coherence", "Bins"], _rows(r), first="Hz")
                         for r in results)


def transfer_results_to_json(results: List[TransferPairResult]) -> Dict:
    """Plain JSON with the full per-bin arrays: NaN is null, an infinity "+inf" / "-inf"."""
    rows = []
    for r in results:
        rows.append({
            "pair_name": r.pair_name, "sample_rate_hz": r.sample_rate_hz, "n_fft": r.n_fft, "hop": r.hop, "window": r.window,
            "delay_samples": r.delay_samples, "samples": r.samples, "frames": r.frames, "status": r.status,
            "band_hz": list(r.band_hz), "coherence_threshold": r.coherence_threshold,
            "mean_coherence": M.json_num(r.mean_coherence), "coherent_fraction": M.json_num(r.coherent_fraction),
            "rows": [{"centre_hz": b.centre_hz, "low_edge_hz": b.low_edge_hz, "high_edge_hz": b.high_edge_hz, "bins": b.bins,
                      "mag_db": M.json_num(b.mag_db), "phase_rad": M.json_num(b.phase_rad),
                      "coherence": M.json_num(b.coherence)} for b in r.rows],
            "frequency_hz": [float(f) for f in r.frequency_hz],
            "arrays": {k: [M.json_num(float(v)) for v in r.arrays[k]] for k in ARRAYS},
        })
    return {"transfer": rows}


def transfer_results_from_json(doc: Dict) -> List[TransferPairResult]:
    out = []
    for d in doc["transfer"]:
        out.append(TransferPairResult(
            pair_name=d["pair_name"], sample_rate_hz=int(d["sample_rate_hz"]), n_fft=int(d["n_fft"]), hop=int(d["hop"]),
            window=str(d["window"]), delay_samples=int(d["delay_samples"]), samples=int(d["samples"]),
            frames=int(d["frames"]), status=int(d["status"]), band_hz=(float(d["band_hz"][0]), float(d["band_hz"][1])),
            coherence_threshold=float(d["coherence_threshold"]), mean_coherence=M.num_json(d["mean_coherence"]),
            coherent_fraction=M.num_json(d["coherent_fraction"]),
            rows=tuple(TransferBandRow(float(b["centre_hz"]), float(b["low_edge_hz"]), float(b["high_edge_hz"]),
                                       int(b["bins"]), M.num_json(b["mag_db"]), M.num_json(b["phase_rad"]),
                                       M.num_json(b["coherence"])) for b in d["rows"]),
            arrays={k: np.array([M.num_json(v) for v in d["arrays"][k]], dtype=np.float64) for k in ARRAYS}))
    return out


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def _delay_argument(text: str):
    if text == "auto":
        return text
    try:
        return int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--delay takes 'auto' or a whole number of samples, got {text!r}") from None


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.transfer",
        description="Dual-channel transfer function (Welch H1 / H2) and coherence between a reference and a measurement.")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--measured", nargs="+", type=Path,
                     help="measured WAV files (every channel of every file is a pair with --reference)")
    src.add_argument("--input", nargs="+", type=Path,
                     help="stereo WAV files holding reference and measurement (see --reference-channel)")
    p.add_argument("--reference", type=Path, default=None, help="with --measured: the signal that was played (mixed down to mono)")
    p.add_argument("--reference-channel", choices=["left", "right"], default=None,
                   help="with --input: the channel that holds the reference; the other one is the measurement")
    p.add_argument("--mono", action="store_true", help="with --measured: analyse stereo files as their mono downmix 0.5 * (L + R)")
    p.add_argument("--n-fft", type=int, default=4096, help="frame length, a power of two 256 .. 8192 (default: 4096)")
    p.add_argument("--overlap", type=float, default=0.5, help="overlap of consecutive frames, in [0, 1) (default: 0.5)")
    p.add_argument("--window", choices=list(WINDOWS), default="hann", help="frame window (default: hann)")
    p.add_argument("--delay", type=_delay_argument, default="auto",
                   help="samples the measurement lags the reference by (may be negative), or auto (default)")
    p.add_argument("--points-per-octave", type=int, default=3, help="rows per octave of the summary, 1 to 48 (default: 3)")
    p.add_argument("--coherence-threshold", type=float, default=0.5,
                   help="the summary counts the bins at or above this coherence (default: 0.5)")
    M.add_output_arguments(p)
    return p


def settings_from_args(args) -> TransferSettings:
    return TransferSettings(n_fft=args.n_fft, overlap=args.overlap, window=args.window, delay=args.delay,
                            points_per_octave=args.points_per_octave, coherence_threshold=args.coherence_threshold,
                            use_mono_downmix_for_stereo=bool(args.mono))


def main(argv: Optional[Sequence[str]] = None) -> None:
    # M.run_cli reads --input | --bundle; this measure takes two kinds of file, or two channels of one, instead
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.measured and (args.reference is None or args.reference_channel is not None):
        parser.error("--measured needs --reference (and takes no --reference-channel)")
    if args.input and (args.reference_channel is None or args.reference is not None or args.mono):
        parser.error("--input needs --reference-channel (and takes neither --reference nor --mono)")
    try:
        settings = settings_from_args(args)
    except ValueError as e:
        parser.error(str(e))
    if args.measured:
        results = analyse_transfer_files(args.measured, args.reference, settings, args.expected_sample_rate)
    else:
        results = analyse_transfer_stereo_files(args.input, args.reference_channel, settings, args.expected_sample_rate)
    sys.stdout.write(summarise_transfer_text(results))
    sys.stdout.flush()
    if args.json is not None:
        args.json.write_text(json.dumps(transfer_results_to_json(results), indent=2) + "\n")


if __name__ == "__main__":
    main()
