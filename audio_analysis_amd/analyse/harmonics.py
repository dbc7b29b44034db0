"""
Harmonic distortion against frequency (HD2 .. HDK, THD) from the recording of a logarithmic sweep.

Deconvolving an exponential sweep (Farina) of T seconds from f1 to f2 does more than give the linear response: every
harmonic the system under test produces is compressed into an impulse of its own at a fixed negative time, the k-th
L ln k seconds before the linear response, L = T / ln(f2 / f1).  `deconvolve_device` already computes those impulses (its
"recorded" output mode cuts them off); this module reads them.  The reference has no such measure.  For sample rate fs:

  1 response  h from deconvolve_device, unchanged: output_length_mode "full_fft", normalise_peak and remove_dc off, the
              setting's regularisation.  float32, circular, n_fft samples per channel (channels of a batch may differ).
  2 lags      d_k = floor(L fs ln k + 0.5) samples, k = 1 .. K (d_1 = 0); host float64.
  3 peak      p = the first maximum of |h| over [0, n_search), n_search = n_fft - ceil(L fs ln(K + 1)) - guard_samples
              (ira_peak_index on a view of h: nothing returns to the host).  The search must not see the harmonic region:
              what the system produces above f2 is amplified by the regularised inverse filter and lands there, and can be
              larger than the linear peak.
  4 window    one length for all harmonics, so that the ratios compare like with like:
              W = min(floor(window_ms fs / 1000), floor(L fs ln(K / (K - 1))) - guard_samples), seg = guard_samples + W,
              n_h = the next power of two >= seg.  w[i] (float64, host): 0.5 - 0.5 cos(pi (i + 0.5) / guard) for i < guard;
              0.5 + 0.5 cos(pi (m + 0.5) / nfade), m = i - (seg - nfade), over the last nfade = floor(fade_fraction W)
              samples; 1 elsewhere.
  5 segments  row (c, k): s[i] = float32(float64(h_c[(p_c - d_k - guard + i) mod n_fft_c]) * w[i]), i < seg
              (ira_harmonic_windows).
  6 spectra   every row zero-padded to n_h, all rows in one rfft_any call (float64 half spectra).
  7 powers    grid f_j = f1 2^(j / P), j = 0 .. floor(P log2(f2 / f1)); bin step df = fs / n_h.  Harmonic k is valid at j
              iff k f_j 2^(1/(2P)) <= min(f2, fs / 2); then a = ceil(k f_j 2^(-1/(2P)) / df), b = floor(k f_j 2^(1/(2P)) / df),
              a = b = floor(k f_j / df + 0.5) if b < a, both clamped to n_h / 2.  E_k(j) = the mean of re^2 + im^2 over the
              bins a .. b (ira_harmonic_band_powers; the tables lo / cnt are built once and shared by all channels).
  8 results   HD_k(j) = sqrt(E_k(j) / E_1(j)), k >= 2; THD(j) = sqrt(sum over the valid k >= 2 of E_k(j) / E_1(j)) with
              the number of harmonics in the sum; NaN where k is invalid (for THD: where k = 2 is); the fundamental level
              10 log10 E_1(j).  Host float64.

Per-channel status (bit flags; a channel with a non-zero status has NaN in every output, the batch carries on):
  1 silent (|h[p]| == 0), 2 too short (n_search < 1 or W < 64), 4 non-finite (the sum of E_1 over the grid is not finite).

Two properties of the method, both seen with exactly these formulas:
  Baseband term of even-order distortion.  A polynomial x + a2 x^2 also produces a rectified, DC-like pulse as long as the
    sweep.  Deconvolution smears that pulse over all negative time, where it swamps the low-frequency points, the
    fundamental included.  AC-coupled systems do not show this; the measure does not try to remove it.
  Low-frequency droop.  The lowest octave or two above f1 are biased by the sweep's fade-in and by the short common
    window; short sweeps are affected more.

Command line (no plots): python -m analyse.harmonics --recorded A.wav [B.wav ...] --sweep S.wav [--mono]
  [--sweep-seconds 10] [--f1 20] [--f2 20000] [--harmonics 5] [--points-per-octave 3] [--window-ms 200]
  [--expected-sample-rate 48000] [--json OUT.json]
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _measure as M
from ..engine import get_engine
from ._measure import MAX_BATCH_CHANNELS  # noqa: F401  (part of this module's surface)
from .deconvolve import MAX_LOG2_FFT, DeconvolveSettings, _downmix_to_mono_1d, _next_power_of_two, deconvolve_device
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ, load_wav_file

STATUS_SILENT = 1
STATUS_TOO_SHORT = 2
STATUS_NON_FINITE = 4
_STATUS_WORDS = ((STATUS_SILENT, "silent"), (STATUS_TOO_SHORT, "too short"), (STATUS_NON_FINITE, "non-finite"))

MAX_HARMONIC = 10                 # IRA_HARMONIC_MAX
MIN_WINDOW_SAMPLES = 64


@dataclass(frozen=True)
class HarmonicDistortionSettings:
    sweep_seconds: float = 10.0
    start_frequency_hz: float = 20.0
    end_frequency_hz: float = 20000.0
    max_harmonic: int = 5
    points_per_octave: int = 3
    window_ms: float = 200.0
    guard_samples: int = 64
    fade_fraction: float = 0.25
    regularization_relative: float = 1e-10
    use_mono_downmix_for_stereo: bool = False

    def __post_init__(self):
        t, f1, f2 = float(self.sweep_seconds), float(self.start_frequency_hz), float(self.end_frequency_hz)
        if not (math.isfinite(t) and t > 0.0):
            raise ValueError(f"sweep_seconds must be positive and finite, got {self.sweep_seconds}")
        if not (math.isfinite(f1) and math.isfinite(f2) and 0.0 < f1 < f2):
            raise ValueError(f"the sweep must run from 0 < start_frequency_hz to a higher end_frequency_hz, got {f1} .. {f2}")
        for name, lo, hi in (("max_harmonic", 2, MAX_HARMONIC), ("points_per_octave", 1, 48), ("guard_samples", 1, None)):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or int(v) < lo or (hi is not None and int(v) > hi):
                raise ValueError(f"{name} must be an integer " + (f"in {lo} .. {hi}" if hi is not None else f">= {lo}") + f", got {v}")
            object.__setattr__(self, name, int(v))
        w, fade, reg = float(self.window_ms), float(self.fade_fraction), float(self.regularization_relative)
        if not (math.isfinite(w) and w > 0.0):
            raise ValueError(f"window_ms must be positive and finite, got {self.window_ms}")
        if not (0.0 < fade <= 0.5):
            raise ValueError(f"fade_fraction must lie in (0, 0.5], got {self.fade_fraction}")
        if not (math.isfinite(reg) and reg >= 0.0):
            raise ValueError(f"regularization_relative must be finite and >= 0, got {self.regularization_relative}")
        for name, v in (("sweep_seconds", t), ("start_frequency_hz", f1), ("end_frequency_hz", f2), ("window_ms", w),
                        ("fade_fraction", fade), ("regularization_relative", reg)):
            object.__setattr__(self, name, v)

    @property
    def sweep_rate_seconds(self) -> float:
        """L = T / ln(f2 / f1): the k-th harmonic arrives L ln k seconds before the linear response."""
        return self.sweep_seconds / math.log(self.end_frequency_hz / self.start_frequency_hz)


@dataclass(frozen=True)
class HarmonicDistortionChannelResult:
    channel_name: str
    sample_rate_hz: int
    status: int
    peak_sample: int                            # p, the linear peak in the circular response
    window_samples: int                         # W
    fft_size: int                               # n_h
    frequencies_hz: Tuple[float, ...]           # f_j
    fundamental_db: Tuple[float, ...]           # 10 log10 E_1(j)
    hd: Tuple[Tuple[float, ...], ...]           # hd[k - 2][j] = HD_k(j), k = 2 .. K (a ratio)
    thd: Tuple[float, ...]                      # THD(j) (a ratio)
    harmonics_counted: Tuple[int, ...]          # how many harmonics THD(j) sums


@dataclass(frozen=True)
class HarmonicPlan:
    """Everything of steps 2, 4 and 7 that depends on the settings and the sample rate alone."""
    lags: np.ndarray                            # int64 (K,)
    search_margin: int                          # n_search = n_fft - search_margin
    window_samples: int                         # W (may be < MIN_WINDOW_SAMPLES: then nothing else is built)
    guard: int
    seg: int
    fft_size: int
    window: Optional[np.ndarray]                # float64 (seg,)
    frequencies: np.ndarray                     # float64 (J,)
    lo: Optional[np.ndarray]                    # int32 (K, J)
    cnt: Optional[np.ndarray]                   # int32 (K, J)

    @property
    def usable(self) -> bool:
        return self.window_samples >= MIN_WINDOW_SAMPLES


@dataclass
class HarmonicSums:
    """What harmonic_distortion_device leaves on the host."""
    plan: HarmonicPlan
    n_fft: np.ndarray                           # int64 (nch,)
    peak: np.ndarray                            # int64 (nch,)
    peak_abs: np.ndarray                        # float32 (nch,)
    powers: np.ndarray                          # float64 (nch, K, J) mean band powers E_k(j)


def status_text(status: int) -> str:
    return M.status_text(status, _STATUS_WORDS)


# ---------------------------------------------------------------------------------------------------
# host: lags, window, tables
# ---------------------------------------------------------------------------------------------------


def harmonic_lags(settings: HarmonicDistortionSettings, sample_rate_hz: float) -> np.ndarray:
    scale = settings.sweep_rate_seconds * float(sample_rate_hz)
    return np.array([math.floor(scale * math.log(k) + 0.5) for k in range(1, settings.max_harmonic + 1)], dtype=np.int64)


def harmonic_window(guard: int, window_samples: int, fade_fraction: float) -> np.ndarray:
    """w of step 4: a raised-cosine rise over the guard samples in front of the peak, 1, a raised-cosine fall over the last
    floor(fade_fraction W) samples."""
    seg = guard + window_samples
    nfade = int(math.floor(fade_fraction * window_samples))
    w = np.ones(seg, dtype=np.float64)
    w[:guard] = [0.5 - 0.5 * math.cos(math.pi * (i + 0.5) / guard) for i in range(guard)]
    w[seg - nfade:] = [0.5 + 0.5 * math.cos(math.pi * (m + 0.5) / nfade) for m in range(nfade)]
    return w


def frequency_grid(settings: HarmonicDistortionSettings) -> np.ndarray:
    p = settings.points_per_octave
    top = int(math.floor(p * math.log2(settings.end_frequency_hz / settings.start_frequency_hz)))
    return np.array([settings.start_frequency_hz * 2.0 ** (j / p) for j in range(top + 1)], dtype=np.float64)


def band_tables(settings: HarmonicDistortionSettings, sample_rate_hz: float, fft_size: int):
    """(f (J,), lo (K, J), cnt (K, J)) of step 7: harmonic k at grid point j covers the bins lo .. lo + cnt - 1 of an
    fft_size-point half spectrum; cnt = 0 where the harmonic is invalid."""
    f = frequency_grid(settings)
    k_max, p = settings.max_harmonic, settings.points_per_octave
    df = float(sample_rate_hz) / fft_size
    half_up, half_down = 2.0 ** (1.0 / (2 * p)), 2.0 ** (-1.0 / (2 * p))
    limit = min(settings.end_frequency_hz, float(sample_rate_hz) / 2.0)
    lo = np.zeros((k_max, f.size), dtype=np.int32)
    cnt = np.zeros((k_max, f.size), dtype=np.int32)
    for k in range(1, k_max + 1):
        for j in range(f.size):
            centre = k * float(f[j])
            if centre * half_up > limit:
                continue
            a = int(math.ceil(centre * half_down / df))
            b = int(math.floor(centre * half_up / df))
            if b < a:
                a = b = int(math.floor(centre / df + 0.5))
            a, b = min(a, fft_size // 2), min(b, fft_size // 2)
            lo[k - 1, j], cnt[k - 1, j] = a, b - a + 1
    return f, lo, cnt


def harmonic_plan(settings: HarmonicDistortionSettings, sample_rate_hz: float) -> HarmonicPlan:
    fs = float(sample_rate_hz)
    if not (fs > 0.0 and settings.end_frequency_hz <= fs / 2.0):
        raise ValueError(f"end_frequency_hz {settings.end_frequency_hz} must not exceed half the sample rate {sample_rate_hz}")
    k, guard = settings.max_harmonic, settings.guard_samples
    scale = settings.sweep_rate_seconds * fs
    margin = int(math.ceil(scale * math.log(k + 1))) + guard
    w_len = min(int(math.floor(settings.window_ms * fs / 1000.0)), int(math.floor(scale * math.log(k / (k - 1)))) - guard)
    lags = harmonic_lags(settings, fs)
    if w_len < MIN_WINDOW_SAMPLES:
        return HarmonicPlan(lags, margin, w_len, guard, 0, 0, None, frequency_grid(settings), None, None)
    seg = guard + w_len
    n_h = _next_power_of_two(seg)
    f, lo, cnt = band_tables(settings, fs, n_h)
    return HarmonicPlan(lags, margin, w_len, guard, seg, n_h, harmonic_window(guard, w_len, settings.fade_fraction), f, lo, cnt)


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def harmonic_distortion_device(eng, recorded, file_of_channel: Sequence[int], sweeps, sweep_of_channel: Sequence[int],
                               sample_rate_hz: int, settings: Optional[HarmonicDistortionSettings] = None,
                               response: Optional[Dict] = None) -> HarmonicSums:
    """
    Mean band powers E_k(j) of every channel of a device batch of recordings: the deconvolution, one peak pick, ONE
    ira_harmonic_windows launch, one rfft_any call over all nch * K rows and ONE ira_harmonic_band_powers launch.
    recorded / file_of_channel / sweeps / sweep_of_channel: as deconvolve_device takes them.  response = what
    deconvolve_device returned for them (full_fft, unnormalised) lets a caller that already holds the responses skip
    the deconvolution.
    """
    settings = settings or HarmonicDistortionSettings()
    plan = harmonic_plan(settings, sample_rate_hz)
    if response is None:
        response = deconvolve_device(eng, recorded, file_of_channel, sweeps, sweep_of_channel, sample_rate_hz,
                                     DeconvolveSettings(regularization_relative=settings.regularization_relative,
                                                        normalise_peak=False, remove_dc=False,
                                                        output_length_mode="full_fft"))
    n_fft = np.asarray(response["n_fft"], dtype=np.int64)
    nch = int(n_fft.size)
    k, j = settings.max_harmonic, int(plan.frequencies.size)
    if nch == 0 or not plan.usable:
        return HarmonicSums(plan, n_fft, np.zeros(nch, np.int64), np.zeros(nch, np.float32), np.zeros((nch, k, j)))
    # a channel too short for the search (status 2) still rides the launches: its peak is looked for in one sample
    n_search = np.maximum(n_fft - plan.search_margin, 1)
    peak_dev, peak_abs_dev = eng.harmonic_peaks(response["h"], response["off"], n_search)
    rows = eng.harmonic_windows(response["h"], response["off"], n_fft, peak_dev, plan.lags, plan.guard, plan.window)
    nrow = nch * k
    spec, spec_off = eng.rfft_any(rows, np.arange(nrow, dtype=np.int64) * plan.seg, np.full(nrow, plan.fft_size, np.int32),
                                  False, data_len=np.full(nrow, plan.seg, np.int32),
                                  win_len=np.full(nrow, plan.fft_size, np.int32))
    powers = eng.harmonic_band_powers(spec, spec_off, plan.lo, plan.cnt, plan.fft_size // 2 + 1)
    return HarmonicSums(plan, n_fft, peak_dev.cpu().numpy().copy(), peak_abs_dev.cpu().numpy().copy(),
                        powers.cpu().numpy().copy())


# ---------------------------------------------------------------------------------------------------
# host: band powers -> ratios
# ---------------------------------------------------------------------------------------------------


def distortion_from_powers(powers: np.ndarray, cnt: np.ndarray):
    """(HD (..., K - 1, J), THD (..., J), harmonics counted (J,), fundamental dB (..., J)) from mean band powers
    (..., K, J) and the validity table cnt (K, J); NaN where a harmonic (for THD: the second) is invalid."""
    e = np.asarray(powers, dtype=np.float64)
    valid = np.asarray(cnt) > 0
    nan = float("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        fund = np.where(valid[0], 10.0 * np.log10(e[..., 0, :]), nan)
        hd = np.where(valid[1:], np.sqrt(e[..., 1:, :] / e[..., :1, :]), nan)
        total = np.zeros_like(e[..., 0, :])
        for i in range(1, e.shape[-2]):                       # ascending k: the order of the sum is fixed
            total = total + np.where(valid[i], e[..., i, :], 0.0)
        thd = np.where(valid[1], np.sqrt(total / e[..., 0, :]), nan)
    return hd, thd, valid[1:].sum(axis=0).astype(np.int64), fund


def harmonic_distortion_results(res: HarmonicSums, sample_rate_hz: int, channel_names: Sequence[str],
                                settings: HarmonicDistortionSettings) -> List[HarmonicDistortionChannelResult]:
    plan = res.plan
    k, j = settings.max_harmonic, int(plan.frequencies.size)
    if plan.usable:
        hd, thd, counted, fund = distortion_from_powers(res.powers, plan.cnt)
    nan_row = tuple(float("nan") for _ in range(j))
    out = []
    for ch, name in enumerate(channel_names):
        status = 0
        if not plan.usable or int(res.n_fft[ch]) - plan.search_margin < 1:
            status |= STATUS_TOO_SHORT
        else:                                                 # the peak and the powers of a channel too short mean nothing
            if float(res.peak_abs[ch]) == 0.0:
                status |= STATUS_SILENT
            if not math.isfinite(float(np.sum(res.powers[ch, 0]))):
                status |= STATUS_NON_FINITE
        common = dict(channel_name=str(name), sample_rate_hz=int(sample_rate_hz), status=status,
                      peak_sample=int(res.peak[ch]), window_samples=int(plan.window_samples), fft_size=int(plan.fft_size),
                      frequencies_hz=tuple(float(v) for v in plan.frequencies))
        if status:
            out.append(HarmonicDistortionChannelResult(fundamental_db=nan_row, hd=tuple(nan_row for _ in range(k - 1)),
                                                       thd=nan_row, harmonics_counted=tuple(0 for _ in range(j)), **common))
        else:
            out.append(HarmonicDistortionChannelResult(
                fundamental_db=tuple(float(v) for v in fund[ch]), hd=tuple(tuple(float(v) for v in row) for row in hd[ch]),
                thd=tuple(float(v) for v in thd[ch]), harmonics_counted=tuple(int(v) for v in counted), **common))
    return out


# ---------------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------------


def _check_transform_size(channel_lengths: Sequence[int], sweep_length: int) -> None:
    longest = max([int(sweep_length), *[int(n) for n in channel_lengths]], default=0)
    if _next_power_of_two(longest) > (1 << MAX_LOG2_FFT):
        raise ValueError(f"a recording or the sweep needs a transform of more than 2^{MAX_LOG2_FFT} points "
                         f"({longest} samples): deconvolution transforms are limited to that on the GPU path")


def analyse_harmonic_distortion_batch(
    channels: Sequence[np.ndarray],
    sweep: np.ndarray,
    sample_rate_hz: int,
    channel_names: Sequence[str],
    settings: Optional[HarmonicDistortionSettings] = None,
) -> List[HarmonicDistortionChannelResult]:
    """Every recorded channel, deconvolved with the one mono sweep, through the device in batches of at most
    MAX_BATCH_CHANNELS channels.  ValueError, before anything is uploaded or launched, when a transform would exceed
    2^21 points."""
    settings = settings or HarmonicDistortionSettings()
    if len(channels) != len(channel_names):
        raise ValueError("one name per channel")
    sweep = np.asarray(sweep, dtype=np.float32).reshape(-1)
    chans = [np.asarray(c, dtype=np.float32).reshape(-1) for c in channels]
    _check_transform_size([c.size for c in chans], sweep.size)
    harmonic_plan(settings, sample_rate_hz)                   # the sample-rate check, before the engine is touched
    eng = get_engine()
    out: List[HarmonicDistortionChannelResult] = []
    sw = eng.upload([sweep]) if chans else None
    for a in range(0, len(chans), MAX_BATCH_CHANNELS):
        chunk = chans[a : a + MAX_BATCH_CHANNELS]
        batch = eng.upload(chunk)
        # no peak normalisation: which file a channel belongs to changes nothing, every channel is its own group
        res = harmonic_distortion_device(eng, batch, list(range(len(chunk))), sw, [0] * len(chunk), sample_rate_hz, settings)
        out += harmonic_distortion_results(res, sample_rate_hz, channel_names[a : a + MAX_BATCH_CHANNELS], settings)
    return out


def analyse_harmonic_distortion_from_wav_files(
    recorded_paths: Sequence[str | Path],
    sweep_path: str | Path,
    settings: Optional[HarmonicDistortionSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[HarmonicDistortionChannelResult]:
    """Every channel of every recording (mono or stereo WAV, rate checked; named "<file name>:<channel>") against the sweep
    file, which is mixed down to mono as deconvolve_from_wav_files does.  ValueError when the sweep file is shorter than
    sweep_seconds, or when a transform would exceed 2^21 points."""
    settings = settings or HarmonicDistortionSettings()
    sweep = load_wav_file(wav_file_path=sweep_path, expected_sample_rate_hz=expected_sample_rate_hz,
                          expected_channel_mode="mono_or_stereo", allow_mono_and_upmix_to_stereo=False)
    mono = _downmix_to_mono_1d(sweep.samples)
    if mono.size < settings.sweep_seconds * float(expected_sample_rate_hz):
        raise ValueError(f"{sweep_path} holds {mono.size} samples, fewer than the {settings.sweep_seconds:g} s sweep at "
                         f"{expected_sample_rate_hz} Hz")
    named = list(M.file_channels(recorded_paths, settings.use_mono_downmix_for_stereo, expected_sample_rate_hz))
    return analyse_harmonic_distortion_batch([c for _, c in named], mono, int(expected_sample_rate_hz),
                                             [n for n, _ in named], settings)


# ---------------------------------------------------------------------------------------------------
# text, Markdown, JSON
# ---------------------------------------------------------------------------------------------------


def _db(ratio: float) -> float:
    if math.isnan(ratio):
        return ratio
    return 20.0 * math.log10(ratio) if ratio > 0.0 else float("-inf")


def _columns(r: HarmonicDistortionChannelResult) -> List[str]:
    return ["H1_dB"] + [f"HD{k}_dB" for k in range(2, len(r.hd) + 2)] + ["THD_%"]


def _rows(r: HarmonicDistortionChannelResult) -> List[List[str]]:
    return [[f"{f:.1f}", M.fmt(r.fundamental_db[j], 2)] + [M.fmt(_db(row[j]), 2) for row in r.hd]
            + [M.fmt(100.0 * r.thd[j], 4)] for j, f in enumerate(r.frequencies_hz)]


def _head(r: HarmonicDistortionChannelResult, sep: str, end: str) -> str:
    return (f"Peak: sample {r.peak_sample}{sep}Window: {r.window_samples} samples, {r.fft_size}-point spectra{sep}"
            f"Status: {status_text(r.status)}{end}")


def summarise_harmonic_distortion_text(channel_results: List[HarmonicDistortionChannelResult]) -> str:
    """
    Fixed text format, one block per channel followed by an empty line:
        [<channel name>]
        Peak: sample <p>  Window: <W> samples, <n_h>-point spectra  Status: ok | <flags> (<words>)
        Hz  H1_dB  HD2_dB  ...  HDK_dB  THD_%
        <f_j, 1 decimal>  <10 log10 E_1, 2 decimals>  <20 log10 HD_k, 2 decimals> ...  <100 THD, 4 decimals>
    one row per grid frequency, ascending.  Cells are separated by two spaces; NaN is "NA", a ratio of 0 "-inf".
    """
    return M.join_blocks(M.text_block(r.channel_name, _head(r, "  ", ""), _columns(r), _rows(r), first="Hz")
                         for r in channel_results)


def summarise_harmonic_distortion_markdown(channel_results: List[HarmonicDistortionChannelResult]) -> str:
    """The same values as a Markdown section per channel: a '### <channel name>' heading, the peak / window / status line
    and a table with a row per grid frequency (levels in dB, THD in per cent)."""
    return M.join_blocks(M.markdown_block(
        r.channel_name, _head(r, ". ", "."), ["H1 (dB)"] + [f"HD{k} (dB)" for k in range(2, len(r.hd) + 2)] + ["THD (%)"],
        _rows(r), first="Hz") for r in channel_results)


def harmonic_results_to_json(channel_results: List[HarmonicDistortionChannelResult]) -> Dict:
    """Plain JSON: NaN is null, an infinity the string "+inf" / "-inf".  Ratios, not dB or per cent."""
    rows = []
    for r in channel_results:
        rows.append({
            "channel_name": r.channel_name, "sample_rate_hz": r.sample_rate_hz, "status": r.status,
            "peak_sample": r.peak_sample, "window_samples": r.window_samples, "fft_size": r.fft_size,
            "max_harmonic": len(r.hd) + 1,
            "points": [{"frequency_hz": f, "fundamental_db": M.json_num(r.fundamental_db[j]),
                        "hd": [M.json_num(row[j]) for row in r.hd], "thd": M.json_num(r.thd[j]),
                        "harmonics_counted": r.harmonics_counted[j]} for j, f in enumerate(r.frequencies_hz)],
        })
    return {"harmonic_distortion": rows}


def harmonic_results_from_json(doc: Dict) -> List[HarmonicDistortionChannelResult]:
    out = []
    for d in doc["harmonic_distortion"]:
        pts = d["points"]
        nk = int(d["max_harmonic"]) - 1
        out.append(HarmonicDistortionChannelResult(
            channel_name=d["channel_name"], sample_rate_hz=int(d["sample_rate_hz"]), status=int(d["status"]),
            peak_sample=int(d["peak_sample"]), window_samples=int(d["window_samples"]), fft_size=int(d["fft_size"]),
            frequencies_hz=tuple(float(p["frequency_hz"]) for p in pts),
            fundamental_db=tuple(M.num_json(p["fundamental_db"]) for p in pts),
            hd=tuple(tuple(M.num_json(p["hd"][i]) for p in pts) for i in range(nk)),
            thd=tuple(M.num_json(p["thd"]) for p in pts),
            harmonics_counted=tuple(int(p["harmonics_counted"]) for p in pts)))
    return out


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.harmonics",
        description="Harmonic distortion against frequency (HD2 .. HDK, THD) from recordings of a logarithmic sweep.")
    p.add_argument("--recorded", nargs="+", type=Path, required=True,
                   help="recorded WAV files (every channel of every file is analysed)")
    p.add_argument("--sweep", type=Path, required=True, help="the sweep that was played (mixed down to mono)")
    p.add_argument("--mono", action="store_true", help="analyse stereo recordings as their mono downmix 0.5 * (L + R)")
    p.add_argument("--sweep-seconds", type=float, default=10.0, help="duration T of the sweep (default: 10)")
    p.add_argument("--f1", type=float, default=20.0, help="start frequency of the sweep in Hz (default: 20)")
    p.add_argument("--f2", type=float, default=20000.0, help="end frequency of the sweep in Hz (default: 20000)")
    p.add_argument("--harmonics", type=int, default=5, help="highest harmonic K, 2 to 10 (default: 5)")
    p.add_argument("--points-per-octave", type=int, default=3, help="grid points per octave, 1 to 48 (default: 3)")
    p.add_argument("--window-ms", type=float, default=200.0, help="longest window per harmonic in ms (default: 200)")
    M.add_output_arguments(p)
    return p


def settings_from_args(args) -> HarmonicDistortionSettings:
    return HarmonicDistortionSettings(sweep_seconds=args.sweep_seconds, start_frequency_hz=args.f1, end_frequency_hz=args.f2,
                                      max_harmonic=args.harmonics, points_per_octave=args.points_per_octave,
                                      window_ms=args.window_ms, use_mono_downmix_for_stereo=bool(args.mono))


def main(argv: Optional[Sequence[str]] = None) -> None:
    # M.run_cli reads --input | --bundle; this measure has two kinds of input file instead, the rest is the same
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        settings = settings_from_args(args)
    except ValueError as e:
        parser.error(str(e))
    results = analyse_harmonic_distortion_from_wav_files(args.recorded, args.sweep, settings, args.expected_sample_rate)
    sys.stdout.write(summarise_harmonic_distortion_text(results))
    sys.stdout.flush()
    if args.json is not None:
        args.json.write_text(json.dumps(harmonic_results_to_json(results), indent=2) + "\n")


if __name__ == "__main__":
    main()
