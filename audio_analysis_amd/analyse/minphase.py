"""
Minimum phase, excess phase and excess group delay per channel, and the minimum-phase version of an impulse response.
frequency_response.py and filterplot.py show a channel's magnitude and phase, group_delay.py, fdw.py and burstdecay.py its
group delay; this module says how much of that phase is simply what the magnitude implies (the minimum phase, which a
minimum-phase equaliser undoes together with the magnitude) and how much is delay, all-pass behaviour or a reflection (the
excess phase, which no such equaliser can undo).  The method is the homomorphic one: the real cepstrum of the log
magnitude, folded onto its causal half (Oppenheim and Schafer).

For a channel x (float32) of L samples at the sample rate fs:

  centre    p = the peak (first index of max |x|) or the onset (eng.onset_index, onset_db = -20), as in fdw.py
  segment   the first D = min(L, p + 1 + rint(post_ms fs / 1000)) samples (post_ms None, the default: D = L)
  size      N = the power of two >= oversample * D (oversample 4 by default, a whole number >= 2), at least 32;
            ValueError above 2^21 (deconvolve.py's MAX_LOG2_FFT), naming oversample and post_ms as the remedies
  X         = rfft(x[:D], n = N), no window                            (Engine.rfft_any, data_len = D, win_len = N)
  floor     P = max_k |X_k|^2, |X|^2 = re^2 + im^2 in float64;  P_floor = P * 10^(floor_db / 10), floor_db = -120
  G_k       = 0.5 ln(max(|X_k|^2, P_floor)),  k = 0 .. N/2            (ira_minphase_logmag, written as the complex (G, 0))
  c         = float32(irfft(G, N))                                     (Engine.band_irfft, all-pass record 2, -1, -1)
  T         = rfft(c[0 : N/2], n = N)                                  (Engine.rfft_any, data_len = N/2)
  phi_min_k = 2 Im T_k     -- the folded cepstrum c[0], 2 c[n], c[N/2], 0.. has exactly this imaginary transform,
                              so no fold pass exists; phi_min is continuous, it is never wrapped
  phi_rel_k = angle(X_k) + 2 pi frac(k p / N), k p mod N reduced in int64 before the division: the phase with the
              delay to the centre taken out
  excess_k  = numpy.unwrap over k = 0 .. N/2 of wrap(phi_rel_k - phi_min_k), wrap(d) = d - 2 pi rint(d / (2 pi))
              (ira_minphase_excess, then the existing ira_phase_unwrap)
  tau_e_k   = -(excess_{k+1} - excess_{k-1}) / (4 pi / N) samples, tau_min_k likewise from phi_min, 1 <= k <= N/2 - 1

The cepstrum passes through float32 because the project's inverse transforms write float32: that moves phi_min by at
most 2^-23 sum |c[n]| (DESIGN.md has the bound and what was observed).

Outputs on the logarithmic grid of fdw_grid (points_per_octave 48, f_min 20, f_max 20000), each point taken at the bin
k_j = clip(rint(f_j N / fs), 1, N/2 - 1), from the record ira_minphase_gather leaves per (channel, point), in float64 NumPy
on the host (minphase_arithmetic; exactly restatable):

  frequencies_hz               k fs / N, the frequency of the bin
  bin                          k
  level_db                     10 log10(max(|X_k|^2, P_floor))
  phase_deg                    wrap(phi_rel_k) in degrees
  minimum_phase_deg            phi_min_k in degrees
  excess_phase_deg             excess_k in degrees, unwrapped
  excess_group_delay_seconds   tau_e_k / fs
  minimum_group_delay_seconds  tau_min_k / fs
  floored                      |X_k|^2 < P_floor
and per channel the centre, N and D, floored_share (the floored bins over all N/2 + 1 bins), excess_delay_seconds (the mean
of tau_e over the grid points weighted by |X|^2, divided by fs) and excess_phase_span_deg (max - min of the unwrapped
excess phase over the grid).

A channel of digital silence (P == 0, or no sample at all) has no values: everything is NaN, and nothing takes the
logarithm of zero.  A NaN or an infinity in the segment makes that channel NaN and touches no other channel.

The minimum-phase response itself (minimum_phase_device stays on the device, minimum_phase_impulse_responses returns
float32 arrays):

  M_k   = e^{G_k} (cos phi_min_k, sin phi_min_k), the imaginary part forced to 0 at k = 0 and N/2   (ira_minphase_spectrum)
  h_min = float32(irfft(M, N)), all-pass band_irfft, the first D samples kept

The defaults are conventions of measurement tools, not citations.

Command line (no plots): python -m analyse.minphase --input A.wav [B.wav ...] | --bundle DIR [--mono] [--oversample 4]
  [--post-ms T] [--floor-db -120] [--points-per-octave 48] [--f-min 20] [--f-max 20000] [--centre peak|onset]
  [--onset-db -20] [--no-curve] [--write-minimum-phase DIR] [--expected-sample-rate 48000] [--json OUT.json]
"""
from __future__ import annotations

import argparse
import json
import math
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _measure as M
from .. import engine as E
from ..engine import MINPHASE_FIELDS, MINPHASE_MAX_LOG2, MINPHASE_MIN_FLOOR_DB, MINPHASE_MIN_N
from ._measure import MAX_BATCH_CHANNELS  # noqa: F401  (part of this module's surface)
from .deconvolve import MAX_LOG2_FFT
from .fdw import FdwSettings, fdw_grid
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ

assert MAX_LOG2_FFT == MINPHASE_MAX_LOG2

CENTRES = ("peak", "onset")
TWO_PI = 2.0 * math.pi
_CURVES = ("frequencies_hz", "bin", "level_db", "phase_deg", "minimum_phase_deg", "excess_phase_deg",
           "excess_group_delay_seconds", "minimum_group_delay_seconds", "floored")


@dataclass(frozen=True)
class MinPhaseSettings:
    oversample: int = 4
    post_ms: Optional[float] = None                # None: the whole channel
    floor_db: float = -120.0                       # the magnitude floor under the logarithm, relative to the largest bin
    points_per_octave: int = 48
    f_min_hz: float = 20.0
    f_max_hz: float = 20000.0                      # clipped to the Nyquist frequency of the channel
    centre: str = "peak"
    onset_db: float = -20.0
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

        def whole(name, least):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least:
                raise ValueError(f"{name} must be a whole number >= {least}, got {v!r}")
            return int(v)

        over, ppo = whole("oversample", 2), whole("points_per_octave", 1)
        f_min, f_max, onset, floor = number("f_min_hz", True), number("f_max_hz", True), number("onset_db"), number("floor_db")
        post = None if self.post_ms is None else number("post_ms")
        if post is not None and post < 0.0:
            raise ValueError(f"post_ms must be >= 0 (or None for the whole channel), got {self.post_ms}")
        if not (MINPHASE_MIN_FLOOR_DB <= floor < 0.0):
            raise ValueError(f"floor_db must lie in {MINPHASE_MIN_FLOOR_DB:g} .. 0 (below 0), got {self.floor_db}")
        if f_max < f_min:
            raise ValueError(f"f_max_hz must be at least f_min_hz, got {self.f_min_hz} .. {self.f_max_hz}")
        if self.centre not in CENTRES:
            raise ValueError(f"centre must be one of {CENTRES}, got {self.centre!r}")
        if onset > 0.0:
            raise ValueError(f"onset_db must be a finite level <= 0 dB relative to the peak, got {self.onset_db}")
        for k, v in (("oversample", over), ("points_per_octave", ppo), ("f_min_hz", f_min), ("f_max_hz", f_max),
                     ("onset_db", onset), ("floor_db", floor), ("post_ms", post)):
            object.__setattr__(self, k, v)

    @property
    def rel_energy(self) -> float:
        return 10.0 ** (self.onset_db / 10.0)

    @property
    def floor_ratio(self) -> float:
        return 10.0 ** (self.floor_db / 10.0)


@dataclass(frozen=True, eq=False)
class MinPhaseChannelResult:
    channel_name: str
    sample_rate_hz: int
    centre: str                                    # "peak" | "onset"
    centre_samples: int
    centre_seconds: float
    segment_samples: int                           # D
    fft_size: int                                  # N
    floor_db: float
    points_per_octave: int
    floored_share: float                           # floored bins / (N/2 + 1); NaN without values
    excess_delay_seconds: float
    excess_phase_span_deg: float
    # per frequency point; None: not kept (a JSON written with --no-curve)
    frequencies_hz: Optional[np.ndarray] = None
    bin: Optional[np.ndarray] = None               # int64
    level_db: Optional[np.ndarray] = None
    phase_deg: Optional[np.ndarray] = None
    minimum_phase_deg: Optional[np.ndarray] = None
    excess_phase_deg: Optional[np.ndarray] = None
    excess_group_delay_seconds: Optional[np.ndarray] = None
    minimum_group_delay_seconds: Optional[np.ndarray] = None
    floored: Optional[np.ndarray] = None           # bool


@dataclass
class MinPhaseRecords:
    """What minphase_device leaves on the host: the grid, per channel the length, the centre, D, N, its bins, P and the
    count of floored bins, and the record of MINPHASE_FIELDS doubles per (channel, point): Re X, Im X, Im T at k - 1, k,
    k + 1, the unwrapped excess phase at k - 1, k, k + 1."""
    settings: MinPhaseSettings
    grid_hz: np.ndarray                            # float64 (J,)
    length: np.ndarray                             # int64 (nch,)
    centre: np.ndarray                             # int64 (nch,)
    segment: np.ndarray                            # int64 (nch,): D
    n_fft: np.ndarray                              # int64 (nch,): N
    bins: np.ndarray                               # int64 (nch, J)
    pmax: np.ndarray                               # float64 (nch,): P; 0 for an empty channel
    floored: np.ndarray                            # int64 (nch,)
    records: np.ndarray                            # float64 (nch, J, MINPHASE_FIELDS)


def minphase_grid(settings: MinPhaseSettings, sample_rate_hz: float) -> np.ndarray:
    """The grid frequencies f_j: fdw_grid's, f_min 2^(j / ppo) while f_j <= min(f_max, fs / 2)."""
    return fdw_grid(FdwSettings(points_per_octave=settings.points_per_octave, f_min_hz=settings.f_min_hz,
                                f_max_hz=settings.f_max_hz), sample_rate_hz)[0]


def minphase_sizes(length, centre, sample_rate_hz: float, settings: MinPhaseSettings) -> Tuple[np.ndarray, np.ndarray]:
    """(D, N) per channel, int64: D = min(L, p + 1 + rint(post_ms fs / 1000)) (L without post_ms), N = the power of two >=
    oversample * D, at least 32.  ValueError where N would exceed 2^21."""
    length = np.asarray(length, dtype=np.int64).reshape(-1)
    centre = np.asarray(centre, dtype=np.int64).reshape(-1)
    if settings.post_ms is None:
        seg = length.copy()
    else:
        seg = np.minimum(length, centre + 1 + int(np.rint(settings.post_ms * float(sample_rate_hz) / 1000.0)))
    seg = np.maximum(seg, 0)
    n_fft = np.array([max(MINPHASE_MIN_N, 1 << int(max(settings.oversample * int(d), 1) - 1).bit_length()) for d in seg],
                     dtype=np.int64)
    if n_fft.size and n_fft.max() > 1 << MAX_LOG2_FFT:
        worst = int(np.argmax(n_fft))
        raise ValueError(f"a segment of {int(seg[worst])} samples at oversample {settings.oversample} needs a transform of "
                         f"{int(n_fft[worst])} points, at most 2^{MAX_LOG2_FFT}: lower oversample or set post_ms")
    return seg, n_fft


def minphase_bins(grid_hz: np.ndarray, n_fft, sample_rate_hz: float) -> np.ndarray:
    """k_j = clip(rint(f_j N / fs), 1, N/2 - 1) per channel: int64 (nch, J)."""
    n = np.asarray(n_fft, dtype=np.int64).reshape(-1, 1)
    k = np.rint(np.asarray(grid_hz, dtype=np.float64)[None, :] * n.astype(np.float64) / float(sample_rate_hz))
    return np.clip(k, 1, n // 2 - 1).astype(np.int64)


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def _centres(eng, batch, settings: MinPhaseSettings, centre_samples) -> np.ndarray:
    """The centre of every channel on the host (the sizes of the transforms depend on it when post_ms is set)."""
    if centre_samples is not None:
        centre = np.asarray(centre_samples, dtype=np.int64).reshape(-1)
        if centre.size != batch.count or (centre.size and (centre.min() < 0 or np.any(centre >= np.maximum(batch.length, 1)))):
            raise ValueError("centre_samples must give one sample index inside every channel")
        return centre
    onset_dev, peak_dev, _ = eng.onset_index(batch, settings.rel_energy)
    centre_dev = peak_dev if settings.centre == "peak" else onset_dev
    return centre_dev.cpu().numpy().astype(np.int64)[: batch.count].copy()


def _chain(eng, x_dev, off: np.ndarray, seg: np.ndarray, n_fft: np.ndarray, sample_rate_hz: float, floor_db: float):
    """X, G -> c -> T of one sub-batch (every channel with D >= 1): dict(spec, spec_off, g, tspec, pmax, floored, n32)."""
    t = eng.torch
    n32, d32 = n_fft.astype(np.int32), seg.astype(np.int32)
    spec, spec_off = eng.rfft_any(x_dev, off, n32, False, data_len=d32, win_len=n32)
    g, pmax, floored = eng.minphase_logmag(spec, spec_off, n32, floor_db)
    # the inverse: all-pass "band" (a high-pass whose pass edge lies below 0 Hz), float32 out, N samples each
    c_off = E.exclusive_cumsum(n_fft)
    c = eng.empty(int(n_fft.sum()), t.float32)
    allpass = np.zeros((n32.size, 8), dtype=np.float64)
    allpass[:, 0], allpass[:, 1], allpass[:, 2] = 2.0, -1.0, -1.0
    bin_step = float(sample_rate_hz) / n_fft.astype(np.float64)
    eng.band_irfft(g, spec_off, n32, allpass, bin_step, c, c_off)
    tspec, tspec_off = eng.rfft_any(c, c_off, n32, False, data_len=n32 // 2, win_len=n32)
    assert np.array_equal(tspec_off, spec_off)
    return dict(spec=spec, spec_off=spec_off, g=g, tspec=tspec, pmax=pmax, floored=floored, n32=n32, allpass=allpass,
                bin_step=bin_step, c_off=c_off)


def minphase_device(eng, batch, sample_rate_hz: int, settings: Optional[MinPhaseSettings] = None,
                    centre_samples: Optional[Sequence[int]] = None) -> MinPhaseRecords:
    """The records of every (channel, grid point) of a device batch.  The batch is cut into sub-batches of consecutive
    channels whose device scratch stays under engine.MINPHASE_SCRATCH_BYTES (engine.minphase_cut); no result depends on
    the cut.  centre_samples (one index per channel) overrides the peak / onset centre."""
    settings = settings or MinPhaseSettings()
    fs = float(sample_rate_hz)
    grid = minphase_grid(settings, fs)
    nch, npts = batch.count, int(grid.size)
    centre = _centres(eng, batch, settings, centre_samples)
    length = batch.length.astype(np.int64).copy()
    seg, n_fft = minphase_sizes(length, centre, fs, settings)
    bins = minphase_bins(grid, n_fft, fs)
    records = np.full((nch, npts, MINPHASE_FIELDS), np.nan)
    pmax, floored = np.zeros(nch), np.zeros(nch, dtype=np.int64)
    live = np.nonzero(seg > 0)[0]                                   # an empty channel is silence: nothing to transform
    for a, b in E.minphase_cut(n_fft[live]):
        idx = live[a:b]
        ch = _chain(eng, batch.x, batch.off[idx], seg[idx], n_fft[idx], fs, settings.floor_db)
        wrapped = eng.minphase_excess(ch["spec"], ch["tspec"], ch["spec_off"], ch["n32"], centre[idx], ch["pmax"])
        unwrapped = eng.phase_unwrap(wrapped, ch["spec_off"], ch["n32"], True, False, as_float64=True)
        rec = eng.minphase_gather(ch["spec"], ch["tspec"], unwrapped, ch["spec_off"], ch["n32"], bins[idx], ch["pmax"])
        records[idx] = rec.cpu().numpy().reshape(idx.size, npts, MINPHASE_FIELDS)
        pmax[idx] = ch["pmax"].cpu().numpy()[: idx.size]
        floored[idx] = ch["floored"].cpu().numpy()[: idx.size]
    return MinPhaseRecords(settings=settings, grid_hz=grid, length=length, centre=centre, segment=seg, n_fft=n_fft, bins=bins,
                           pmax=pmax, floored=floored, records=records)


def minimum_phase_device(eng, batch, sample_rate_hz: int, settings: Optional[MinPhaseSettings] = None,
                         centre_samples: Optional[Sequence[int]] = None) -> Dict:
    """The minimum-phase version of every channel, left on the device.  Returns dict(h=flat float32 device buffer, off,
    n_out, n_fft, pmax): channel e's response is h[off[e] : off[e] + n_out[e]], n_out = D; pmax[e] (host) is P, and a
    channel whose P is not a positive finite number has zeros there (silence stays silence; the host function turns a
    non-finite channel into NaN)."""
    settings = settings or MinPhaseSettings()
    fs = float(sample_rate_hz)
    centre = _centres(eng, batch, settings, centre_samples)
    seg, n_fft = minphase_sizes(batch.length, centre, fs, settings)
    off = E.exclusive_cumsum(n_fft)
    h = eng.empty(int(n_fft.sum()), eng.torch.float32)
    pmax = np.zeros(batch.count)
    if batch.count:
        h.zero_()
    live = np.nonzero(seg > 0)[0]
    for a, b in E.minphase_cut(n_fft[live]):
        idx = live[a:b]
        ch = _chain(eng, batch.x, batch.off[idx], seg[idx], n_fft[idx], fs, settings.floor_db)
        eng.minphase_spectrum(ch["g"], ch["tspec"], ch["spec_off"], ch["n32"], ch["pmax"])
        eng.band_irfft(ch["g"], ch["spec_off"], ch["n32"], ch["allpass"], ch["bin_step"], h, off[idx])
        pmax[idx] = ch["pmax"].cpu().numpy()[: idx.size]
    return dict(h=h, off=off, n_out=seg.astype(np.int32), n_fft=n_fft.astype(np.int32), pmax=pmax)


def minimum_phase_impulse_responses(channels: Sequence[np.ndarray], sample_rate_hz: int,
                                    settings: Optional[MinPhaseSettings] = None, eng=None) -> List[np.ndarray]:
    """h_min of every channel: float32 arrays of D samples each.  A channel of silence comes back as zeros, a channel with
    a NaN or an infinity in its segment as NaN."""
    settings = settings or MinPhaseSettings()
    eng = eng or E.get_engine()
    out: List[np.ndarray] = []
    for a in range(0, len(channels), MAX_BATCH_CHANNELS):
        batch = eng.upload([np.asarray(c, dtype=np.float32).reshape(-1) for c in channels[a : a + MAX_BATCH_CHANNELS]])
        dev = minimum_phase_device(eng, batch, sample_rate_hz, settings)
        host = dev["h"].cpu().numpy()
        for o, n, p in zip(dev["off"], dev["n_out"], dev["pmax"]):
            h = host[int(o) : int(o) + int(n)].astype(np.float32)
            if not (p == 0.0 or (p > 0.0 and math.isfinite(p))):
                h = np.full(int(n), np.nan, dtype=np.float32)
            out.append(h)
    return out


# ---------------------------------------------------------------------------------------------------
# host: records -> results
# ---------------------------------------------------------------------------------------------------


def wrap_phase(d):
    """wrap(d) = d - 2 pi rint(d / (2 pi)), as ira_minphase_excess forms it."""
    d = np.asarray(d, dtype=np.float64)
    return d - TWO_PI * np.rint(d / TWO_PI)


def minphase_arithmetic(records: np.ndarray, bins: np.ndarray, n_fft: int, centre: int, pmax: float, floored_bins: int,
                        sample_rate_hz: float, floor_db: float = -120.0) -> Dict:
    """The curves and the channel values of one channel from its (J, MINPHASE_FIELDS) records, its bins, N, the centre, P
    and the count of floored bins, float64 NumPy (the module's docstring states each line).  Without values (P not a
    positive finite number) everything is NaN and no bin is floored."""
    r = np.asarray(records, dtype=np.float64).reshape(-1, MINPHASE_FIELDS)
    k = np.asarray(bins, dtype=np.int64).reshape(-1)
    n, fs, p = int(n_fft), float(sample_rate_hz), int(centre)
    npts = r.shape[0]
    nan = np.full(npts, np.nan)
    freq = k.astype(np.float64) * fs / float(n)
    pmax = float(pmax)
    if not (pmax > 0.0 and math.isfinite(pmax)):
        return dict(frequencies_hz=freq, bin=k.copy(), level_db=nan, phase_deg=nan.copy(), minimum_phase_deg=nan.copy(),
                    excess_phase_deg=nan.copy(), excess_group_delay_seconds=nan.copy(), minimum_group_delay_seconds=nan.copy(),
                    floored=np.zeros(npts, dtype=bool), floored_share=math.nan, excess_delay_seconds=math.nan,
                    excess_phase_span_deg=math.nan)
    re, im, t_lo, t_mid, t_hi, e_lo, e_mid, e_hi = (r[:, q] for q in range(MINPHASE_FIELDS))
    p_floor = pmax * 10.0 ** (float(floor_db) / 10.0)
    with np.errstate(all="ignore"):
        power = re * re + im * im
        level = 10.0 * np.log10(np.maximum(power, p_floor))
        turn = ((k * p) % n).astype(np.float64) / float(n)
        phase = np.degrees(wrap_phase(np.arctan2(im, re) + TWO_PI * turn))
        step = 4.0 * math.pi / float(n)
        tau_e = -(e_hi - e_lo) / step
        tau_min = -(2.0 * t_hi - 2.0 * t_lo) / step
        weight = float(np.sum(power))
        delay = float(np.sum(power * tau_e)) / weight / fs if npts and weight > 0.0 else math.nan
        excess_deg = np.degrees(e_mid)
        span = float(np.max(excess_deg) - np.min(excess_deg)) if npts else math.nan
    return dict(frequencies_hz=freq, bin=k.copy(), level_db=level, phase_deg=phase, minimum_phase_deg=np.degrees(2.0 * t_mid),
                excess_phase_deg=excess_deg, excess_group_delay_seconds=tau_e / fs, minimum_group_delay_seconds=tau_min / fs,
                floored=power < p_floor, floored_share=float(floored_bins) / float(n // 2 + 1), excess_delay_seconds=delay,
                excess_phase_span_deg=span)


def minphase_results(res: MinPhaseRecords, sample_rate_hz: int, channel_names: Sequence[str],
                     keep_curve: bool = True) -> List["MinPhaseChannelResult"]:
    fs = float(sample_rate_hz)
    st = res.settings
    out = []
    for ch, name in enumerate(channel_names):
        v = minphase_arithmetic(res.records[ch], res.bins[ch], int(res.n_fft[ch]), int(res.centre[ch]), float(res.pmax[ch]),
                                int(res.floored[ch]), fs, st.floor_db)
        scalars = {q: v.pop(q) for q in ("floored_share", "excess_delay_seconds", "excess_phase_span_deg")}
        p = int(res.centre[ch])
        out.append(MinPhaseChannelResult(
            channel_name=str(name), sample_rate_hz=int(sample_rate_hz), centre=st.centre, centre_samples=p,
            centre_seconds=p / fs, segment_samples=int(res.segment[ch]), fft_size=int(res.n_fft[ch]), floor_db=st.floor_db,
            points_per_octave=st.points_per_octave, **scalars, **(v if keep_curve else {})))
    return out


# ---------------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------------


def _results_of_batch(eng, batch, sample_rate_hz, names, settings) -> List[MinPhaseChannelResult]:
    return minphase_results(minphase_device(eng, batch, sample_rate_hz, settings), sample_rate_hz, names)


def analyse_minphase_batch(
    channels: Sequence[np.ndarray],
    sample_rate_hz: int,
    channel_names: Sequence[str],
    settings: Optional[MinPhaseSettings] = None,
) -> List[MinPhaseChannelResult]:
    """Every channel through the device in batches of at most MAX_BATCH_CHANNELS channels."""
    return M.analyse_channel_batches(channels, sample_rate_hz, channel_names, settings or MinPhaseSettings(), _results_of_batch)


def analyse_minphase_for_channel(
    samples: np.ndarray,
    sample_rate_hz: int,
    channel_name: str,
    settings: Optional[MinPhaseSettings] = None,
) -> MinPhaseChannelResult:
    return analyse_minphase_batch([samples], sample_rate_hz, [channel_name], settings)[0]


def analyse_minphase_from_wav_file(
    input_wav_file_path: str | Path,
    settings: Optional[MinPhaseSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[MinPhaseChannelResult]:
    """One WAV file (mono or stereo, rate checked against expected_sample_rate_hz); channels named as by
    get_analysis_channels ("mono", "left", "right")."""
    return M.analyse_wav_file_channels(input_wav_file_path, settings or MinPhaseSettings(), expected_sample_rate_hz,
                                       analyse_minphase_batch)


def analyse_minphase_files(
    paths: Sequence[str | Path],
    settings: Optional[MinPhaseSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[MinPhaseChannelResult]:
    """Every channel of every file in one device batch per MAX_BATCH_CHANNELS channels; channels named
    "<file name>:<channel>"."""
    return M.analyse_file_channels(paths, settings or MinPhaseSettings(), expected_sample_rate_hz, analyse_minphase_batch)


def analyse_minphase_bundle(
    bundle_root: str | Path,
    settings: Optional[MinPhaseSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[MinPhaseChannelResult]:
    """The taps a bundle's meta.json lists (taps/<name>.wav), read by the native ingest (ingest.TapSet) a group at a
    time; channels named "<tap>:<channel>"."""
    return M.analyse_bundle_channels(bundle_root, settings or MinPhaseSettings(), expected_sample_rate_hz, _results_of_batch)


def write_minimum_phase_files(paths: Sequence[str | Path], output_dir: str | Path,
                              settings: Optional[MinPhaseSettings] = None,
                              expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> List[Path]:
    """<output_dir>/<stem>_minphase.wav per input file: the minimum-phase version of each of its channels as float32
    (the writer of deconvolve.py).  Channels of one file whose segments differ in length (post_ms) are zero-padded to the
    longest."""
    from ._common import wav_channels
    from .deconvolve import _write_wav_float32

    settings = settings or MinPhaseSettings()
    written = []
    for p in paths:
        loaded, chans = wav_channels(p, settings.use_mono_downmix_for_stereo, expected_sample_rate_hz=expected_sample_rate_hz)
        hs = minimum_phase_impulse_responses([c for _, c in chans], loaded.sample_rate_hz, settings)
        out = np.zeros((max(h.size for h in hs), len(hs)), dtype=np.float32)
        for q, h in enumerate(hs):
            out[: h.size, q] = h
        target = Path(output_dir) / f"{Path(p).stem}_minphase.wav"
        _write_wav_float32(target, loaded.sample_rate_hz, out)
        written.append(target)
    return written


# ---------------------------------------------------------------------------------------------------
# text, Markdown, JSON
# ---------------------------------------------------------------------------------------------------


def _rows(r: MinPhaseChannelResult) -> List[List[str]]:
    """One row per octave from the first grid point (every points_per_octave-th point); none without the curve."""
    if r.frequencies_hz is None:
        return []
    return [[f"{r.frequencies_hz[j]:.1f}", M.fmt(float(r.level_db[j]), 2), M.fmt(float(r.phase_deg[j]), 1),
             M.fmt(float(r.minimum_phase_deg[j]), 1), M.fmt(float(r.excess_phase_deg[j]), 1),
             M.fmt(1000.0 * float(r.excess_group_delay_seconds[j]), 3),
             M.fmt(1000.0 * float(r.minimum_group_delay_seconds[j]), 3), "yes" if r.floored[j] else "no"]
            for j in range(0, len(r.frequencies_hz), r.points_per_octave)]


def _head(r: MinPhaseChannelResult, sep: str, end: str) -> str:
    points = "NA" if r.frequencies_hz is None else str(len(r.frequencies_hz))
    return (f"Centre: {r.centre} at {r.centre_samples} samples ({1000.0 * r.centre_seconds:.3f} ms){sep}"
            f"Segment: {r.segment_samples} samples, N = {r.fft_size}{sep}Floor: {r.floor_db:g} dB{sep}"
            f"Points: {points} ({r.points_per_octave} per octave){end}")


def _tail(r: MinPhaseChannelResult, end: str) -> List[str]:
    return [f"excess delay: {M.fmt(1000.0 * r.excess_delay_seconds, 3)} ms, excess phase span: "
            f"{M.fmt(r.excess_phase_span_deg, 1)} deg, floored bins: {M.fmt(100.0 * r.floored_share, 2)} %{end}"]


_COLUMNS = ["level_dB", "phase_deg", "min_phase_deg", "excess_phase_deg", "excess_gd_ms", "min_gd_ms", "floored"]
_MD_COLUMNS = ["level (dB)", "phase (deg)", "minimum phase (deg)", "excess phase (deg)", "excess group delay (ms)",
               "minimum group delay (ms)", "floored"]


def summarise_minphase_text(channel_results: List[MinPhaseChannelResult]) -> str:
    """
    Fixed text format, one block per channel followed by an empty line:
        [<channel name>]
        Centre: <kind> at <p> samples (<p / fs in ms, 3 decimals> ms)  Segment: <D> samples, N = <N>  Floor: <dB> dB  Points: <J> (<ppo> per octave)
        freq_Hz  level_dB  phase_deg  min_phase_deg  excess_phase_deg  excess_gd_ms  min_gd_ms  floored
        <f, 1 decimal>  <2 decimals>  <1 decimal>  <1 decimal>  <1 decimal>  <3 decimals>  <3 decimals>  yes | no   (one row per octave)
        excess delay: <3 decimals> ms, excess phase span: <1 decimal> deg, floored bins: <2 decimals> %
    Cells are separated by two spaces; NaN is "NA".  Phases and delays are relative to the centre.
    """
    return M.join_blocks(M.text_block(r.channel_name, _head(r, "  ", ""), _COLUMNS, _rows(r), tail=_tail(r, ""),
                                      first="freq_Hz") for r in channel_results)


def summarise_minphase_markdown(channel_results: List[MinPhaseChannelResult]) -> str:
    """The same values as a Markdown section per channel: a '### <channel name>' heading, the centre / segment / floor /
    points line, a table with a row per octave and the channel's line."""
    return M.join_blocks(M.markdown_block(r.channel_name, _head(r, ". ", "."), _MD_COLUMNS, _rows(r), tail=_tail(r, "."),
                                          first="freq (Hz)") for r in channel_results)


_SCALARS = ("channel_name", "sample_rate_hz", "centre", "centre_samples", "centre_seconds", "segment_samples", "fft_size",
            "floor_db", "points_per_octave", "floored_share", "excess_delay_seconds", "excess_phase_span_deg")
_NAN_SCALARS = ("floored_share", "excess_delay_seconds", "excess_phase_span_deg")


def minphase_results_to_json(channel_results: List[MinPhaseChannelResult], with_curve: bool = True) -> Dict:
    """Plain JSON: NaN is null.  The curves are written for the channels that kept them unless with_curve is False."""
    rows = []
    for r in channel_results:
        d = {name: (M.json_num(float(getattr(r, name))) if name in _NAN_SCALARS else getattr(r, name)) for name in _SCALARS}
        if with_curve and r.frequencies_hz is not None:
            for name in _CURVES:
                v = getattr(r, name)
                if name == "floored":
                    d[name] = [bool(b) for b in v]
                elif name == "bin":
                    d[name] = [int(k) for k in v]
                else:
                    d[name] = [M.json_num(float(x)) for x in v]
        rows.append(d)
    return {"minimum_phase": rows}


def minphase_results_from_json(doc: Dict) -> List[MinPhaseChannelResult]:
    out = []
    for d in doc["minimum_phase"]:
        curves = {}
        if "frequencies_hz" in d:
            for name in _CURVES:
                if name == "floored":
                    curves[name] = np.asarray(d[name], dtype=bool)
                elif name == "bin":
                    curves[name] = np.asarray(d[name], dtype=np.int64)
                else:
                    curves[name] = np.asarray([M.num_json(v) for v in d[name]], dtype=np.float64)
        out.append(MinPhaseChannelResult(
            channel_name=d["channel_name"], sample_rate_hz=int(d["sample_rate_hz"]), centre=str(d["centre"]),
            centre_samples=int(d["centre_samples"]), centre_seconds=float(d["centre_seconds"]),
            segment_samples=int(d["segment_samples"]), fft_size=int(d["fft_size"]), floor_db=float(d["floor_db"]),
            points_per_octave=int(d["points_per_octave"]), floored_share=M.num_json(d["floored_share"]),
            excess_delay_seconds=M.num_json(d["excess_delay_seconds"]),
            excess_phase_span_deg=M.num_json(d["excess_phase_span_deg"]), **curves))
    return out


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.minphase",
        description="Minimum phase, excess phase and excess group delay per channel on a logarithmic grid, by the real "
                    "cepstrum of the log magnitude; optionally the minimum-phase version of every file.")
    M.add_source_arguments(p)
    p.add_argument("--oversample", type=int, default=4,
                   help="the transform is the power of two >= this many times the segment (default: 4)")
    p.add_argument("--post-ms", type=float, default=None,
                   help="keep this many milliseconds after the centre (default: the whole channel)")
    p.add_argument("--floor-db", type=float, default=-120.0,
                   help="magnitude floor under the logarithm, relative to the largest bin (default: -120 dB)")
    p.add_argument("--points-per-octave", type=int, default=48, help="grid density (default: 48)")
    p.add_argument("--f-min", type=float, default=20.0, help="first grid frequency in Hz (default: 20)")
    p.add_argument("--f-max", type=float, default=20000.0,
                   help="the grid ends at or below this frequency and the Nyquist frequency (default: 20000)")
    p.add_argument("--centre", choices=CENTRES, default="peak", help="time reference: the peak or the onset (default: peak)")
    p.add_argument("--onset-db", type=float, default=-20.0,
                   help="onset: first sample within this level of the peak (default: -20 dB, ISO 3382-1)")
    p.add_argument("--no-curve", action="store_true", help="leave the per-frequency curves out of the JSON")
    p.add_argument("--write-minimum-phase", type=Path, default=None, metavar="DIR",
                   help="also write the minimum-phase version of every input file to DIR/<stem>_minphase.wav (float32)")
    M.add_output_arguments(p)
    return p


def settings_from_args(args) -> MinPhaseSettings:
    return MinPhaseSettings(oversample=args.oversample, post_ms=args.post_ms, floor_db=args.floor_db,
                            points_per_octave=args.points_per_octave, f_min_hz=args.f_min, f_max_hz=args.f_max,
                            centre=args.centre, onset_db=args.onset_db, use_mono_downmix_for_stereo=bool(args.mono))


def main(argv: Optional[Sequence[str]] = None) -> None:
    parser = build_parser()
    args = parser.parse_args(argv)
    no_curve = bool(args.no_curve)
    M.run_cli(parser, argv, settings_from_args, analyse_minphase_files, analyse_minphase_bundle, summarise_minphase_text,
              lambda results: minphase_results_to_json(results, not no_curve))
    if args.write_minimum_phase is not None:
        if args.input:
            paths = list(args.input)
        else:
            taps = json.loads((Path(args.bundle) / "meta.json").read_text()).get("taps", [])
            paths = [Path(args.bundle) / "taps" / f"{t}.wav" for t in taps]
        write_minimum_phase_files(paths, args.write_minimum_phase, settings_from_args(args), args.expected_sample_rate)


if __name__ == "__main__":
    main()
