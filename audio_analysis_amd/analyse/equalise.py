"""
Equalisation filter design: a regularised inverse of the smoothed magnitude response as a minimum-phase FIR filter, per
channel or for the power average of several channels.  The other modules measure a response (level, phase, decay, ...);
minphase.py says what "a minimum-phase equaliser undoes".  This module computes that equaliser: the fractional-octave
smoothed power response (Hatziantoniou and Mourjopoulos), inverted with frequency-dependent regularisation (Kirkeby and
Nelson) towards a target, made minimum phase by the cepstral chain of minphase.py and cut to a tapered FIR.

Inputs: channels x_e (float32) at the sample rate fs.

  rows      a ROW is one filter.  By default one row per channel; average = True: one row for all channels of the call,
            their power spectra averaged (at most MAX_BATCH_CHANNELS channels, more is a ValueError); its members are the
            channels in the order given
  segment   D_e = L_e; with post_ms: D_e = min(L_e, p_e + 1 + rint(post_ms fs / 1000)), p_e the peak (eng.onset_index)
  size      one N per call: the power of two >= max(oversample * max_e D_e, 2 * taps, 32), oversample 2; n_fft overrides it
            (a power of two >= max D_e and >= 2 * taps); ValueError above 2^21 (deconvolve.py's MAX_LOG2_FFT), naming
            post_ms, oversample and taps as the remedies
  X^e       = rfft(x_e[:D_e], n = N), no window                                   (Engine.rfft_any, data_len = D_e)
  P_k       = (sum over the row's members, ascending from 0.0, of (re^2 + im^2)) / (double)count, float64, k = 0 .. N/2
                                                                                  (ira_eq_power)
  smoothing b (1/b octave; a whole number 0 .. 48, default 6, 0 = none):  lo_k = ceil(k 2^(-1/(2b))), hi_k = min(floor(k
            2^(1/(2b))), N/2); b = 0: lo_k = hi_k = k.  int32 host tables made in float64 NumPy (engine.equalise_windows)
  S_k       = W(lo_k, hi_k) / (double)(hi_k - lo_k + 1)                            (ira_eq_pyramid, ira_eq_smooth)
            W is the window sum over a dyadic pyramid: level 0 is P, level j + 1 has ceil(n_j / 2) entries, L_(j+1)[i] =
            L_j[2i] + L_j[2i + 1], an entry without a partner is copied.  W(lo, hi): l = lo, r = hi + 1, left = right =
            0.0, j = 0; while l < r: if l is odd left += L_j[l++]; if r is odd right += L_j[--r]; l >>= 1, r >>= 1, j++.
            W = left + right.  Every term is non-negative (no cancellation, unlike prefix sums) and the order is fixed:
            NumPy restates it bit for bit.  O(log N) per bin.
  ref       = exp(mean_j ln S_(k_j)) over the grid points f_low <= f_j <= f_high; the grid is fdw_grid's (points_per_octave
            48, f_min 20, f_max 20000), k_j = clip(rint(f_j N / fs), 1, N/2 - 1); on the host in float64 from the gathered S
            (ira_eq_gather).  A row whose ref is not a positive finite number (silence, a NaN, an infinity, no grid point in
            the band) has no values: its filter and curves are NaN, and it touches no other row
  t_k       = 10^(tilt log2(f_k / 1000) / 20), t_0 = t_1, f_k = k fs / N                    (engine.equalise_tables, float64)
  beta_k    = 10^(beta_dB / 10), beta_dB = reg_in + w (reg_out - reg_in), w = 0.5 (1 - cos pi u), u = clamp(log2(f_low / f_k)
            / transition_octaves, 0, 1) below the band, clamp(log2(f_k / f_high) / transition_octaves, 0, 1) above; w = 1 at
            k = 0.  Defaults: f_low 40, f_high 16000, transition 0.5 octave, reg_in -20 dB, reg_out +20 dB, tilt 0
  c_k       s = S_k / ref, a = sqrt(s): c_k = min((a t_k + beta_k) / (s + beta_k), 10^(max_boost_db / 20)), max_boost_db 12
            (ira_eq_invert).  Kirkeby-Nelson regularisation with the unit filter as the fallback: where beta << s it
            inverts (c -> t / a), where beta >> s (outside the band) it leaves the response alone (c -> 1), and at a deep
            notch (a -> 0) it leaves the notch alone too.  beta > 0, so c is finite for every s >= 0; without the clamp the
            largest boost at reg_in -20 dB is 14.85 dB.  The count of clamped bins per row is reported.  A row without values
            gets c = 1 (no logarithm of zero is taken); the host turns its outputs into NaN
  filter    the complex (c_k, 0) through minphase.py's chain (minphase_logmag at floor_db -300, band_irfft, rfft_any with
            data_len N/2, minphase_spectrum, band_irfft) gives g (float32, N samples);
            f[n] = float32((double)g[n] v[n]), n < taps (ira_eq_taper); taps 8192, fade 0.25;
            v = 1 up to n0 = taps - rint(fade taps), from n0 on 0.5 (1 + cos(pi (n - n0 + 1) / (taps - n0 + 1)))
  predict   F = rfft(f, n = N) (data_len = taps); A_k = P_k (Fre^2 + Fim^2); the same pyramid and windows smooth A; the result
            A_s is gathered on the grid

Per row: the name, the members, N and taps, reference_level_db = 10 log10 ref, clamped_share (clamped bins / (N/2 + 1)),
deviation_before_db and deviation_after_db (the rms over the in-band grid points of 10 log10(S / ref) - target_db, and of
10 log10(A_s / ref) - target_db) and the curves frequencies_hz (k fs / N), bin, before_db = 10 log10(S / ref), target_db =
20 log10 t, correction_db = 20 log10 c and after_db = 10 log10(A_s / ref), float64 NumPy on the host (equalise_arithmetic).

An empty channel (no samples) is silence: its row has no values; averaging refuses it.  With more than MAX_BATCH_CHANNELS
channels (no averaging) every batch of that many is a call of its own, with its own N.

The defaults are conventions of room-correction tools, not citations.

Command line (no plots): python -m analyse.equalise --input A.wav [B.wav ...] | --bundle DIR [--mono] [--average]
  [--smoothing 6] [--f-low 40] [--f-high 16000] [--transition-octaves 0.5] [--regularisation-db -20] [--outside-db 20]
  [--max-boost-db 12] [--tilt-db-per-octave 0] [--taps 8192] [--fade 0.25] [--oversample 2] [--fft-size N] [--post-ms T]
  [--points-per-octave 48] [--f-min 20] [--f-max 20000] [--no-curve] [--write-filters DIR] [--expected-sample-rate 48000]
  [--json OUT.json]
"""
from __future__ import annotations

import argparse
import json
import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _measure as M
from .. import engine as E
from ..engine import EQ_MAX_SMOOTHING, MINPHASE_MIN_FLOOR_DB, MINPHASE_MIN_N
from ._measure import MAX_BATCH_CHANNELS  # noqa: F401  (part of this module's surface)
from .deconvolve import MAX_LOG2_FFT
from .fdw import FdwSettings, fdw_grid
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ

_CURVES = ("frequencies_hz", "bin", "before_db", "target_db", "correction_db", "after_db")
AVERAGE_NAME = "average"
PEAK_REL_ENERGY = 0.01                               # eng.onset_index wants a level; the peak does not depend on it


@dataclass(frozen=True)
class EqualiseSettings:
    smoothing: int = 6                             # 1/b octave; 0: none
    f_low_hz: float = 40.0
    f_high_hz: float = 16000.0
    transition_octaves: float = 0.5
    regularisation_db: float = -20.0               # reg_in: beta inside the band
    outside_db: float = 20.0                       # reg_out: beta outside the band
    max_boost_db: float = 12.0
    tilt_db_per_octave: float = 0.0
    taps: int = 8192
    fade: float = 0.25                             # the share of the taps the cosine fade takes
    oversample: int = 2
    n_fft: Optional[int] = None                    # None: from oversample, the segments and taps
    post_ms: Optional[float] = None                # None: the whole channel
    points_per_octave: int = 48
    f_min_hz: float = 20.0
    f_max_hz: float = 20000.0                      # clipped to the Nyquist frequency
    average: bool = False
    use_mono_downmix_for_stereo: bool = False

    def __post_init__(self):
        def number(name, positive=False, lo=None, hi=None):
            try:
                v = float(getattr(self, name))
            except (TypeError, ValueError):
                raise ValueError(f"{name} must be a number, got {getattr(self, name)!r}") from None
            if not math.isfinite(v) or (positive and v <= 0.0):
                raise ValueError(f"{name} must be finite{' and > 0' if positive else ''}, got {getattr(self, name)}")
            if (lo is not None and v < lo) or (hi is not None and v > hi):
                raise ValueError(f"{name} must lie in {lo:g} .. {hi:g}, got {getattr(self, name)}")
            return v

        def whole(name, least, most=None):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least or (most is not None and v > most):
                raise ValueError(f"{name} must be a whole number >= {least}" + (f" and <= {most}" if most is not None else "")
                                 + f", got {v!r}")
            return int(v)

        vals = dict(
            smoothing=whole("smoothing", 0, EQ_MAX_SMOOTHING), taps=whole("taps", 1, 1 << (MAX_LOG2_FFT - 1)),
            oversample=whole("oversample", 1), points_per_octave=whole("points_per_octave", 1),
            f_low_hz=number("f_low_hz", True), f_high_hz=number("f_high_hz", True),
            transition_octaves=number("transition_octaves", True),
            regularisation_db=number("regularisation_db", lo=MINPHASE_MIN_FLOOR_DB, hi=-MINPHASE_MIN_FLOOR_DB),
            outside_db=number("outside_db", lo=MINPHASE_MIN_FLOOR_DB, hi=-MINPHASE_MIN_FLOOR_DB),
            max_boost_db=number("max_boost_db", lo=MINPHASE_MIN_FLOOR_DB, hi=-MINPHASE_MIN_FLOOR_DB),
            tilt_db_per_octave=number("tilt_db_per_octave", lo=-24.0, hi=24.0), fade=number("fade", lo=0.0, hi=1.0),
            f_min_hz=number("f_min_hz", True), f_max_hz=number("f_max_hz", True),
            post_ms=None if self.post_ms is None else number("post_ms"))
        if vals["post_ms"] is not None and vals["post_ms"] < 0.0:
            raise ValueError(f"post_ms must be >= 0 (or None for the whole channel), got {self.post_ms}")
        if vals["f_high_hz"] <= vals["f_low_hz"]:
            raise ValueError(f"f_high_hz must lie above f_low_hz, got {self.f_low_hz} .. {self.f_high_hz}")
        if vals["f_max_hz"] < vals["f_min_hz"]:
            raise ValueError(f"f_max_hz must be at least f_min_hz, got {self.f_min_hz} .. {self.f_max_hz}")
        if self.n_fft is not None:
            n = whole("n_fft", MINPHASE_MIN_N, 1 << MAX_LOG2_FFT)
            if n & (n - 1) or n < 2 * vals["taps"]:
                raise ValueError(f"n_fft must be a power of two >= 2 * taps = {2 * vals['taps']}, got {self.n_fft}")
            vals["n_fft"] = n
        for k, v in vals.items():
            object.__setattr__(self, k, v)
        object.__setattr__(self, "average", bool(self.average))

    @property
    def max_gain(self) -> float:
        return 10.0 ** (self.max_boost_db / 20.0)


@dataclass(frozen=True, eq=False)
class EqualiseResult:
    name: str
    members: Tuple[str, ...]
    sample_rate_hz: int
    fft_size: int                                  # N
    taps: int
    smoothing: int
    points_per_octave: int
    reference_level_db: float                      # NaN without values
    clamped_share: float
    deviation_before_db: float
    deviation_after_db: float
    # per grid point; None: not kept (a JSON written with --no-curve)
    frequencies_hz: Optional[np.ndarray] = None
    bin: Optional[np.ndarray] = None               # int64
    before_db: Optional[np.ndarray] = None
    target_db: Optional[np.ndarray] = None
    correction_db: Optional[np.ndarray] = None
    after_db: Optional[np.ndarray] = None


@dataclass
class EqualiseRecords:
    """What equalise_device leaves: the filters on the device and, on the host, the grid, the rows and per (row, grid point)
    S, c and the smoothed prediction A_s."""
    settings: EqualiseSettings
    grid_hz: np.ndarray                            # float64 (J,)
    bins: np.ndarray                               # int64 (J,)
    in_band: np.ndarray                            # bool (J,)
    target: np.ndarray                             # float64 (J,): t at the bins
    n_fft: int
    segment: np.ndarray                            # int64 (nch,): D
    rows: List[List[int]]                          # the member channels of every row
    ref: np.ndarray                                # float64 (rows,); NaN for a row of empty channels
    clamped: np.ndarray                            # int64 (rows,)
    s_grid: np.ndarray                             # float64 (rows, J)
    c_grid: np.ndarray
    a_grid: np.ndarray
    filters: "object"                              # torch.float32 (rows, taps) on the device
    kept: List[Dict] = field(default_factory=list)  # keep = True: per sub-batch the device arrays (tests)


def equalise_grid(settings: EqualiseSettings, sample_rate_hz: float) -> np.ndarray:
    """The grid frequencies f_j: fdw_grid's, f_min 2^(j / ppo) while f_j <= min(f_max, fs / 2)."""
    return fdw_grid(FdwSettings(points_per_octave=settings.points_per_octave, f_min_hz=settings.f_min_hz,
                                f_max_hz=settings.f_max_hz), sample_rate_hz)[0]


def equalise_bins(grid_hz: np.ndarray, n_fft: int, sample_rate_hz: float) -> np.ndarray:
    """k_j = clip(rint(f_j N / fs), 1, N/2 - 1): int64 (J,)."""
    k = np.rint(np.asarray(grid_hz, dtype=np.float64) * float(n_fft) / float(sample_rate_hz))
    return np.clip(k, 1, int(n_fft) // 2 - 1).astype(np.int64)


def equalise_sizes(length, centre, sample_rate_hz: float, settings: EqualiseSettings) -> Tuple[np.ndarray, int]:
    """(D per channel int64, N): the module docstring's segment and size lines.  ValueError where N would exceed 2^21 or a
    given n_fft is shorter than a segment."""
    length = np.asarray(length, dtype=np.int64).reshape(-1)
    if settings.post_ms is None:
        seg = length.copy()
    else:
        centre = np.asarray(centre, dtype=np.int64).reshape(-1)
        seg = np.minimum(length, centre + 1 + int(np.rint(settings.post_ms * float(sample_rate_hz) / 1000.0)))
    seg = np.maximum(seg, 0)
    longest = int(seg.max()) if seg.size else 0
    if settings.n_fft is not None:
        if settings.n_fft < longest:
            raise ValueError(f"n_fft {settings.n_fft} is shorter than a segment of {longest} samples: raise it or set post_ms")
        return seg, int(settings.n_fft)
    need = max(settings.oversample * longest, 2 * settings.taps, MINPHASE_MIN_N)
    n = 1 << (need - 1).bit_length()
    if n > 1 << MAX_LOG2_FFT:
        raise ValueError(f"a segment of {longest} samples at oversample {settings.oversample} with {settings.taps} taps needs a "
                         f"transform of {n} points, at most 2^{MAX_LOG2_FFT}: set post_ms, or lower oversample or taps")
    return seg, n


def reference_level(s_grid: np.ndarray, in_band: np.ndarray) -> float:
    """ref = exp(mean ln S) over the in-band grid points, float64; NaN where there is none, whatever S holds otherwise."""
    s = np.asarray(s_grid, dtype=np.float64)[np.asarray(in_band, dtype=bool)]
    if s.size == 0:
        return math.nan
    with np.errstate(all="ignore"):
        return float(np.exp(np.mean(np.log(s))))


def has_values(ref: float) -> bool:
    return bool(ref > 0.0 and math.isfinite(ref))


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def _rows_of(nch: int, seg: np.ndarray, settings: EqualiseSettings) -> List[List[int]]:
    if not settings.average:
        return [[e] for e in range(nch)]
    if nch > MAX_BATCH_CHANNELS:
        raise ValueError(f"an average holds at most {MAX_BATCH_CHANNELS} channels, got {nch}")
    if nch and int(seg.min()) < 1:
        raise ValueError("an empty channel cannot be averaged")
    return [list(range(nch))] if nch else []


def equalise_device(eng, batch, sample_rate_hz: int, settings: Optional[EqualiseSettings] = None,
                    keep: bool = False) -> EqualiseRecords:
    """The filters of a device batch, left on the device (records.filters, float32 (rows, taps); a row without values holds
    the unit filter there, equalisation_filters turns it into NaN), and the per-row records on the host.  The rows are cut
    into sub-batches of whole rows whose device scratch stays under engine.EQ_SCRATCH_BYTES (engine.equalise_cut); no
    result depends on the cut.  keep: also keep every sub-batch's device arrays (X, S, c, F, A_s; for tests)."""
    settings = settings or EqualiseSettings()
    t = eng.torch
    fs = float(sample_rate_hz)
    nch = batch.count
    length = batch.length.astype(np.int64).copy()
    centre = None
    if settings.post_ms is not None and nch:
        centre = eng.onset_index(batch, PEAK_REL_ENERGY)[1].cpu().numpy().astype(np.int64)[:nch]
    seg, n = equalise_sizes(length, centre, fs, settings)
    taps = settings.taps
    if 2 * taps > n:
        raise ValueError(f"n_fft {n} must be at least 2 * taps = {2 * taps}")
    nbins = n // 2 + 1
    grid = equalise_grid(settings, fs)
    bins = equalise_bins(grid, n, fs)
    in_band = (grid >= settings.f_low_hz) & (grid <= settings.f_high_hz)
    npts = int(grid.size)
    rows = _rows_of(nch, seg, settings)
    nrows = len(rows)
    lo, hi = E.equalise_windows(n, settings.smoothing)
    target, beta = E.equalise_tables(n, fs, settings.f_low_hz, settings.f_high_hz, settings.transition_octaves,
                                     settings.regularisation_db, settings.outside_db, settings.tilt_db_per_octave)
    taper = E.equalise_taper(taps, settings.fade)
    rec = EqualiseRecords(settings=settings, grid_hz=grid, bins=bins, in_band=in_band, target=target[bins], n_fft=n, segment=seg,
                          rows=rows, ref=np.full(nrows, np.nan), clamped=np.zeros(nrows, dtype=np.int64),
                          s_grid=np.full((nrows, npts), np.nan), c_grid=np.full((nrows, npts), np.nan),
                          a_grid=np.full((nrows, npts), np.nan), filters=eng.out_view(t.float32, nrows, taps))
    if nrows:
        rec.filters.zero_()
        rec.filters[:, 0] = 1.0                                       # a row that never reaches the device: the unit filter
    live = np.array([r for r in range(nrows) if all(seg[e] > 0 for e in rows[r])], dtype=np.int64)
    n32 = lambda count: np.full(count, n, dtype=np.int32)
    for a, b in E.equalise_cut(n, [len(rows[r]) for r in live]):
        idx = live[a:b]
        chans = np.array([e for r in idx for e in rows[r]], dtype=np.int64)
        members, pos = [], 0
        for r in idx:
            members.append(list(range(pos, pos + len(rows[r]))))
            pos += len(rows[r])
        nr = int(idx.size)
        spec, spec_off = eng.rfft_any(batch.x, batch.off[chans], n32(chans.size), False, data_len=seg[chans].astype(np.int32),
                                      win_len=n32(chans.size))
        pyr = eng.eq_power(spec, spec_off, members, n)
        eng.eq_pyramid(pyr, n)
        s_dev = eng.eq_smooth(pyr, lo, hi, n)
        s_off = np.arange(nr, dtype=np.int64) * nbins
        s_grid = eng.eq_gather(s_dev, s_off, 1, bins, n).cpu().numpy().reshape(nr, npts)           # the one fetch before ref
        ref = np.array([reference_level(s_grid[q], in_band) for q in range(nr)], dtype=np.float64)
        c_dev, clamped = eng.eq_invert(s_dev, ref, target, beta, settings.max_gain, s_off, n)
        c_grid = eng.eq_gather(c_dev, 2 * s_off, 2, bins, n)
        kept = dict(rows=idx.copy(), channels=chans, members=members, spec=spec, spec_off=spec_off, s=s_dev, ref=ref) if keep else None
        if keep:
            kept["c"] = c_dev.clone()
        # (c, 0) -> G -> cepstrum -> T -> M -> g: the chain of minphase.py, every row at N
        g_spec, pmax, _ = eng.minphase_logmag(c_dev, s_off, n32(nr), MINPHASE_MIN_FLOOR_DB)
        allpass = np.zeros((nr, 8), dtype=np.float64)
        allpass[:, 0], allpass[:, 1], allpass[:, 2] = 2.0, -1.0, -1.0
        bin_step = np.full(nr, fs / float(n))
        t_off = np.arange(nr, dtype=np.int64) * n
        cep = eng.empty(nr * n, t.float32)
        eng.band_irfft(g_spec, s_off, n32(nr), allpass, bin_step, cep, t_off)
        tspec, tspec_off = eng.rfft_any(cep, t_off, n32(nr), False, data_len=n32(nr) // 2, win_len=n32(nr))
        assert np.array_equal(tspec_off, s_off)
        eng.minphase_spectrum(g_spec, tspec, s_off, n32(nr), pmax)
        eng.band_irfft(g_spec, s_off, n32(nr), allpass, bin_step, cep, t_off)                       # g, in place of the cepstrum
        f_dev = eng.eq_taper(cep, t_off, taper, n)
        # the prediction: what the filter leaves of the smoothed response
        fspec, fspec_off = eng.rfft_any(f_dev.reshape(-1), np.arange(nr, dtype=np.int64) * taps, n32(nr), False,
                                        data_len=np.full(nr, taps, dtype=np.int32), win_len=n32(nr))
        eng.eq_power(spec, spec_off, members, n, spec2_dev=fspec, spec2_off=fspec_off, pyr=pyr)
        eng.eq_pyramid(pyr, n)
        a_dev = eng.eq_smooth(pyr, lo, hi, n)
        a_grid = eng.eq_gather(a_dev, s_off, 1, bins, n)
        rec.filters[t.as_tensor(idx, device=rec.filters.device)] = f_dev
        rec.ref[idx], rec.s_grid[idx] = ref, s_grid
        rec.c_grid[idx] = c_grid.cpu().numpy().reshape(nr, npts)
        rec.a_grid[idx] = a_grid.cpu().numpy().reshape(nr, npts)
        rec.clamped[idx] = clamped.cpu().numpy()[:nr]
        if keep:
            kept.update(fspec=fspec, fspec_off=fspec_off, a=a_dev, f=f_dev, c_off=s_off)
            rec.kept.append(kept)
    return rec


def equalisation_filters(channels: Sequence[np.ndarray], sample_rate_hz: int, settings: Optional[EqualiseSettings] = None,
                         eng=None) -> List[np.ndarray]:
    """The filter of every row: float32 arrays of taps samples, one per channel (or one in all with average).  A row without
    values (silence, a NaN or an infinity among its samples, no grid point in the band) comes back as NaN."""
    settings = settings or EqualiseSettings()
    eng = eng or E.get_engine()
    if settings.average and len(channels) > MAX_BATCH_CHANNELS:
        raise ValueError(f"an average holds at most {MAX_BATCH_CHANNELS} channels, got {len(channels)}")
    out: List[np.ndarray] = []
    for a in range(0, len(channels), MAX_BATCH_CHANNELS):
        batch = eng.upload([np.asarray(c, dtype=np.float32).reshape(-1) for c in channels[a : a + MAX_BATCH_CHANNELS]])
        rec = equalise_device(eng, batch, sample_rate_hz, settings)
        host = rec.filters.cpu().numpy().reshape(len(rec.rows), settings.taps)
        for r in range(len(rec.rows)):
            out.append(host[r].astype(np.float32) if has_values(float(rec.ref[r]))
                       else np.full(settings.taps, np.nan, dtype=np.float32))
    return out


# ---------------------------------------------------------------------------------------------------
# host: records -> results
# ---------------------------------------------------------------------------------------------------


def equalise_arithmetic(s_grid: np.ndarray, c_grid: np.ndarray, a_grid: np.ndarray, target: np.ndarray, bins: np.ndarray,
                        in_band: np.ndarray, n_fft: int, ref: float, clamped_bins: int, sample_rate_hz: float) -> Dict:
    """The curves and the row values from the gathered S, c and A_s, the target at the bins, the bins, the in-band flags, N,
    ref and the count of clamped bins, float64 NumPy (the module's docstring states each line).  Without values (ref not a
    positive finite number) everything but the frequencies, the bins and the target is NaN."""
    k = np.asarray(bins, dtype=np.int64).reshape(-1)
    n, fs = int(n_fft), float(sample_rate_hz)
    freq = k.astype(np.float64) * fs / float(n)
    with np.errstate(all="ignore"):
        target_db = 20.0 * np.log10(np.asarray(target, dtype=np.float64).reshape(-1))
    nan = np.full(k.size, np.nan)
    if not has_values(float(ref)):
        return dict(frequencies_hz=freq, bin=k.copy(), before_db=nan, target_db=target_db, correction_db=nan.copy(),
                    after_db=nan.copy(), reference_level_db=math.nan, clamped_share=math.nan, deviation_before_db=math.nan,
                    deviation_after_db=math.nan)
    band = np.asarray(in_band, dtype=bool).reshape(-1)
    with np.errstate(all="ignore"):
        before = 10.0 * np.log10(np.asarray(s_grid, dtype=np.float64).reshape(-1) / float(ref))
        after = 10.0 * np.log10(np.asarray(a_grid, dtype=np.float64).reshape(-1) / float(ref))
        correction = 20.0 * np.log10(np.asarray(c_grid, dtype=np.float64).reshape(-1))
        dev_before = float(np.sqrt(np.mean((before[band] - target_db[band]) ** 2)))
        dev_after = float(np.sqrt(np.mean((after[band] - target_db[band]) ** 2)))
    return dict(frequencies_hz=freq, bin=k.copy(), before_db=before, target_db=target_db, correction_db=correction,
                after_db=after, reference_level_db=10.0 * math.log10(float(ref)),
                clamped_share=float(clamped_bins) / float(n // 2 + 1), deviation_before_db=dev_before,
                deviation_after_db=dev_after)


def equalise_results(rec: EqualiseRecords, sample_rate_hz: int, channel_names: Sequence[str],
                     keep_curve: bool = True) -> List[EqualiseResult]:
    st = rec.settings
    out = []
    for r, members in enumerate(rec.rows):
        v = equalise_arithmetic(rec.s_grid[r], rec.c_grid[r], rec.a_grid[r], rec.target, rec.bins, rec.in_band, rec.n_fft,
                                float(rec.ref[r]), int(rec.clamped[r]), float(sample_rate_hz))
        scalars = {q: v.pop(q) for q in ("reference_level_db", "clamped_share", "deviation_before_db", "deviation_after_db")}
        out.append(EqualiseResult(
            name=AVERAGE_NAME if st.average else str(channel_names[members[0]]),
            members=tuple(str(channel_names[e]) for e in members), sample_rate_hz=int(sample_rate_hz), fft_size=rec.n_fft,
            taps=st.taps, smoothing=st.smoothing, points_per_octave=st.points_per_octave, **scalars,
            **(v if keep_curve else {})))
    return out


# ---------------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------------


def _results_of_batch(eng, batch, sample_rate_hz, names, settings) -> List[EqualiseResult]:
    return equalise_results(equalise_device(eng, batch, sample_rate_hz, settings), sample_rate_hz, names)


def analyse_equalise_batch(
    channels: Sequence[np.ndarray],
    sample_rate_hz: int,
    channel_names: Sequence[str],
    settings: Optional[EqualiseSettings] = None,
) -> List[EqualiseResult]:
    """Every channel through the device in batches of at most MAX_BATCH_CHANNELS channels: one row per channel, or with
    average one row in all (at most MAX_BATCH_CHANNELS channels)."""
    settings = settings or EqualiseSettings()
    if settings.average and len(channels) > MAX_BATCH_CHANNELS:
        raise ValueError(f"an average holds at most {MAX_BATCH_CHANNELS} channels, got {len(channels)}")
    return M.analyse_channel_batches(channels, sample_rate_hz, channel_names, settings, _results_of_batch)


def analyse_equalise_files(
    paths: Sequence[str | Path],
    settings: Optional[EqualiseSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[EqualiseResult]:
    """Every channel of every file; channels named "<file name>:<channel>"."""
    return M.analyse_file_channels(paths, settings or EqualiseSettings(), expected_sample_rate_hz, analyse_equalise_batch)


def analyse_equalise_bundle(
    bundle_root: str | Path,
    settings: Optional[EqualiseSettings] = None,
    expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
) -> List[EqualiseResult]:
    """The taps a bundle's meta.json lists (taps/<name>.wav), read by the native ingest a group at a time; channels named
    "<tap>:<channel>".  With average every group of taps (MAX_BATCH_CHANNELS // 2 of them) is a row."""
    return M.analyse_bundle_channels(bundle_root, settings or EqualiseSettings(), expected_sample_rate_hz, _results_of_batch)


def write_filter_files(paths: Sequence[str | Path], output_dir: str | Path, settings: Optional[EqualiseSettings] = None,
                       expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> List[Path]:
    """<output_dir>/<stem>_eq.wav per input file, one channel per row of that file, float32 (the writer of deconvolve.py);
    with average one mono file <output_dir>/average_eq.wav.  The channels of all files go through the device as
    analyse_equalise_files sends them, so the files hold the filters whose curves it reports."""
    from ._common import wav_channels
    from .deconvolve import _write_wav_float32

    settings = settings or EqualiseSettings()
    chans, counts, rate = [], [], int(expected_sample_rate_hz)
    for p in paths:
        loaded, cs = wav_channels(p, settings.use_mono_downmix_for_stereo, expected_sample_rate_hz=expected_sample_rate_hz)
        rate = loaded.sample_rate_hz
        chans += [c for _, c in cs]
        counts.append(len(cs))
    filters = equalisation_filters(chans, rate, settings)
    written = []
    if settings.average:
        target = Path(output_dir) / f"{AVERAGE_NAME}_eq.wav"
        _write_wav_float32(target, rate, np.stack(filters, axis=1))
        return [target]
    pos = 0
    for p, count in zip(paths, counts):
        target = Path(output_dir) / f"{Path(p).stem}_eq.wav"
        _write_wav_float32(target, rate, np.stack(filters[pos : pos + count], axis=1))
        written.append(target)
        pos += count
    return written


# ---------------------------------------------------------------------------------------------------
# text, Markdown, JSON
# ---------------------------------------------------------------------------------------------------


def _rows(r: EqualiseResult) -> List[List[str]]:
    """One row per octave from the first grid point (every points_per_octave-th point); none without the curve."""
    if r.frequencies_hz is None:
        return []
    return [[f"{r.frequencies_hz[j]:.1f}", M.fmt(float(r.before_db[j]), 2), M.fmt(float(r.target_db[j]), 2),
             M.fmt(float(r.correction_db[j]), 2), M.fmt(float(r.after_db[j]), 2)]
            for j in range(0, len(r.frequencies_hz), r.points_per_octave)]


def _head(r: EqualiseResult, sep: str, end: str) -> str:
    points = "NA" if r.frequencies_hz is None else str(len(r.frequencies_hz))
    smoothing = "none" if r.smoothing == 0 else f"1/{r.smoothing} octave"
    return (f"Members: {len(r.members)}{sep}N = {r.fft_size}, {r.taps} taps{sep}Smoothing: {smoothing}{sep}"
            f"Reference level: {M.fmt(r.reference_level_db, 2)} dB{sep}Points: {points} ({r.points_per_octave} per octave){end}")


def _tail(r: EqualiseResult, end: str) -> List[str]:
    return [f"deviation from the target: {M.fmt(r.deviation_before_db, 2)} dB before, {M.fmt(r.deviation_after_db, 2)} dB "
            f"after, clamped bins: {M.fmt(100.0 * r.clamped_share, 2)} %{end}"]


_COLUMNS = ["before_dB", "target_dB", "correction_dB", "after_dB"]
_MD_COLUMNS = ["before (dB)", "target (dB)", "correction (dB)", "after (dB)"]


def summarise_equalise_text(results: List[EqualiseResult]) -> str:
    """
    Fixed text format, one block per row followed by an empty line:
        [<row name>]
        Members: <count>  N = <N>, <taps> taps  Smoothing: 1/<b> octave | none  Reference level: <2 decimals> dB  Points: <J> (<ppo> per octave)
        freq_Hz  before_dB  target_dB  correction_dB  after_dB
        <f, 1 decimal>  <2 decimals>  <2 decimals>  <2 decimals>  <2 decimals>          (one row per octave)
        deviation from the target: <2 decimals> dB before, <2 decimals> dB after, clamped bins: <2 decimals> %
    Cells are separated by two spaces; NaN is "NA".  Levels are relative to the reference level.
    """
    return M.join_blocks(M.text_block(r.name, _head(r, "  ", ""), _COLUMNS, _rows(r), tail=_tail(r, ""), first="freq_Hz")
                         for r in results)


def summarise_equalise_markdown(results: List[EqualiseResult]) -> str:
    """The same values as a Markdown section per row: a '### <row name>' heading, the head line, a table with a row per
    octave and the row's line."""
    return M.join_blocks(M.markdown_block(r.name, _head(r, ". ", "."), _MD_COLUMNS, _rows(r), tail=_tail(r, "."),
                                          first="freq (Hz)") for r in results)


_SCALARS = ("name", "members", "sample_rate_hz", "fft_size", "taps", "smoothing", "points_per_octave", "reference_level_db",
            "clamped_share", "deviation_before_db", "deviation_after_db")
_NAN_SCALARS = ("reference_level_db", "clamped_share", "deviation_before_db", "deviation_after_db")


def equalise_results_to_json(results: List[EqualiseResult], with_curve: bool = True) -> Dict:
    """Plain JSON: NaN is null.  The curves are written for the rows that kept them unless with_curve is False."""
    rows = []
    for r in results:
        d = {}
        for name in _SCALARS:
            v = getattr(r, name)
            d[name] = M.json_num(float(v)) if name in _NAN_SCALARS else (list(v) if name == "members" else v)
        if with_curve and r.frequencies_hz is not None:
            for name in _CURVES:
                v = getattr(r, name)
                d[name] = [int(k) for k in v] if name == "bin" else [M.json_num(float(x)) for x in v]
        rows.append(d)
    return {"equalisation": rows}


def equalise_results_from_json(doc: Dict) -> List[EqualiseResult]:
    out = []
    for d in doc["equalisation"]:
        curves = {}
        if "frequencies_hz" in d:
            for name in _CURVES:
                curves[name] = (np.asarray(d[name], dtype=np.int64) if name == "bin"
                                else np.asarray([M.num_json(v) for v in d[name]], dtype=np.float64))
        out.append(EqualiseResult(
            name=d["name"], members=tuple(d["members"]), sample_rate_hz=int(d["sample_rate_hz"]), fft_size=int(d["fft_size"]),
            taps=int(d["taps"]), smoothing=int(d["smoothing"]), points_per_octave=int(d["points_per_octave"]),
            **{q: M.num_json(d[q]) for q in _NAN_SCALARS}, **curves))
    return out


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.equalise",
        description="Equalisation filter design: the regularised inverse of the fractional-octave smoothed response as a "
                    "minimum-phase FIR filter per channel (or for the power average of all channels), with the predicted "
                    "response after correction.")
    M.add_source_arguments(p)
    p.add_argument("--average", action="store_true", help="one filter for the power average of all channels")
    p.add_argument("--smoothing", type=int, default=6, help="1/b octave smoothing, b = 0 .. 48, 0 = none (default: 6)")
    p.add_argument("--f-low", type=float, default=40.0, help="lower edge of the corrected band in Hz (default: 40)")
    p.add_argument("--f-high", type=float, default=16000.0, help="upper edge of the corrected band in Hz (default: 16000)")
    p.add_argument("--transition-octaves", type=float, default=0.5,
                   help="width of the regularisation's transition outside each edge (default: 0.5 octave)")
    p.add_argument("--regularisation-db", type=float, default=-20.0, help="regularisation inside the band (default: -20 dB)")
    p.add_argument("--outside-db", type=float, default=20.0, help="regularisation outside the band (default: +20 dB)")
    p.add_argument("--max-boost-db", type=float, default=12.0, help="the correction never exceeds this gain (default: 12 dB)")
    p.add_argument("--tilt-db-per-octave", type=float, default=0.0, help="slope of the target around 1 kHz (default: 0)")
    p.add_argument("--taps", type=int, default=8192, help="length of the filter in samples (default: 8192)")
    p.add_argument("--fade", type=float, default=0.25, help="share of the taps the cosine fade-out takes (default: 0.25)")
    p.add_argument("--oversample", type=int, default=2,
                   help="the transform is the power of two >= this many times the longest segment (default: 2)")
    p.add_argument("--fft-size", type=int, default=None, metavar="N", help="the transform size, a power of two (default: derived)")
    p.add_argument("--post-ms", type=float, default=None,
                   help="keep this many milliseconds after the peak (default: the whole channel)")
    p.add_argument("--points-per-octave", type=int, default=48, help="grid density (default: 48)")
    p.add_argument("--f-min", type=float, default=20.0, help="first grid frequency in Hz (default: 20)")
    p.add_argument("--f-max", type=float, default=20000.0,
                   help="the grid ends at or below this frequency and the Nyquist frequency (default: 20000)")
    p.add_argument("--no-curve", action="store_true", help="leave the per-frequency curves out of the JSON")
    p.add_argument("--write-filters", type=Path, default=None, metavar="DIR",
                   help="also write the filters to DIR/<stem>_eq.wav (float32, one channel per row; average_eq.wav with --average)")
    M.add_output_arguments(p)
    return p


def settings_from_args(args) -> EqualiseSettings:
    return EqualiseSettings(smoothing=args.smoothing, f_low_hz=args.f_low, f_high_hz=args.f_high,
                            transition_octaves=args.transition_octaves, regularisation_db=args.regularisation_db,
                            outside_db=args.outside_db, max_boost_db=args.max_boost_db,
                            tilt_db_per_octave=args.tilt_db_per_octave, taps=args.taps, fade=args.fade,
                            oversample=args.oversample, n_fft=args.fft_size, post_ms=args.post_ms,
                            points_per_octave=args.points_per_octave, f_min_hz=args.f_min, f_max_hz=args.f_max,
                            average=bool(args.average), use_mono_downmix_for_stereo=bool(args.mono))


def main(argv: Optional[Sequence[str]] = None) -> None:
    parser = build_parser()
    args = parser.parse_args(argv)
    no_curve = bool(args.no_curve)
    M.run_cli(parser, argv, settings_from_args, analyse_equalise_files, analyse_equalise_bundle, summarise_equalise_text,
              lambda results: equalise_results_to_json(results, not no_curve))
    if args.write_filters is not None:
        if args.input:
            paths = list(args.input)
        else:
            taps = json.loads((Path(args.bundle) / "meta.json").read_text()).get("taps", [])
            paths = [Path(args.bundle) / "taps" / f"{t}.wav" for t in taps]
        write_filter_files(paths, args.write_filters, settings_from_args(args), args.expected_sample_rate)


if __name__ == "__main__":
    main()
