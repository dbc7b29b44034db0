"""
The measure launchers of the device engine, one method per library call (or short chain of calls): ISO 3382-1 energy
parameters and IACC, Lundeby, multi-slope fits, STI sums, harmonics, the echo criterion, echo density, reflections,
transfer functions, the energy decay relief, FDW, burst decay, minimum phase, equalisation, MLS measurement, and the
suffix-energy tables.  Each checks its
tables on the host (engine_geometry holds what several share), allocates its outputs, uploads its job tables in one copy
and enqueues the call.  MeasureLaunchers is a base class of engine.Engine, which supplies the plumbing (empty, out_view,
job_tables, ...).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import TYPE_CHECKING, Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import check, ptr as _ptr
from .engine_geometry import *  # noqa: F401,F403  (the constants, the geometry and the table checks)
from .engine_plan import exclusive_cumsum
if TYPE_CHECKING:
    from .engine import ChannelBatch


@dataclass
class BurstTable:
    """What Engine.burst_table leaves on the device for Engine.burst_decay: the wavelets of every point, one after the
    other, and the tables the map kernel reads beside them."""
    rho: np.ndarray              # float64 (J,) host
    half: np.ndarray             # int32 (J,) host
    window: str
    offsets: np.ndarray          # int64 (J,) host: burst_table_offsets(half)
    doubles: int                 # burst_table_doubles(half)
    table: "object"              # torch.float64 (doubles,) on device: (re, im) per entry
    half_dev: "object"
    offsets_dev: "object"


class MeasureLaunchers:
    # ------------------------------------------------------------------ ISO 3382-1 energy parameters
    def onset_index(self, b: ChannelBatch, rel_energy: float):
        """ISO 3382-1 onset per channel: the first n <= peak with x[n]^2 >= x[peak]^2 * rel_energy (float64 compare).  The
        peak pick and the search both run on the device (ira_peak_index -> ira_onset_index): nothing returns to the host.
        Returns (onset int64 device (B,), peak int64 device (B,), |x[peak]| float32 device (B,))."""
        t = self.torch
        n = b.count
        pk, pa = self._batch_peak_pick(b)
        on = self.empty(n, t.int64)
        max_len = int(b.length.max()) if n else 0
        check(self.lib.ira_onset_index(_ptr(b.x), _ptr(b.off_dev), _ptr(b.len_dev), n, max_len, _ptr(pk), _ptr(pa),
                                       float(rel_energy), _ptr(on), self.stream), "ira_onset_index")
        return on[:n], pk[:n], pa[:n]

    def energy_windows(self, x_dev, base_off: np.ndarray, base_len: np.ndarray, chan_of_seg: np.ndarray, onset_dev,
                       limits: np.ndarray):
        """Windowed float64 energy sums (ira_energy_windows).  Segment j: base_len[j] - o samples from base_off[j] + o of
        x_dev, o = onset_dev[chan_of_seg[j]]; limits (nseg, nlim) int64 ascending sample counts from the segment's start.
        Returns (nseg, nlim + 2) float64 device: P_0 .. P_nlim (energy between consecutive limits, the last one up to the
        segment's end), S1 = sum n x[n]^2."""
        t = self.torch
        base_off, base_len, chan_of_seg = segment_tables(base_off, base_len, chan_of_seg)
        nseg = int(base_off.size)
        limits = np.ascontiguousarray(limits, dtype=np.int64)
        if limits.ndim != 2 or limits.shape[0] != nseg:
            raise ValueError("limits must be (nseg, nlim)")
        nlim = int(limits.shape[1])
        max_len = int(base_len.max()) if nseg else 0
        scratch = self._scratch("ira_energy_scratch_doubles", nseg, max_len, nlim)
        out = self.out_view(t.float64, nseg, nlim + 2)
        d_off, d_len, d_ch, d_lim = self.job_tables(base_off, base_len, chan_of_seg, limits.reshape(-1))
        check(self.lib.ira_energy_windows(_ptr(x_dev), _ptr(d_off), _ptr(d_len), _ptr(d_ch), _ptr(onset_dev), nseg,
                                          max_len, _ptr(d_lim), nlim, _ptr(scratch), _ptr(out), self.stream),
              "ira_energy_windows")
        return out

    # ------------------------------------------------------------------ Dietsch-Kraak echo criterion
    # A/B: True lets the first sample pass of ira_echo_criterion leave s = |y|^n behind as float64 for the second pass to
    # read back (8 bytes written and 16 read per sample) instead of forming it again (both times); the
    # results are the same to the bit.
    echo_stash = False

    def echo_criterion(self, x_dev, base_off: np.ndarray, base_len: np.ndarray, chan_of_seg: np.ndarray, onset_dev,
                       params: np.ndarray, param_of_seg: np.ndarray):
        """Echo criterion records and curves (ira_echo_criterion).  Segment j: the samples from base_off[j] + o of x_dev,
        o = onset_dev[chan_of_seg[j]], L = base_len[j] - o; its parameters are row param_of_seg[j] of params (nparam, 8)
        float64: exponent n, D, G, Mmax, S (samples per curve step, 0 = none), threshold_10, threshold_50, fs.
        Returns (records (nseg, 8) float64 device: EK_max, its first index, the first indices at or above the two
        thresholds (-1 = none), ts[M-1], W[M-1], M, V[M-1]; curve (nseg, ncurve) float32 device: the maximum of EK per
        step, NaN past a segment's range, ncurve = 0 when no row asks for a curve)."""
        t = self.torch
        base_off, base_len, chan_of_seg = segment_tables(base_off, base_len, chan_of_seg)
        param_of_seg = flat(param_of_seg, np.int32)
        params = np.ascontiguousarray(params, dtype=np.float64)
        nseg = int(base_off.size)
        if params.ndim != 2 or params.shape[1] != ECHO_PARAM_DOUBLES or not 1 <= params.shape[0] <= ECHO_MAX_PARAMS:
            raise ValueError(f"params must be (1..{ECHO_MAX_PARAMS}, {ECHO_PARAM_DOUBLES})")
        same_rows("base_off, base_len, chan_of_seg and param_of_seg must be (nseg,)", base_off, base_len, chan_of_seg,
                  param_of_seg)
        if nseg and (param_of_seg.min() < 0 or param_of_seg.max() >= params.shape[0]):
            raise ValueError("param_of_seg must index params")
        # M <= min(base_len - G, Mmax) whatever the onset: this bound sizes the grid, the scratch and the curve
        with np.errstate(invalid="ignore"):
            m_up = np.clip(np.minimum(base_len - params[param_of_seg, 2], params[param_of_seg, 3]), 0, None) if nseg else np.zeros(0)
            step = params[param_of_seg, 4] if nseg else np.zeros(0)
            steps = np.where(step > 0, np.ceil(m_up / np.where(step > 0, step, 1.0)), 0.0)
        max_len = int(np.nan_to_num(m_up).max()) if nseg else 0
        ncurve = int(np.nan_to_num(steps).max()) if nseg else 0
        scratch = self._scratch("ira_echo_scratch_doubles", nseg, max_len)
        stash = self.empty(nseg * (-(-max_len // ECHO_CHUNK)) * ECHO_CHUNK, t.float64) if self.echo_stash else None
        rec = self.out_view(t.float64, nseg, ECHO_DOUBLES)
        curve = self.out_view(t.float32, nseg, ncurve)
        d_off, d_len, d_ch, d_par = self.job_tables(base_off, base_len, chan_of_seg, param_of_seg)
        with self.tagged("[stash]" if self.echo_stash else self.event_tag):
            check(self.lib.ira_echo_criterion(_ptr(x_dev), _ptr(d_off), _ptr(d_len), _ptr(d_ch), _ptr(d_par),
                                              _ptr(onset_dev), nseg, max_len, _lib.dbl_array(params.reshape(-1)),
                                              int(params.shape[0]), ncurve, _ptr(scratch),
                                              _ptr(stash), _ptr(rec), _ptr(curve), self.stream), "ira_echo_criterion")
        return rec, curve

    # ------------------------------------------------------------------ normalized echo density (Abel & Huang)
    def echo_density(self, x_dev, off: np.ndarray, length: np.ndarray, onset_dev, weights: np.ndarray, delta: int,
                     step: int, kmax: int, thresholds: Sequence[float]):
        """Normalized echo density profiles and their records (ira_echo_density).  Channel c: length[c] samples at off[c]
        of x_dev, the profile starts at onset_dev[c] (int64 device, read on the device); weights: the 2 delta + 1 float64
        window weights, step the distance of neighbouring positions in samples, kmax the most positions per channel,
        thresholds 0..NED_MAX_THRESHOLDS levels.  Returns (prof float32 device, flat; prof_off int64 host (nch,): row c
        starts at prof_off[c] and holds ned_positions(length[c], 0, step, kmax) values -- the onset is not known on the
        host -- of which the first K are the profile and the rest NaN; rec (nch, NED_DOUBLES) float64 device: K, the
        positions whose window is digital silence, those whose window sum is not finite, the maximum of the others, its
        first index, the first index at or above each threshold (-1: none))."""
        t = self.torch
        off = flat(off, np.int64)
        length = flat(length, np.int64)
        delta, step, kmax = int(delta), int(step), int(kmax)
        nch = same_rows("off and length must be (nch,)", off, length)
        if not 1 <= delta <= NED_MAX_DELTA:
            raise ValueError(f"delta must be 1..{NED_MAX_DELTA} samples, got {delta}")
        weights = window_weights(weights, delta, "delta")
        if not (1 <= step < 1 << 31 and 0 <= kmax <= 1 << 31):
            raise ValueError("step must be >= 1 and kmax 0..2^31")
        thresholds = [float(v) for v in thresholds]
        if len(thresholds) > NED_MAX_THRESHOLDS:
            raise ValueError(f"at most {NED_MAX_THRESHOLDS} thresholds")
        room = ned_positions(length, 0, step, kmax)
        prof_off = exclusive_cumsum(room)
        total = int(room.sum())
        prof = self.empty(total, t.float32)
        rec = self.out_view(t.float64, nch, NED_DOUBLES)
        d_off, d_len, d_poff, d_w = self.job_tables(off, length, prof_off, weights)
        check(self.lib.ira_echo_density(_ptr(x_dev), _ptr(d_off), _ptr(d_len), _ptr(onset_dev), nch, _ptr(d_w), delta, step,
                                        kmax, _lib.dbl_array(thresholds), len(thresholds), _ptr(prof), _ptr(d_poff),
                                        _ptr(rec), self.stream), "ira_echo_density")
        return prof[:total], prof_off, rec

    # ------------------------------------------------------------------ early reflections
    def reflections(self, x_dev, off: np.ndarray, length: np.ndarray, onset_dev, weights: np.ndarray, half: int,
                    direct: int, direct_window: int, guard: int, separation: int, background: int, tn: int, rel: float,
                    prom: float, keep: int):
        """Energy-time rows, kept reflections and records (ira_reflections, one call).  Channel c: length[c] samples at
        off[c] of x_dev, the row starts at onset_dev[c] (int64 device, read on the device); weights: the 2 half + 1 float64
        smoothing weights; direct, direct_window, guard, separation, background: D, Dw, G, S, B in samples; tn: Tn in
        samples (REFL_UNBOUNDED and more: no bound); rel, prom: the level and prominence factors; keep: reflections kept.
        Returns (erow float64 device, flat; erow_off int64 host (nch,): row c starts at erow_off[c] and holds
        refl_row_room(length[c], ..) values -- the onset is not known on the host -- of which the first R are e[o + j]
        and the rest NaN; list (nch, keep, REFL_FIELDS) float64 device: n, e[n], Bsum, cnt, peak index, peak sample of
        the kept reflections in time order (-1 / NaN rows behind them); rec (nch, REFL_DOUBLES) float64 device: n0, Ed,
        M, kept, first candidate (-1), the direct and the remaining energy, non-finite row entries)."""
        t = self.torch
        off = flat(off, np.int64)
        length = flat(length, np.int64)
        half, direct, direct_window, guard = int(half), int(direct), int(direct_window), int(guard)
        separation, background, tn, keep = int(separation), int(background), int(tn), int(keep)
        nch = same_rows("off and length must be (nch,)", off, length)
        if not 1 <= half <= REFL_MAX_HALF:
            raise ValueError(f"half must be 1..{REFL_MAX_HALF} samples, got {half}")
        weights = window_weights(weights, half, "half")
        if not 1 <= direct <= REFL_MAX_DIRECT:
            raise ValueError(f"direct must be 1..{REFL_MAX_DIRECT} samples, got {direct}")
        if not 1 <= direct_window < 1 << 31:
            raise ValueError(f"direct_window must be >= 1 sample, got {direct_window}")
        if not 1 <= separation <= REFL_MAX_SEP:
            raise ValueError(f"separation must be 1..{REFL_MAX_SEP} samples, got {separation}")
        if not separation <= guard < 1 << 31:
            raise ValueError(f"guard must be at least the separation ({separation} samples), got {guard}")
        if not separation < background <= REFL_MAX_BG:
            raise ValueError(f"background must be more than the separation and at most {REFL_MAX_BG} samples, got {background}")
        if tn < 0:
            raise ValueError("tn must be >= 0")
        if not (math.isfinite(rel) and rel >= 0.0 and math.isfinite(prom) and prom >= 1.0):
            raise ValueError("rel must be finite and >= 0, prom finite and >= 1")
        if not 1 <= keep <= REFL_MAX_KEEP:
            raise ValueError(f"keep must be 1..{REFL_MAX_KEEP}, got {keep}")
        tn = min(tn, REFL_UNBOUNDED)
        room = refl_row_room(length, direct, tn, background)
        erow_off = exclusive_cumsum(room)
        total, max_room = int(room.sum()), int(room.max()) if nch else 0
        scratch_doubles = refl_scratch_doubles(nch, max_room, separation)
        erow = self.empty(total, t.float64)
        scratch = self.empty(scratch_doubles, t.float64)
        lst = self.out_view(t.float64, nch, keep, REFL_FIELDS)
        rec = self.out_view(t.float64, nch, REFL_DOUBLES)
        d_off, d_len, d_eoff = self.job_tables(off, length, erow_off)
        d_w = self.to_dev(weights)
        check(self.lib.ira_reflections(_ptr(x_dev), _ptr(d_off), _ptr(d_len), _ptr(onset_dev), nch, _ptr(d_w), half, direct,
                                       direct_window, guard, separation, background, tn, float(rel), float(prom), keep,
                                       max_room, _ptr(erow), _ptr(d_eoff), _ptr(scratch), scratch_doubles, _ptr(lst),
                                       _ptr(rec), self.stream), "ira_reflections")
        return erow[:total], erow_off, lst, rec

    # ------------------------------------------------------------------ frequency-dependent-window response
    def fdw_response(self, x_dev, off: np.ndarray, length: np.ndarray, centre_dev, rho: np.ndarray, half: np.ndarray,
                     window: str):
        """Windowed Fourier sums around a centre sample, one window length per frequency point (ira_fdw_response, one
        call).  Channel c: length[c] samples at off[c] of x_dev, centred at centre_dev[c] (int64 device, read on the
        device; it may lie outside the channel); point j: rho[j] = f_j / fs in (0, 0.5] and the half width half[j] >= 1
        samples (terms k = -half .. half); window "hann" or "rect".  Returns (nch, J, FDW_FIELDS) float64 device: Re S0,
        Im S0, Re S1, Im S1, A = sum |v|, N = the terms inside the channel."""
        t = self.torch
        off = flat(off, np.int64)
        length = flat(length, np.int64)
        rho = flat(rho, np.float64)
        nch, npts = same_rows("off and length must be (nch,)", off, length), int(rho.size)
        if nch > 65535:
            raise ValueError("at most 65535 channels per launch")
        half = point_grid(rho, half, window)
        if nch == 0 or npts == 0:                                   # nothing to launch (zero-size tables have no address)
            return self.out_view(t.float64, nch, npts, FDW_FIELDS)
        scratch_doubles = fdw_scratch_doubles(nch, half)
        scratch = self.empty(scratch_doubles, t.float64)
        out = self.out_view(t.float64, nch, npts, FDW_FIELDS)
        d_off, d_len, d_rho, d_half = self.job_tables(off, length, rho, half)
        with self.tagged(f"[{window}]"):
            check(self.lib.ira_fdw_response(_ptr(x_dev), _ptr(d_off), _ptr(d_len), _ptr(centre_dev), nch,
                                            _lib.dbl_array(rho.tolist()), _lib.i32_array(half.tolist()), _ptr(d_rho),
                                            _ptr(d_half), npts, FDW_WINDOWS.index(window), _ptr(scratch), scratch_doubles,
                                            _ptr(out), self.stream), "ira_fdw_response")
        return out

    # ------------------------------------------------------------------ burst decay (constant-Q level-over-periods map)
    def burst_table(self, rho: np.ndarray, half: np.ndarray, window: str) -> BurstTable:
        """The wavelets g_j(k) = w(k) e^{-2 pi i k rho_j}, k = -half[j] .. half[j], of every point as (re, im) doubles, one
        point after the other (ira_burst_table, one call): weight and phasor exactly as ira_fdw_response forms them.  rho[j]
        in (0, 0.5], half[j] >= 1 samples, window "hann" or "rect"."""
        t = self.torch
        rho = flat(rho, np.float64)
        half, npts = point_grid(rho, half, window), int(rho.size)
        offsets, doubles = burst_table_offsets(half), burst_table_doubles(half)
        if npts == 0:                                               # nothing to launch (zero-size tables have no address)
            return BurstTable(rho, half, window, offsets, 0, None, None, None)
        table = self.empty(doubles, t.float64)
        d_rho, d_half, d_off = self.job_tables(rho, half, offsets)
        with self.tagged(f"[{window}]"):
            check(self.lib.ira_burst_table(_lib.dbl_array(rho.tolist()), _lib.i32_array(half.tolist()), _ptr(d_rho),
                                           _ptr(d_half), _ptr(d_off), npts, FDW_WINDOWS.index(window), _ptr(table), doubles,
                                           self.stream), "ira_burst_table")
        return BurstTable(rho, half, window, offsets, doubles, table, d_half, d_off)

    def burst_decay(self, x_dev, off: np.ndarray, length: np.ndarray, centre_dev, table: BurstTable, delta: np.ndarray) -> List:
        """The map S[c, j, m] = sum over k of g_j(k) * x_c[centre_c + delta[j, m] + k] (ira_burst_decay).  Channel c:
        length[c] samples at off[c] of x_dev, centred at centre_dev[c] (int64 device, read on the device); table from
        burst_table; delta (J, M) whole samples, non-decreasing along m, |delta| <= BURST_MAX_DELTA.  The batch is cut into
        calls of burst_channels_per_call(J, M) channels, so that one call writes at most BURST_MAX_OUT_BYTES.  Returns the
        list of the calls' outputs in channel order: (channels of the call, J, M, 2) float64 device, (Re S, Im S)."""
        t = self.torch
        off = flat(off, np.int64)
        length = flat(length, np.int64)
        nch, npts = same_rows("off and length must be (nch,)", off, length), int(table.half.size)
        delta_in = np.asarray(delta)
        if delta_in.ndim != 2 or delta_in.shape[0] != npts:
            raise ValueError("delta must be (J, M)")
        nsteps = int(delta_in.shape[1])
        if nsteps > BURST_MAX_STEPS:
            raise ValueError(f"at most {BURST_MAX_STEPS} steps, got {nsteps}")
        if not whole_numbers(delta_in, -BURST_MAX_DELTA, BURST_MAX_DELTA):
            raise ValueError(f"delta must be whole numbers of at most {BURST_MAX_DELTA} samples either way")
        if delta_in.size and np.any(np.diff(delta_in, axis=1) < 0):
            raise ValueError("delta must not decrease along the steps")
        delta = np.ascontiguousarray(delta_in, dtype=np.int32)
        if nch == 0 or npts == 0 or nsteps == 0:                    # nothing to launch
            return [self.out_view(t.float64, nch, npts, nsteps, 2)]
        per_call = self.burst_channels_per_call(npts, nsteps)
        d_off, d_len, d_delta = self.job_tables(off, length, delta.reshape(-1))
        c_half = _lib.i32_array(table.half.tolist())
        c_delta = _lib.i32_array(delta.reshape(-1).tolist())
        outs = []
        with self.tagged(f"[{table.window}]"):
            for a in range(0, nch, per_call):
                n = min(per_call, nch - a)
                out = self.out_view(t.float64, n, npts, nsteps, 2)
                check(self.lib.ira_burst_decay(_ptr(x_dev), _ptr(d_off[a:]), _ptr(d_len[a:]), _ptr(centre_dev[a:]), n, c_half,
                                               _ptr(table.half_dev), _ptr(table.offsets_dev), _ptr(table.table), table.doubles,
                                               c_delta, _ptr(d_delta), npts, nsteps, _ptr(out), self.stream),
                      "ira_burst_decay")
                outs.append(out)
        return outs

    # ------------------------------------------------------------------ minimum phase / excess phase (real cepstrum)
    @staticmethod
    def _minphase_sizes(spec_off: np.ndarray, n_fft: np.ndarray):
        spec_off = flat(spec_off, np.int64)
        n_in = np.asarray(n_fft).reshape(-1)
        same_rows("spec_off and n_fft must be (n,)", spec_off, n_in)
        if spec_off.size > 65535:
            raise ValueError("at most 65535 channels per launch")
        n64 = n_in.astype(np.int64)
        if not (whole_numbers(n_in, MINPHASE_MIN_N, 1 << MINPHASE_MAX_LOG2) and np.all(n64 & (n64 - 1) == 0)):
            raise ValueError(f"n_fft must be powers of two {MINPHASE_MIN_N}..2^{MINPHASE_MAX_LOG2}")
        return spec_off, n64.astype(np.int32)

    def minphase_logmag(self, spec_dev, spec_off: np.ndarray, n_fft: np.ndarray, floor_db: float):
        """G = 0.5 ln(max(|X|^2, P 10^(floor_db / 10))) as the complex (G, 0) at the spectra's own offsets, P = max |X|^2 per
        element and the count of bins below the floor (ira_minphase_logmag).  Returns (g float64 device laid out like
        spec_dev, pmax float64 device (n,), floored int64 device (n,))."""
        t = self.torch
        spec_off, n_fft = self._minphase_sizes(spec_off, n_fft)
        if not (MINPHASE_MIN_FLOOR_DB <= float(floor_db) <= 0.0):
            raise ValueError(f"floor_db must lie in {MINPHASE_MIN_FLOOR_DB:g} .. 0, got {floor_db}")
        n = int(spec_off.size)
        g = self.empty(int((n_fft.astype(np.int64) // 2 + 1).sum()) * 2, t.float64)
        pmax, floored = self.empty(n, t.float64), self.empty(n, t.int64)
        if n:
            d_so, d_nf = self.job_tables(spec_off, n_fft)
            check(self.lib.ira_minphase_logmag(_ptr(spec_dev), _ptr(d_so), _ptr(d_nf), n, int(n_fft.max()), float(floor_db),
                                               _ptr(g), _ptr(pmax), _ptr(floored), self.stream), "ira_minphase_logmag")
        return g, pmax[:n], floored[:n]

    def minphase_excess(self, spec_dev, tspec_dev, spec_off: np.ndarray, n_fft: np.ndarray, centre: np.ndarray, pmax_dev):
        """wrap(phi_rel - phi_min) per bin, float64 radians, one double per bin at spec_off (the offsets phase_unwrap
        takes): phi_rel = angle(X_k) + 2 pi frac(k centre / N), phi_min = 2 Im T_k (ira_minphase_excess)."""
        t = self.torch
        spec_off, n_fft = self._minphase_sizes(spec_off, n_fft)
        centre = flat(centre, np.int64)
        n = int(spec_off.size)
        if centre.size != n or (n and (centre.min() < 0 or centre.max() >= 1 << 31)):
            raise ValueError("centre must be (n,) sample indices 0 .. 2^31 - 1")
        ex = self.empty(int((n_fft.astype(np.int64) // 2 + 1).sum()), t.float64)
        if n:
            d_so, d_nf, d_c = self.job_tables(spec_off, n_fft, centre)
            check(self.lib.ira_minphase_excess(_ptr(spec_dev), _ptr(tspec_dev), _ptr(d_so), _ptr(d_nf), _ptr(d_c),
                                               _ptr(pmax_dev), n, int(n_fft.max()), _ptr(ex), self.stream),
                  "ira_minphase_excess")
        return ex

    def minphase_gather(self, spec_dev, tspec_dev, unwrapped_dev, spec_off: np.ndarray, n_fft: np.ndarray, bins: np.ndarray,
                        pmax_dev):
        """The records of the grid points: bins (n, J) whole numbers 1 .. N/2 - 1 per element -> (n, J, MINPHASE_FIELDS)
        float64 device: Re X, Im X, Im T at k - 1, k, k + 1, the unwrapped excess phase at k - 1, k, k + 1; NaN for an
        element without values (ira_minphase_gather)."""
        t = self.torch
        spec_off, n_fft = self._minphase_sizes(spec_off, n_fft)
        n = int(spec_off.size)
        bins_in = np.asarray(bins)
        if bins_in.ndim != 2 or bins_in.shape[0] != n:
            raise ValueError("bins must be (n, J)")
        npts = int(bins_in.shape[1])
        if npts > FDW_MAX_POINTS:
            raise ValueError(f"at most {FDW_MAX_POINTS} frequency points, got {npts}")
        if not whole_numbers(bins_in, 1, (n_fft.astype(np.int64) // 2 - 1)[:, None]):
            raise ValueError("bins must be whole numbers 1 .. n_fft / 2 - 1")
        bins = np.ascontiguousarray(bins_in, dtype=np.int32)
        if n == 0 or npts == 0:                                     # nothing to launch (zero-size tables have no address)
            return self.out_view(t.float64, n, npts, MINPHASE_FIELDS)
        out = self.out_view(t.float64, n, npts, MINPHASE_FIELDS)
        d_so, d_nf, d_b = self.job_tables(spec_off, n_fft, bins.reshape(-1))
        check(self.lib.ira_minphase_gather(_ptr(spec_dev), _ptr(tspec_dev), _ptr(unwrapped_dev), _ptr(d_so), _ptr(d_nf),
                                           _ptr(d_b), _ptr(pmax_dev), n, npts, _ptr(out), self.stream), "ira_minphase_gather")
        return out

    def minphase_spectrum(self, g_dev, tspec_dev, spec_off: np.ndarray, n_fft: np.ndarray, pmax_dev) -> None:
        """M = e^G (cos phi_min, sin phi_min), phi_min = 2 Im T, in place of G; Im M = 0 at k = 0 and N/2
        (ira_minphase_spectrum)."""
        spec_off, n_fft = self._minphase_sizes(spec_off, n_fft)
        n = int(spec_off.size)
        if n:
            d_so, d_nf = self.job_tables(spec_off, n_fft)
            check(self.lib.ira_minphase_spectrum(_ptr(g_dev), _ptr(tspec_dev), _ptr(d_so), _ptr(d_nf), _ptr(pmax_dev), n,
                                                 int(n_fft.max()), self.stream), "ira_minphase_spectrum")

    # ------------------------------------------------------------------ equalisation (smoothing pyramid, inversion, taper)
    @staticmethod
    def _eq_sizes(nrows: int, n_fft: int) -> int:
        n = int(n_fft)
        if not 0 <= int(nrows) <= 65535:
            raise ValueError("at most 65535 rows per launch")
        if not (MINPHASE_MIN_N <= n <= 1 << MINPHASE_MAX_LOG2 and n & (n - 1) == 0):
            raise ValueError(f"n_fft must be a power of two {MINPHASE_MIN_N}..2^{MINPHASE_MAX_LOG2}, got {n_fft}")
        return n

    def eq_power(self, spec_dev, spec_off: np.ndarray, members: Sequence[Sequence[int]], n_fft: int, spec2_dev=None,
                 spec2_off: Optional[np.ndarray] = None, pyr=None):
        """Level 0 of every row's pyramid (ira_eq_power): row r = the mean over members[r] (indices into spec_off, in this
        order) of |X|^2, times |F|^2 of the row's second spectrum at spec2_off[r] when spec2_dev is given.  Returns the
        pyramid buffer, float64 device (rows, equalise_row_doubles(n_fft)); pyr: one to write into instead."""
        t = self.torch
        spec_off = flat(spec_off, np.int64)
        nrows = len(members)
        n = self._eq_sizes(nrows, n_fft)
        counts = np.array([len(m) for m in members], dtype=np.int64)
        table = np.array([int(i) for m in members for i in m], dtype=np.int64)
        if nrows and (counts.min() < 1 or counts.max() > EQ_MAX_MEMBERS):
            raise ValueError(f"a row holds 1 .. {EQ_MAX_MEMBERS} members")
        if table.size and (table.min() < 0 or table.max() >= spec_off.size):
            raise ValueError("members must index spec_off")
        if spec2_dev is not None:
            spec2_off = flat(spec2_off, np.int64)
            if spec2_off is None or spec2_off.size != nrows:
                raise ValueError("spec2_off must give one offset per row")
        row_doubles = equalise_row_doubles(n)
        if pyr is None:
            pyr = self.out_view(t.float64, nrows, row_doubles)
        elif tuple(pyr.shape) != (nrows, row_doubles):
            raise ValueError("pyr must be (rows, equalise_row_doubles(n_fft))")
        if nrows:
            first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
            d_so, d_m, d_f, d_s2 = self.job_tables(spec_off, table.astype(np.int32), first,
                                                   spec2_off if spec2_dev is not None else None)
            check(self.lib.ira_eq_power(_ptr(spec_dev), _ptr(d_so), int(spec_off.size), _ptr(d_m), int(table.size), _ptr(d_f),
                                        nrows, _ptr(spec2_dev), _ptr(d_s2), n, _ptr(pyr), self.stream), "ira_eq_power")
        return pyr

    def eq_pyramid(self, pyr, n_fft: int) -> None:
        """The upper levels of every row's pyramid from level 0, in place (ira_eq_pyramid)."""
        n = self._eq_sizes(int(pyr.shape[0]), n_fft)
        if pyr.ndim != 2 or int(pyr.shape[1]) != equalise_row_doubles(n):
            raise ValueError("pyr must be (rows, equalise_row_doubles(n_fft))")
        if pyr.shape[0]:
            check(self.lib.ira_eq_pyramid(_ptr(pyr), int(pyr.shape[0]), n, self.stream), "ira_eq_pyramid")

    def eq_smooth(self, pyr, lo: np.ndarray, hi: np.ndarray, n_fft: int):
        """S_k = W(lo_k, hi_k) / (hi_k - lo_k + 1) of every row (ira_eq_smooth): float64 device (rows, N/2 + 1).  lo, hi: (N/2 + 1,)
        whole numbers with 0 <= lo <= hi <= N/2, one pair per call."""
        nrows = int(pyr.shape[0])
        n = self._eq_sizes(nrows, n_fft)
        if pyr.ndim != 2 or int(pyr.shape[1]) != equalise_row_doubles(n):
            raise ValueError("pyr must be (rows, equalise_row_doubles(n_fft))")
        half = n // 2
        lo_in, hi_in = np.asarray(lo).reshape(-1), np.asarray(hi).reshape(-1)
        if lo_in.size != half + 1 or hi_in.size != half + 1:
            raise ValueError("lo and hi must have n_fft / 2 + 1 entries")
        if not (whole_numbers(lo_in, 0, half) and whole_numbers(hi_in, 0, half) and np.all(lo_in <= hi_in)):
            raise ValueError("lo and hi must be whole numbers with 0 <= lo <= hi <= n_fft / 2")
        d_lo, d_hi = self.job_tables(lo_in.astype(np.int32), hi_in.astype(np.int32))
        out = self.out_view(self.torch.float64, nrows, n // 2 + 1)
        if nrows:
            check(self.lib.ira_eq_smooth(_ptr(pyr), _ptr(d_lo), _ptr(d_hi), nrows, n, _ptr(out), self.stream), "ira_eq_smooth")
        return out

    def eq_invert(self, s_dev, ref: np.ndarray, target: np.ndarray, beta: np.ndarray, max_gain: float, c_off: np.ndarray,
                  n_fft: int, c_dev=None):
        """c = (a t + beta) / (s + beta), s = S / ref, a = sqrt(s), max_gain where it exceeds that, as the complex (c, 0) of row
        r at c_off[r] (in complex doubles), and the clamped bins per row (ira_eq_invert).  A row whose ref is not a positive
        finite number gets c = 1.  Returns (c float64 device, clamped int64 device (rows,))."""
        t = self.torch
        ref, c_off = flat(ref, np.float64), flat(c_off, np.int64)
        target, beta = flat(target, np.float64), flat(beta, np.float64)
        nrows = same_rows("ref and c_off must be (rows,)", ref, c_off)
        n = self._eq_sizes(nrows, n_fft)
        nbins = n // 2 + 1
        if target.size != nbins or beta.size != nbins:
            raise ValueError("target and beta must have n_fft / 2 + 1 entries")
        if not (float(max_gain) > 0.0 and math.isfinite(float(max_gain))):
            raise ValueError(f"max_gain must be a positive finite number, got {max_gain}")
        if tuple(s_dev.shape) != (nrows, nbins):
            raise ValueError("s_dev must be (rows, n_fft / 2 + 1)")
        if nrows and (c_off.min() < 0 or np.any(np.diff(np.sort(c_off)) < nbins)):
            raise ValueError("c_off must place the rows n_fft / 2 + 1 bins apart")
        if c_dev is None:
            c_dev = self.empty(2 * (int(c_off.max()) + nbins) if nrows else 0, t.float64)
        elif nrows and c_dev.numel() < 2 * (int(c_off.max()) + nbins):
            raise ValueError("c_dev is too short for c_off")
        clamped = self.empty(nrows, t.int64)
        if nrows:
            d_ref, d_co = self.job_tables(ref, c_off)
            d_t, d_b = self.to_dev(target), self.to_dev(beta)
            check(self.lib.ira_eq_invert(_ptr(s_dev), _ptr(d_ref), _ptr(d_t), _ptr(d_b), float(max_gain), _ptr(d_co), nrows, n,
                                         _ptr(c_dev), _ptr(clamped), self.stream), "ira_eq_invert")
        return c_dev, clamped[:nrows]

    def eq_gather(self, src_dev, src_off: np.ndarray, stride: int, bins: np.ndarray, n_fft: int):
        """src[src_off[r] + stride * bins[j]] per (row, grid point), offsets and stride in doubles (ira_eq_gather): float64
        device (rows, J).  bins: whole numbers 0 .. N/2, one table per call."""
        src_off = flat(src_off, np.int64)
        nrows = int(src_off.size)
        n = self._eq_sizes(nrows, n_fft)
        bins_in = np.asarray(bins).reshape(-1)
        npts = int(bins_in.size)
        if npts > FDW_MAX_POINTS:
            raise ValueError(f"at most {FDW_MAX_POINTS} frequency points, got {npts}")
        if not whole_numbers(bins_in, 0, n // 2):
            raise ValueError("bins must be whole numbers 0 .. n_fft / 2")
        if int(stride) not in (1, 2):
            raise ValueError("stride must be 1 or 2")
        if nrows and (src_off.min() < 0 or int(src_off.max()) + int(stride) * (n // 2) >= src_dev.numel()):
            raise ValueError("src_off leaves the source")
        out = self.out_view(self.torch.float64, nrows, npts)
        if nrows and npts:
            d_so, d_b = self.job_tables(src_off, bins_in.astype(np.int32))
            check(self.lib.ira_eq_gather(_ptr(src_dev), _ptr(d_so), int(stride), _ptr(d_b), nrows, npts, n, _ptr(out),
                                         self.stream), "ira_eq_gather")
        return out

    def eq_taper(self, g_dev, g_off: np.ndarray, taper: np.ndarray, n_fft: int):
        """f[r, n] = float32((double)g[g_off[r] + n] * taper[n]), n < taps (ira_eq_taper): float32 device (rows, taps)."""
        g_off, taper = flat(g_off, np.int64), flat(taper, np.float64)
        nrows, taps = int(g_off.size), int(taper.size)
        n = self._eq_sizes(nrows, n_fft)
        if not 1 <= taps <= n // 2:
            raise ValueError(f"1 <= taps <= n_fft / 2, got {taps} at n_fft {n}")
        if nrows and (g_off.min() < 0 or int(g_off.max()) + taps > g_dev.numel()):
            raise ValueError("g_off leaves the source")
        out = self.out_view(self.torch.float32, nrows, taps)
        if nrows:
            d_go = self.job_tables(g_off)[0]
            check(self.lib.ira_eq_taper(_ptr(g_dev), _ptr(d_go), _ptr(self.to_dev(taper)), nrows, taps, n, _ptr(out),
                                        self.stream), "ira_eq_taper")
        return out

    # ------------------------------------------------------------------ MLS measurement (fast Hadamard transform)
    def mls_device_tables(self, order: int, taps=None):
        """(G, out) of mls_tables(order, taps) on the device, int32 (P,) each: made on the host and uploaded once per
        engine and (order, taps)."""
        tp = mls_taps(order, taps)
        # (a copy goes up: the host's cached tables are read-only arrays)
        return self._cached(("mls", int(order), tp),
                            lambda: tuple(self._table_to_dev(v.copy()) for v in mls_tables(order, tp)))

    @staticmethod
    def _mls_sizes(nb: int, order: int, periods: Optional[int] = None) -> None:
        mls_taps(order)                                             # (the order's own check)
        if not 0 <= int(nb) <= 65535:
            raise ValueError("at most 65535 channels per launch")
        if periods is not None and not 1 <= int(periods) <= MLS_MAX_PERIODS:
            raise ValueError(f"periods must be 1..{MLS_MAX_PERIODS}, got {periods}")

    def mls_fold(self, x_dev, begin: np.ndarray, order: int, periods: int, taps=None):
        """The periods of every channel folded into one and scattered through G (ira_mls_fold).  Channel e: periods * P
        samples from begin[e] of x_dev (P = 2^order - 1; one order and one count of periods per call).  Returns (w float64
        device (nb, 2^order): Y[n] at w[G[n]], 0 at w[0]; sums float64 device (nb, 2): E = sum Y^2 and the residual energy
        D = sum (x - Y / periods)^2)."""
        t = self.torch
        begin = flat(begin, np.int64)
        nb, order, periods = int(begin.size), int(order), int(periods)
        self._mls_sizes(nb, order, periods)
        if nb and (begin.min() < 0 or int(begin.max()) + periods * ((1 << order) - 1) > int(x_dev.numel())):
            raise ValueError("every channel's periods must lie inside x_dev")
        w = self.out_view(t.float64, nb, 1 << order)
        sums = self.out_view(t.float64, nb, 2)
        if nb:
            g_dev, _ = self.mls_device_tables(order, taps)
            scratch = self.empty(2 * nb * mls_fold_blocks(order), t.float64)
            d_begin, = self.job_tables(begin)
            with self.tagged(f"[{order}]"):
                check(self.lib.ira_mls_fold(_ptr(x_dev), _ptr(d_begin), nb, order, periods, _ptr(g_dev), _ptr(w), _ptr(sums),
                                            _ptr(scratch), self.stream), "ira_mls_fold")
        return w, sums

    def mls_hadamard(self, w_dev, nb: int, order: int) -> None:
        """The natural-order Walsh-Hadamard transform of the nb rows of 2^order doubles of w_dev, in place, stages
        h = 1, 2, 4 .. in that order (ira_mls_hadamard; mls_pass_plan(order) says in how many passes)."""
        nb, order = int(nb), int(order)
        self._mls_sizes(nb, order)
        if int(w_dev.numel()) < nb << order:
            raise ValueError("w_dev must hold nb rows of 2^order doubles")
        if nb:
            with self.tagged(f"[{order}]"):
                check(self.lib.ira_mls_hadamard(_ptr(w_dev), nb, order, self.stream), "ira_mls_hadamard")

    def mls_finish(self, w_dev, nb: int, order: int, periods: int, h_dev, h_off: np.ndarray, taps=None) -> None:
        """h[k] = float32((W[out[k]] - W[0]) / (2^order periods)), k < P, of every row of the transformed workspace, written
        at h_off[e] of h_dev (float32 device); nothing else of h_dev is touched (ira_mls_finish)."""
        nb, order, periods = int(nb), int(order), int(periods)
        h_off = flat(h_off, np.int64)
        self._mls_sizes(nb, order, periods)
        if h_off.size != nb or int(w_dev.numel()) < nb << order:
            raise ValueError("h_off must be (nb,) and w_dev hold nb rows of 2^order doubles")
        if nb and (h_off.min() < 0 or int(h_off.max()) + (1 << order) - 1 > int(h_dev.numel())):
            raise ValueError("every response must lie inside h_dev")
        if nb:
            _, out_dev = self.mls_device_tables(order, taps)
            d_off, = self.job_tables(h_off)
            with self.tagged(f"[{order}]"):
                check(self.lib.ira_mls_finish(_ptr(w_dev), _ptr(out_dev), nb, order, periods, _ptr(h_dev), _ptr(d_off),
                                              self.stream), "ira_mls_finish")

    # ------------------------------------------------------------------ dual-channel spectral sums (Welch H1 / H2)
    def cross_spectra(self, x_dev, x_off: np.ndarray, y_off: np.ndarray, n: np.ndarray, n_fft: int, hop: int,
                      use_hann: bool):
        """Auto- and cross-spectra of (reference, measurement) pairs summed over overlapping frames, and what follows from
        them (ira_xspec_accumulate, ira_xspec_finish).  Pair p: reference n[p] samples at x_off[p] of x_dev, measurement
        n[p] samples at y_off[p] (the pair's delay is in the offsets); K = 1 + (n[p] - n_fft) // hop frames, none when
        n[p] < n_fft.  The window is window(n_fft, use_hann, 64).  Returns (npairs, XSPEC_ROWS, n_fft // 2 + 1) float64
        device: Sxx, Syy, Re Sxy, Im Sxy, H1 (re, im), H2 (re, im), coherence, 20 log10 |H1|, phase."""
        t = self.torch
        x_off = flat(x_off, np.int64)
        y_off = flat(y_off, np.int64)
        n = flat(n, np.int64)
        n_fft, hop = int(n_fft), int(hop)
        npairs = same_rows("x_off, y_off and n must be (npairs,)", x_off, y_off, n)
        if n_fft < XSPEC_MIN_FFT or n_fft > XSPEC_MAX_FFT or n_fft & (n_fft - 1):
            raise ValueError(f"n_fft must be a power of two from {XSPEC_MIN_FFT} to {XSPEC_MAX_FFT}, got {n_fft}")
        if not 1 <= hop <= n_fft:
            raise ValueError(f"hop must be 1 .. n_fft, got {hop}")
        if npairs > 65535:
            raise ValueError("at most 65535 pairs per launch")
        total = int(x_dev.numel())
        if npairs and (n.min() < 0 or min(x_off.min(), y_off.min()) < 0 or max((x_off + n).max(), (y_off + n).max()) > total):
            raise ValueError("a pair's rows must lie inside x_dev")
        nbins = n_fft // 2 + 1
        if npairs == 0:                                         # nothing to launch (zero-size tables have no address)
            return self.out_view(t.float64, 0, XSPEC_ROWS, nbins)
        max_frames = int(xspec_frames(n, n_fft, hop).max())
        if max_frames >= 1 << 31:
            raise ValueError("too many frames for one launch")
        chunks = -(-max_frames // XSPEC_FRAMES)
        partial = self.empty(npairs * chunks * 4 * nbins, t.float64)
        out = self.out_view(t.float64, npairs, XSPEC_ROWS, nbins)
        win, tw = self.window(n_fft, use_hann, 64), self.twiddle(n_fft, 64)
        d_xo, d_yo, d_n = self.job_tables(x_off, y_off, n)
        with self.tagged(f"[{n_fft}]"):
            check(self.lib.ira_xspec_accumulate(_ptr(x_dev), _ptr(d_xo), _ptr(d_yo), _ptr(d_n), npairs, max_frames, n_fft,
                                                hop, _ptr(win), _ptr(tw), _ptr(partial), self.stream),
                  "ira_xspec_accumulate")
            check(self.lib.ira_xspec_finish(_ptr(partial), _ptr(d_n), npairs, max_frames, n_fft, hop, _ptr(out),
                                            self.stream), "ira_xspec_finish")
        return out

    # ------------------------------------------------------------------ energy decay relief (Jot)
    @staticmethod
    def _edr_sizes(nseg: int, nrows: int) -> None:
        if nseg > 65535:
            raise ValueError("at most 65535 segments per launch")
        if not 1 <= nrows <= EDR_MAX_ROWS:
            raise ValueError(f"1 to {EDR_MAX_ROWS} rows, got {nrows}")

    def edr_power(self, x_dev, x_off: np.ndarray, n: np.ndarray, n_fft: int, hop: int, use_hann: bool, first: np.ndarray,
                  count: np.ndarray):
        """Band powers of every frame (ira_edr_power).  Segment s: n[s] samples at x_off[s] of x_dev, T = 1 + (n[s] - n_fft)
        // hop frames (none when n[s] < n_fft); row j: the rFFT bins first[j] .. first[j] + count[j] - 1 (count 0: an empty
        row, powers 0.0).  The window is window(n_fft, use_hann, 64).  Returns (P float64 device, flat, in the layout of
        edr_layout; frames int64 host (nseg,); p_off int64 host (nseg,))."""
        t = self.torch
        x_off, n = flat(x_off, np.int64), flat(n, np.int64)
        first, count = flat(first, np.int32), flat(count, np.int32)
        n_fft, hop = int(n_fft), int(hop)
        nseg = same_rows("x_off and n must be (nseg,)", x_off, n)
        nrows = same_rows("first and count must be (nrows,)", first, count)
        self._edr_sizes(nseg, nrows)
        if n_fft < EDR_MIN_FFT or n_fft > EDR_MAX_FFT or n_fft & (n_fft - 1):
            raise ValueError(f"n_fft must be a power of two from {EDR_MIN_FFT} to {EDR_MAX_FFT}, got {n_fft}")
        if not 1 <= hop <= n_fft:
            raise ValueError(f"hop must be 1 .. n_fft, got {hop}")
        if first.min() < 0 or count.min() < 0 or int((first.astype(np.int64) + count).max()) > n_fft // 2 + 1:
            raise ValueError("a row's bins must lie in 0 .. n_fft / 2")
        if nseg and (n.min() < 0 or x_off.min() < 0 or int((x_off + n).max()) > int(x_dev.numel())):
            raise ValueError("a segment must lie inside x_dev")
        frames = xspec_frames(n, n_fft, hop)
        _, p_off, _, total = edr_layout(frames, nrows)
        max_frames = int(frames.max()) if nseg else 0
        if max_frames >= 1 << 31:
            raise ValueError("too many frames for one launch")
        p = self.empty(total, t.float64)
        if nseg and max_frames:
            win, tw = self.window(n_fft, use_hann, 64), self.twiddle(n_fft, 64)
            d_xo, d_n, d_po, d_first, d_count = self.job_tables(x_off, n, p_off, first, count)
            with self.tagged(f"[{n_fft}]"):
                check(self.lib.ira_edr_power(_ptr(x_dev), _ptr(d_xo), _ptr(d_n), _ptr(d_po), nseg, max_frames, n_fft, hop,
                                             _ptr(win), _ptr(tw), _ptr(d_first), _ptr(d_count), nrows, _ptr(p), self.stream),
                      "ira_edr_power")
        return p[:total], frames, p_off

    def edr_integrate(self, p_dev, frames: np.ndarray, nrows: int, noise_frames: np.ndarray, eps: float, floor_db: float,
                      with_sums: bool = False):
        """Backward sums of the band powers along the frame axis, their records and float32 dB curves (ira_edr_integrate).
        p_dev: P in the layout of edr_layout(frames, nrows) (what edr_power returns, or a host-made one); noise_frames[s] =
        q, 0 <= q <= frames[s], the last frames whose mean level is subtracted (0: none).  Returns (curves float32 device,
        flat: (nrows, T_s) at c_off[s]; c_off int64 host (nseg,); records (nseg, nrows, EDR_DOUBLES) float64 device: S(0), N,
        max P, the first frame of that maximum; S float64 device in the layout of P, or None unless with_sums)."""
        t = self.torch
        frames, noise_frames = flat(frames, np.int64), flat(noise_frames, np.int64)
        nrows = int(nrows)
        nseg = same_rows("frames and noise_frames must be (nseg,)", frames, noise_frames)
        self._edr_sizes(nseg, nrows)
        eps, floor_db = float(eps), float(floor_db)
        if not (math.isfinite(eps) and eps >= 0.0 and math.isfinite(floor_db)):
            raise ValueError("eps must be finite and >= 0, floor_db finite")
        if nseg and (frames.min() < 0 or frames.max() >= 1 << 31 or noise_frames.min() < 0 or np.any(noise_frames > frames)):
            raise ValueError("frames must be 0 .. 2^31 - 1 and noise_frames 0 .. frames")
        _, p_off, c_off, total = edr_layout(frames, nrows)
        if total > int(p_dev.numel()):
            raise ValueError("p_dev is smaller than the layout of frames and nrows")
        ncurve = int(frames.sum()) * nrows
        curves = self.empty(ncurve, t.float32)
        rec = self.out_view(t.float64, nseg, nrows, EDR_DOUBLES)
        sums = self.empty(total, t.float64) if with_sums else None
        if nseg:
            d_po, d_t, d_q, d_co = self.job_tables(p_off, frames.astype(np.int32), noise_frames.astype(np.int32), c_off)
            check(self.lib.ira_edr_integrate(_ptr(p_dev), _ptr(d_po), _ptr(d_t), _ptr(d_q), _ptr(d_co), nseg, nrows, eps,
                                             floor_db, _ptr(curves), _ptr(rec), _ptr(sums), self.stream),
                  "ira_edr_integrate")
        return curves[:ncurve], c_off, rec, (sums[:total] if with_sums else None)

    # ------------------------------------------------------------------ ISO 3382-1 inter-channel cross-correlation
    def xcorr_windows(self, x_dev, l_off: np.ndarray, r_off: np.ndarray, seg_len: np.ndarray, lchan_of_seg: np.ndarray,
                      rchan_of_seg: np.ndarray, onset_dev, limits: np.ndarray, max_lag: int):
        """Partitioned float64 lag sums between the two channels of stereo pairs (ira_xcorr_windows).  Segment j: left
        channel seg_len[j] samples at l_off[j] of x_dev, right channel at r_off[j]; it starts at
        o = min(onset_dev[lchan_of_seg[j]], onset_dev[rchan_of_seg[j]]), taken on the device; limits (nseg, nlim) int64
        ascending sample counts from o.  Returns (nseg, nlim + 1, 2 max_lag + 3) float64 device: per partition
        C(-max_lag .. +max_lag), El, Er."""
        t = self.torch
        l_off = flat(l_off, np.int64)
        r_off = flat(r_off, np.int64)
        seg_len = flat(seg_len, np.int64)
        nseg = int(l_off.size)
        limits = np.ascontiguousarray(limits, dtype=np.int64)
        if limits.ndim != 2 or limits.shape[0] != nseg or r_off.size != nseg or seg_len.size != nseg:
            raise ValueError("l_off, r_off, seg_len must be (nseg,) and limits (nseg, nlim)")
        nlim, max_lag = int(limits.shape[1]), int(max_lag)
        max_len = int(seg_len.max()) if nseg else 0
        scratch = self._scratch("ira_xcorr_scratch_doubles", nseg, max_len, nlim, max_lag)
        nrec = 2 * max_lag + 3
        out = self.out_view(t.float64, nseg, nlim + 1, nrec)
        d_lo, d_ro, d_len, d_lc, d_rc, d_lim = self.job_tables(l_off, r_off, seg_len, flat(lchan_of_seg, np.int32),
                                                               flat(rchan_of_seg, np.int32), limits.reshape(-1))
        with self.tagged(f"[T{max_lag}]"):
            check(self.lib.ira_xcorr_windows(_ptr(x_dev), _ptr(d_lo), _ptr(d_ro), _ptr(d_len), _ptr(d_lc), _ptr(d_rc),
                                             _ptr(onset_dev), nseg, max_len, _ptr(d_lim), nlim, max_lag, _ptr(scratch),
                                             _ptr(out), self.stream), "ira_xcorr_windows")
        return out

    # ------------------------------------------------------------------ IEC 60268-16 modulation transfer sums
    def mtf_sums(self, x_dev, seg_off: np.ndarray, seg_len: np.ndarray, w: np.ndarray):
        """Float64 modulation transfer sums of the squared signal (ira_mtf_sums).  Row j: seg_len[j] samples at seg_off[j] of
        x_dev; w (nseg, nf) float64 modulation frequencies in turns per sample (frequency / sample rate, per row), nf <= 16,
        0 <= w <= 0.5.  Returns (nseg, 2 nf + 1) float64 device: E = sum x^2, then A_i = sum x[n]^2 cos(2 pi w_i n) and
        B_i = sum x[n]^2 sin(2 pi w_i n) per frequency, n counted from the row's first sample."""
        t = self.torch
        seg_off = flat(seg_off, np.int64)
        seg_len = flat(seg_len, np.int64)
        nseg = int(seg_off.size)
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.ndim != 2 or w.shape[0] != nseg or seg_len.size != nseg:
            raise ValueError("seg_off, seg_len must be (nseg,) and w (nseg, nf)")
        nf = int(w.shape[1])
        if not np.all((w >= 0.0) & (w <= 0.5)):
            raise ValueError("modulation frequencies must lie in 0 .. 0.5 turns per sample")
        max_len = int(seg_len.max()) if nseg else 0
        scratch = self._scratch("ira_mtf_scratch_doubles", nseg, max_len, nf)
        nrec = 2 * nf + 1
        out = self.out_view(t.float64, nseg, nrec)
        d_off, d_len, d_w = self.job_tables(seg_off, seg_len, w.reshape(-1))
        check(self.lib.ira_mtf_sums(_ptr(x_dev), _ptr(d_off), _ptr(d_len), _ptr(d_w), nseg, max_len, nf, _ptr(scratch),
                                    _ptr(out), self.stream), "ira_mtf_sums")
        return out

    # ------------------------------------------------------------------ harmonic distortion from a deconvolved sweep
    def harmonic_peaks(self, h_dev, h_off: np.ndarray, n_search: np.ndarray):
        """The linear peak of circular responses: the first maximum of |h| over the first n_search[c] samples of channel c
        (ira_peak_index on a view of h; nothing returns to the host).  Returns (peak int64 device, |h[peak]| float32
        device), one entry per channel."""
        h_off = flat(h_off, np.int64)
        n_search = np.ascontiguousarray(n_search, dtype=np.int64)
        n = int(h_off.size)
        if n_search.shape != (n,) or (n and n_search.min() < 1):
            raise ValueError("n_search must hold one length >= 1 per channel")
        d_off, d_len = self.job_tables(h_off, n_search)
        pk, pa = self._peak_pick(h_dev, d_off, d_len, n, int(n_search.max()) if n else 0)
        return pk[:n], pa[:n]

    def harmonic_windows(self, h_dev, h_off: np.ndarray, n_fft: np.ndarray, peak_dev, lags: np.ndarray, guard: int,
                         window: np.ndarray):
        """Windowed harmonic segments (ira_harmonic_windows).  Channel c: the circular response of n_fft[c] samples at
        h_off[c] of h_dev, peak_dev[c] its linear peak on the device; lags (K,) int64 samples; window (seg,) float64.
        Returns (nch * K, seg) float32 device, row c * K + k:
        float32(float64(h_c[(peak - lags[k] - guard + i) mod n_fft[c]]) * window[i])."""
        t = self.torch
        h_off = flat(h_off, np.int64)
        n_fft = np.ascontiguousarray(n_fft, dtype=np.int32)
        lags = flat(lags, np.int64)
        window = flat(window, np.float64)
        nch, k, seg, guard = int(h_off.size), int(lags.size), int(window.size), int(guard)
        if n_fft.shape != (nch,) or (nch and n_fft.min() < 1):
            raise ValueError("n_fft must hold one length >= 1 per channel")
        if not (1 <= guard < seg):
            raise ValueError("guard must be at least 1 sample and the window longer than it")
        out = self.out_view(t.float32, nch * k, seg)
        if nch:
            d_off, d_n, d_lag, d_win = self.job_tables(h_off, n_fft, lags, window)
            check(self.lib.ira_harmonic_windows(_ptr(h_dev), _ptr(d_off), _ptr(d_n), _ptr(peak_dev), _ptr(d_lag),
                                                _ptr(d_win), nch, k, guard, seg, _ptr(out), self.stream),
                  "ira_harmonic_windows")
        return out

    def harmonic_band_powers(self, spec_dev, spec_off: np.ndarray, lo: np.ndarray, cnt: np.ndarray, nbins: int):
        """Mean band powers of half spectra (ira_harmonic_band_powers).  Row r: nbins complex float64 values at spec_off[r]
        (in complex values, as rfft_any returns them) of spec_dev; lo / cnt (K, J) int32, shared by every channel; row r
        belongs to harmonic r % K.  Returns (nrow // K, K, J) float64 device: the mean of re^2 + im^2 over the bins
        lo .. lo + cnt - 1, 0 where cnt = 0."""
        t = self.torch
        spec_off = flat(spec_off, np.int64)
        lo = np.ascontiguousarray(lo, dtype=np.int32)
        cnt = np.ascontiguousarray(cnt, dtype=np.int32)
        nrow, nbins = int(spec_off.size), int(nbins)
        if lo.ndim != 2 or lo.shape != cnt.shape or lo.size == 0:
            raise ValueError("lo and cnt must be (K, J)")
        k, j = lo.shape
        if nrow % k:
            raise ValueError("one spectrum per channel and harmonic: nrow must be a multiple of K")
        if cnt.min() < 0 or lo.min() < 0 or int((lo.astype(np.int64) + cnt).max()) > nbins:
            raise ValueError("every band must lie inside the half spectrum")
        out = self.out_view(t.float64, nrow // k, k, j)
        if nrow:
            d_so, d_lo, d_cnt = self.job_tables(spec_off, lo.reshape(-1), cnt.reshape(-1))
            check(self.lib.ira_harmonic_band_powers(_ptr(spec_dev), _ptr(d_so), _ptr(d_lo), _ptr(d_cnt), nrow, k, j, nbins,
                                                    _ptr(out), self.stream), "ira_harmonic_band_powers")
        return out

    # ------------------------------------------------------------------ ISO 3382-1 noise handling (Lundeby)
    def lundeby_rows(self, base_off: np.ndarray, base_len: np.ndarray, chan_of_seg: np.ndarray, blk_size: np.ndarray,
                     nblk: np.ndarray, first_m: np.ndarray) -> Dict[str, object]:
        """The row tables block_energy, lundeby_estimate and edc_truncated share, checked on the host (lundeby_layout:
        ValueError before anything is uploaded or launched) and uploaded once.  Row j: base_len[j] samples at base_off[j] of
        the sample buffer, read from the start index of channel chan_of_seg[j] on; blk_size / nblk / first_m: B, nb, m0."""
        lay = lundeby_layout(base_off, base_len, chan_of_seg, blk_size, nblk, first_m)
        dev = self.job_tables(lay["base_off"], lay["base_len"], lay["chan_of_seg"], lay["blk_size"], lay["nblk"],
                              lay["first_m"], lay["blk_off"])
        lay["dev"] = dev
        return lay

    def block_energy(self, x_dev, rows, start_dev):
        """Float64 block energies (ira_block_energy): row j's nb + 1 values (the last one its partial tail block) at
        rows["blk_off"][j] of the returned device array."""
        t = self.torch
        n = rows["nseg"]
        blk = self.empty(rows["table_doubles"], t.float64)
        if n:
            d_off, d_len, d_ch, d_b, d_nb, _, d_boff = rows["dev"]
            check(self.lib.ira_block_energy(_ptr(x_dev), _ptr(d_off), _ptr(d_len), _ptr(d_ch), _ptr(start_dev), _ptr(d_b),
                                            _ptr(d_nb), _ptr(d_boff), n, rows["max_chunks"], _ptr(blk), self.stream),
                  "ira_block_energy")
        return blk

    def lundeby_estimate(self, rows, start_dev, blk_dev, compensate: bool = True):
        """Cross-point estimate per row (ira_lundeby_estimate).  Returns (records (nseg, LUNDEBY_DOUBLES) float64 device,
        curve lengths int64 device (nseg,), per-block suffix energies float64 device laid out like blk_dev)."""
        t = self.torch
        n = rows["nseg"]
        rec = self.out_view(t.float64, n, LUNDEBY_DOUBLES)
        lens = self.empty(n, t.int64)
        suffix = self.empty(rows["table_doubles"], t.float64)
        if n:
            _, d_len, d_ch, d_b, d_nb, d_m, d_boff = rows["dev"]
            check(self.lib.ira_lundeby_estimate(_ptr(d_len), _ptr(d_ch), _ptr(start_dev), _ptr(d_b), _ptr(d_nb), _ptr(d_m),
                                                _ptr(d_boff), n, _ptr(blk_dev), 1 if compensate else 0, _ptr(rec),
                                                _ptr(lens), _ptr(suffix), self.stream), "ira_lundeby_estimate")
        return rec, lens[:n], suffix

    def edc_truncated(self, x_dev, rows, start_dev, rec_dev, lens_dev, suffix_dev, eps: float, floor_db: float, edc_dev,
                      edc_off: np.ndarray) -> None:
        """The truncated, compensated float32 dB curve of every row (ira_edc_truncated) at edc_off[j] of edc_dev (float32
        device); nothing is written at or after the row's curve length.  edc_dev may be the sample buffer itself for a row
        whose curve replaces its own samples (edc_off[j] = the address of the row's start index)."""
        n = rows["nseg"]
        edc_off = np.ascontiguousarray(edc_off, dtype=np.int64)
        if edc_off.shape != (n,):
            raise ValueError("edc_off must be (nseg,)")
        if not (float(eps) >= 0.0) or math.isnan(float(floor_db)):
            raise ValueError("eps must be >= 0 and floor_db a number")
        if n:
            d_off, d_len, d_ch, d_b, d_nb, _, d_boff = rows["dev"]
            d_eoff, = self.job_tables(edc_off)
            check(self.lib.ira_edc_truncated(_ptr(x_dev), _ptr(d_off), _ptr(d_len), _ptr(d_ch), _ptr(start_dev), _ptr(d_b),
                                             _ptr(d_nb), _ptr(d_boff), n, rows["max_chunks"], _ptr(rec_dev), _ptr(lens_dev),
                                             _ptr(suffix_dev), float(eps), float(floor_db), _ptr(edc_dev), _ptr(d_eoff),
                                             self.stream), "ira_edc_truncated")

    # ------------------------------------------------------------------ multi-slope decay fits
    def multislope_points(self, rows, start_dev, blk_dev, fit_fraction: float):
        """The Schroeder points of every row of the block-energy tables (ira_multislope_points).  Returns (d float64 device,
        laid out like blk_dev; info int32 device (nseg, 2): row status and J; records float64 device
        (nseg, MS_MAX_ORDER, MS_DOUBLES), which multislope_search fills)."""
        t = self.torch
        n = rows["nseg"]
        if not 0.0 < float(fit_fraction) <= 1.0:
            raise ValueError("fit_fraction must satisfy 0 < fit_fraction <= 1")
        d = self.empty(rows["table_doubles"], t.float64)
        info = self.out_view(t.int32, n, 2)
        rec = self.out_view(t.float64, n, MS_MAX_ORDER, MS_DOUBLES)
        if n:
            _, d_len, d_ch, d_b, d_nb, _, d_boff = rows["dev"]
            check(self.lib.ira_multislope_points(_ptr(d_len), _ptr(d_ch), _ptr(start_dev), _ptr(d_b), _ptr(d_nb), _ptr(d_boff),
                                                 n, _ptr(blk_dev), float(fit_fraction), _ptr(d), _ptr(info), _ptr(rec),
                                                 self.stream), "ira_multislope_points")
        return d, info, rec

    def multislope_gram(self, rows, start_dev, d_dev, info_dev, jobs, grid_dev, grid_n_dev, grid_stride: int, ngrids: int,
                        max_g: int, sample_rate_hz: float, nslots: int, gram_dev=None):
        """Gram matrices and right-hand sides (ira_multislope_gram).  jobs (njobs, 3): row, grid slot, Gram slot.  Returns
        the float64 device array of nslots slots of multislope_slot_doubles(max_g) doubles (gram_dev if given)."""
        t = self.torch
        n = rows["nseg"]
        jobs = multislope_jobs(jobs, 3, n, ngrids, nslots, max_g)
        if int(grid_stride) < int(max_g):
            raise ValueError("grid_stride must be at least max_g")
        if not float(sample_rate_hz) > 0.0:
            raise ValueError("the sample rate must be positive")
        if gram_dev is None:
            gram_dev = self.empty(int(nslots) * multislope_slot_doubles(max_g), t.float64)
        if n and jobs.size:
            _, d_len, d_ch, d_b, d_nb, _, d_boff = rows["dev"]
            d_job, = self.job_tables(jobs.reshape(-1))
            check(self.lib.ira_multislope_gram(_ptr(d_len), _ptr(d_ch), _ptr(start_dev), _ptr(d_b), _ptr(d_nb), _ptr(d_boff), n,
                                               _ptr(d_dev), _ptr(info_dev), _ptr(d_job), int(jobs.shape[0]), _ptr(grid_dev),
                                               _ptr(grid_n_dev), int(grid_stride), int(ngrids), int(max_g),
                                               float(sample_rate_hz), int(nslots), _ptr(gram_dev), self.stream),
                  "ira_multislope_gram")
        return gram_dev

    def multislope_search(self, nseg: int, info_dev, jobs, grid_dev, grid_n_dev, grid_stride: int, ngrids: int, max_g: int,
                          gram_dev, nslots: int, min_ratio: float, rec_dev, refine_step: float = 0.0):
        """The candidate search (ira_multislope_search) into rec_dev (multislope_points' records).  jobs (njobs, 4): row,
        order, Gram slot, grid slot.  refine_step > 0: returns the next level's grids (float64 device
        (nseg * MS_MAX_ORDER, MS_REFINED)) and their sizes (int32 device), slot row * MS_MAX_ORDER + order - 1; else None."""
        t = self.torch
        n = int(nseg)
        jobs = multislope_jobs(jobs, 4, n, ngrids, nslots, max_g)
        if int(grid_stride) < int(max_g):
            raise ValueError("grid_stride must be at least max_g")
        if not float(min_ratio) > 1.0:
            raise ValueError("min_ratio must exceed 1")
        if not (float(refine_step) >= 0.0 and math.isfinite(float(refine_step))):
            raise ValueError("refine_step must be finite and >= 0")
        out = None
        if refine_step > 0.0:
            out = (self.empty(n * MS_MAX_ORDER * MS_REFINED, t.float64), self.empty(n * MS_MAX_ORDER, t.int32))
        if n and jobs.size:
            d_job, = self.job_tables(jobs.reshape(-1))
            check(self.lib.ira_multislope_search(n, _ptr(info_dev), _ptr(d_job), int(jobs.shape[0]), _ptr(grid_dev),
                                                 _ptr(grid_n_dev), int(grid_stride), int(ngrids), int(max_g), _ptr(gram_dev),
                                                 int(nslots), float(min_ratio), float(refine_step),
                                                 _ptr(out[0]) if out else 0, _ptr(out[1]) if out else 0, _ptr(rec_dev),
                                                 self.stream), "ira_multislope_search")
        return out

    # ------------------------------------------------------------------ suffix energies (quiet tails of the STFT calls)
    def tail_energy(self, x_dev, start: np.ndarray, end: np.ndarray) -> Dict[str, object]:
        """Float64 suffix energies (ira_tail_energy) of the segments [start[s], end[s]) of x_dev in blocks of TAIL_BLOCK
        samples: S[j] = sum of x^2 over [start[s] + j TAIL_BLOCK, end[s]), j <= nblk[s] = ceil((end - start) / TAIL_BLOCK), at
        off[s] of the returned table.  Returns dict(tab float64 device, off host, off_dev, nblk, start, end)."""
        t = self.torch
        start = np.ascontiguousarray(start, dtype=np.int64)
        end = np.ascontiguousarray(end, dtype=np.int64)
        n = int(start.size)
        if end.shape != start.shape or start.ndim != 1 or n > 65535:
            raise ValueError("start and end must be (nseg,) with nseg <= 65535")
        if n and (start.min() < 0 or np.any(end < start) or int(end.max()) > int(x_dev.numel())):
            raise ValueError("every segment must satisfy 0 <= start <= end <= the size of the sample buffer")
        nblk = -(-(end - start) // TAIL_BLOCK)
        if n and int(nblk.max()) >= 1 << 31:
            raise ValueError("segment too long")
        off = exclusive_cumsum(nblk + 1)
        tab = self.empty(int((nblk + 1).sum()), t.float64)
        d_off = None
        if n:
            d_start, d_end, d_off = self.job_tables(start, end, off)
            check(self.lib.ira_tail_energy(_ptr(x_dev), _ptr(d_start), _ptr(d_end), _ptr(d_off), n, int(nblk.max()),
                                           _ptr(tab), self.stream), "ira_tail_energy")
        return dict(tab=tab, off=off, off_dev=d_off, nblk=nblk, start=start, end=end)

    def tail_table(self, b: ChannelBatch, starts: np.ndarray) -> Dict[str, object]:
        """tail_energy of every channel of the batch from sample starts[i] of the channel to its end, computed once per
        batch and start vector: the blocks of a report step that trim alike (spectrogram, modal cloud) share one pass over
        the samples.  A block on another stream than the one the table was made on waits for it there."""
        t = self.torch
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        key = starts.tobytes()
        cur = t.cuda.current_stream(self.device) if self.device.type == "cuda" else None      # (None: a host-side engine)
        if b._tail is None or b._tail[0] != key:
            tab = self.tail_energy(b.x, b.off + starts, b.off + b.length)
            ev = None
            if cur is not None:
                ev = t.cuda.Event()
                ev.record(cur)
            b._tail = (key, tab, ev, cur)
            return tab
        _, tab, ev, made_on = b._tail
        if cur is not None and cur != made_on:
            cur.wait_event(ev)
            for buf in (tab["tab"], tab["off_dev"]):
                if buf is not None:
                    buf.record_stream(cur)
        return tab
