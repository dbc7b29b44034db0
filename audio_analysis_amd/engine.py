"""
Device engine: owns torch-ROCm tensors (device memory only), twiddle/window tables and the stream, and
calls the hand-written HIP kernels in libira.so through ctypes.  PyTorch is plumbing here -- no torch op
computes anything on the data path.

One Engine per process (= per GPU).  All entry points are batched over channels ("segments"); the
single-channel drop-in functions in audio_analysis_amd.analyse.* call them with a batch of one.
"""
from __future__ import annotations

import ctypes
import math
import os
from contextlib import contextmanager
from dataclasses import dataclass, fields
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import IraError, check
from .engine_plan import (SMOOTH, Switches, conv_size, exclusive_cumsum, pair_bands, plan_band_irfft,  # noqa: F401
                          plan_rfft)

FIT_DOUBLES = 8
EDC_SCRATCH_DOUBLES = 4096
EDC_TILE = 4096


def _ptr(t) -> int:
    return 0 if t is None else int(t.data_ptr())


def _unit_roots(count: int, period: int) -> np.ndarray:
    """exp(-2 pi i k / period), k < count: float64 (count, 2), interleaved (re, im)."""
    ang = -2.0 * np.pi * np.arange(count, dtype=np.float64) / float(period)
    return np.stack([np.cos(ang), np.sin(ang)], axis=1)


TAIL_BLOCK = 512              # IRA_TAIL_BLOCK: samples per block of ira_tail_energy's suffix energies
LUNDEBY_DOUBLES = 16          # IRA_LUNDEBY_DOUBLES
LUNDEBY_MAX_BLOCKS = 4096     # IRA_LUNDEBY_MAX_BLOCKS
LUNDEBY_STAGE = 4096          # samples a workgroup of the two sample passes stages; the largest block size
LUNDEBY_MAX_LEN = 2047 * 4096
MS_DOUBLES = 16               # IRA_MS_DOUBLES
MS_MAX_GRID = 128             # IRA_MS_MAX_GRID
MS_MAX_ORDER = 3              # IRA_MS_MAX_ORDER
MS_TILE = 32                  # IRA_MS_TILE: points of j a workgroup of ira_multislope_gram stages at a time
MS_REFINE_R = 3               # IRA_MS_REFINE_R
MS_REFINED = 21               # IRA_MS_REFINED: (2 R + 1) * MS_MAX_ORDER, the stride of the refined grids
ECHO_DOUBLES = 8              # IRA_ECHO_DOUBLES
ECHO_CHUNK = 4096             # IRA_ECHO_CHUNK: samples per workgroup of the two sample passes, counted from the onset
ECHO_MAX_LAG = 2048           # IRA_ECHO_MAX_LAG: the largest D (the halo the emit pass keeps of the chunk in front)
ECHO_MAX_PARAMS = 16          # IRA_ECHO_MAX_PARAMS
ECHO_PARAM_DOUBLES = 8        # IRA_ECHO_PARAM_DOUBLES
NED_DOUBLES = 8               # IRA_NED_DOUBLES
NED_TILE = 1024               # IRA_NED_TILE: positions a workgroup of ira_echo_density takes at a time when their span fits
NED_MAX_DELTA = 2048          # IRA_NED_MAX_DELTA: the largest half window (W = 2 delta + 1 <= 4097)
NED_MAX_THRESHOLDS = 3        # IRA_NED_MAX_THRESHOLDS
NED_NAN_SILENT = 0x7fc00000   # IRA_NED_NAN_SILENT: the profile's NaN where the window holds digital silence (B == 0)
NED_NAN_NONFINITE = 0x7fc00001  # IRA_NED_NAN_NONFINITE: the profile's NaN where B is not finite
NED_SLOTS = 5120              # float64 squares a workgroup stages (NED_SLOTS of ira_echodensity.hip)
REFL_DOUBLES = 8              # IRA_REFL_DOUBLES
REFL_FIELDS = 6               # IRA_REFL_FIELDS
REFL_TILE = 1024              # IRA_REFL_TILE: row entries a workgroup of ira_reflections takes
REFL_MAX_HALF = 512           # IRA_REFL_MAX_HALF: the largest half smoothing window (W = 2 d + 1 <= 1025)
REFL_MAX_DIRECT = 1024        # IRA_REFL_MAX_DIRECT
REFL_MAX_BG = 2048            # IRA_REFL_MAX_BG
REFL_MAX_KEEP = 64            # IRA_REFL_MAX_KEEP
REFL_MAX_SEP = 1024           # the largest separation S
REFL_UNBOUNDED = 1 << 40      # a Tn from here on is no bound (REFL_UNBOUNDED of ira_reflections.hip)
XSPEC_FRAMES = 16             # IRA_XSPEC_FRAMES: frames a workgroup of ira_xspec_accumulate sums before it writes
XSPEC_ROWS = 11               # IRA_XSPEC_ROWS
XSPEC_MIN_FFT, XSPEC_MAX_FFT = 256, 8192
FDW_FIELDS = 6                # IRA_FDW_FIELDS
FDW_SUMS = 5                  # IRA_FDW_SUMS
FDW_MAX_POINTS = 4096         # IRA_FDW_MAX_POINTS
FDW_MAX_HALF = 1 << 20        # IRA_FDW_MAX_HALF
FDW_CHUNK = 4096              # IRA_FDW_CHUNK: terms of a wide point a workgroup of ira_fdw_response sums
FDW_NARROW_HALF = 127         # IRA_FDW_NARROW_HALF: up to here one wavefront takes the point
FDW_WINDOWS = ("hann", "rect")
BURST_STEPS = 8               # IRA_BURST_STEPS: steps of a point a wavefront of ira_burst_decay serves from one walk
BURST_LANES = 64              # IRA_BURST_LANES: terms per round of that walk, one a lane
BURST_CHANNELS = 4            # IRA_BURST_CHANNELS: channels (waves) per workgroup
BURST_MAX_STEPS = 4096        # IRA_BURST_MAX_STEPS
BURST_MAX_DELTA = 1 << 24     # IRA_BURST_MAX_DELTA: the largest |delta| in samples
BURST_MAX_OUT_BYTES = 256 << 20  # Engine.burst_decay: one ira_burst_decay call writes at most this (the default map of 256 channels is 60 MB)
MINPHASE_FIELDS = 8           # IRA_MINPHASE_FIELDS: Re X, Im X, Im T at k - 1, k, k + 1, the unwrapped excess phase at k - 1, k, k + 1
MINPHASE_MAX_LOG2 = 21        # IRA_MINPHASE_MAX_LOG2
MINPHASE_MIN_N = 32           # the smallest transform of the chain
MINPHASE_MIN_FLOOR_DB = -300.0  # IRA_MINPHASE_MIN_FLOOR_DB
MINPHASE_SCRATCH_BYTES = 4 << 30  # minphase_cut: the device scratch of one sub-batch of the minimum-phase chain stays under this


def xspec_frames(n, n_fft: int, hop: int) -> np.ndarray:
    """K = 1 + (n - n_fft) // hop frames of n samples, 0 when n < n_fft (int64, elementwise)."""
    n = np.asarray(n, dtype=np.int64)
    return np.where(n >= n_fft, 1 + (n - n_fft) // hop, 0).astype(np.int64)


def ned_positions(length, onset, step: int, kmax: int) -> np.ndarray:
    """K = 0 if L <= o else min((L - 1 - o) // S + 1, Kmax) positions of a profile (int64, elementwise)."""
    length, onset = np.asarray(length, dtype=np.int64), np.asarray(onset, dtype=np.int64)
    return np.where(length > onset, np.minimum((length - 1 - onset) // int(step) + 1, int(kmax)), 0).astype(np.int64)


def ned_tile_positions(delta: int, step: int) -> int:
    """Positions a workgroup of ira_echo_density takes at a time (ned_geometry of ira_echodensity.hip, restated): NED_TILE
    when their span fits NED_SLOTS, fewer for large steps and windows.  No result depends on it; tests place K at its
    multiples."""
    w, s = 2 * int(delta) + 1, int(step)
    if 1 < s <= NED_SLOTS:
        wq = -(-w // s)
        t = min(NED_TILE, NED_SLOTS // s - wq + 1)
        while t >= 1 and s * ((t - 1 + wq) | 1) > NED_SLOTS:
            t -= 1
        if t >= 1:
            return t
    return min(NED_TILE, (NED_SLOTS - w) // s + 1)


def refl_row_room(length, direct: int, tn: int, background: int) -> np.ndarray:
    """Entries of a channel's energy-time row as the host sizes it, for onset 0: min(L, Rmax), Rmax = D + Tn + B, L for
    an unbounded Tn (int64, elementwise)."""
    length = np.clip(np.asarray(length, dtype=np.int64), 0, None)
    if int(tn) >= REFL_UNBOUNDED:
        return length.copy()
    return np.minimum(length, int(direct) + int(tn) + int(background)).astype(np.int64)


def refl_tile_candidates(separation: int) -> int:
    """Candidates a tile of REFL_TILE row entries can hold: two candidates lie more than S entries apart, so
    ceil(REFL_TILE / (S + 1)) (ira_reflections.hip restated)."""
    return (REFL_TILE + int(separation)) // (int(separation) + 1)


def refl_scratch_doubles(nch: int, max_room: int, separation: int) -> int:
    """Doubles of scratch ira_reflections needs: per channel and tile of the longest row a count and 4 doubles per
    candidate the tile can hold (the geometry of ira_reflections.hip restated; the call checks it)."""
    return int(nch) * (-(-int(max_room) // REFL_TILE)) * (1 + 4 * refl_tile_candidates(separation))


def fdw_chunks(half) -> np.ndarray:
    """Chunks of FDW_CHUNK terms of each point: ceil((2 H + 1) / FDW_CHUNK) for a wide point, 0 for a narrow one (H <=
    FDW_NARROW_HALF), which one wavefront sums without a partial (int64, elementwise)."""
    half = np.asarray(half, dtype=np.int64)
    return np.where(half > FDW_NARROW_HALF, -(-(2 * half + 1) // FDW_CHUNK), 0).astype(np.int64)


def fdw_scratch_doubles(nch: int, half) -> int:
    """Doubles of scratch ira_fdw_response needs (ira_fdw_scratch_doubles restated; the call checks it): FDW_SUMS per
    channel and chunk, then the int32 tables the plan launch builds (first chunk of each point and the total, the point
    of each chunk, the narrow points)."""
    chunks = fdw_chunks(half)
    total, narrow, npts = int(chunks.sum()), int(np.count_nonzero(chunks == 0)), int(chunks.size)
    return int(nch) * total * FDW_SUMS + (npts + 1 + total + narrow + 1) // 2


def burst_table_offsets(half) -> np.ndarray:
    """tab_off[j], the first entry of point j in the wavelet table of ira_burst_table: the points' 2 H + 1 entries lie one
    after the other (int64, exclusive running sum)."""
    half = np.asarray(half, dtype=np.int64).reshape(-1)
    return exclusive_cumsum(2 * half + 1).astype(np.int64)


def burst_table_doubles(half) -> int:
    """Doubles of the wavelet table (ira_burst_table_doubles restated; both calls check it): (re, im) per entry, 2 H + 1
    entries per point."""
    half = np.asarray(half, dtype=np.int64).reshape(-1)
    return 2 * int(np.sum(2 * half + 1))


def burst_channels_per_call(npts: int, nsteps: int) -> int:
    """Channels one ira_burst_decay call of Engine.burst_decay takes: as many as keep its output of 16 bytes per (channel,
    point, step) within BURST_MAX_OUT_BYTES, at least one, at most the 65535 of a launch."""
    return int(max(1, min(65535, BURST_MAX_OUT_BYTES // max(1, 16 * int(npts) * int(nsteps)))))


def minphase_scratch_bytes(n_fft) -> np.ndarray:
    """Device scratch of the minimum-phase chain per channel of transform size N, in bytes: X, G and T (16 (N/2 + 1) each),
    the cepstrum (4 N), the wrapped and the unwrapped excess phase (8 (N/2 + 1) each) and a transform's work array (8 N):
    44 N + 64, 92 MB at N = 2^21."""
    return 44 * np.asarray(n_fft, dtype=np.int64) + 64


def minphase_cut(n_fft) -> List[Tuple[int, int]]:
    """[(first, end), ..]: consecutive channels cut into sub-batches whose scratch (minphase_scratch_bytes) stays under
    MINPHASE_SCRATCH_BYTES; a channel that alone exceeds it is a sub-batch of its own."""
    need = minphase_scratch_bytes(n_fft).reshape(-1)
    cuts, first, total = [], 0, 0
    for i, b in enumerate(need.tolist()):
        if i > first and total + b > MINPHASE_SCRATCH_BYTES:
            cuts.append((first, i))
            first, total = i, 0
        total += b
    if need.size:
        cuts.append((first, int(need.size)))
    return cuts


def lundeby_layout(base_off, base_len, chan_of_seg, blk_size, nblk, first_m) -> Dict[str, object]:
    """Host side of the Lundeby row tables (pure NumPy): the tables in the kernels' types, every row's table offset
    blk_off = j * (max nb + 1), table_doubles = nseg * (max nb + 1) (what ira_lundeby_scratch_doubles answers) and
    max_chunks = max over the rows of ceil((nb + 1) / (4096 // B)), the grid width of the two sample passes.
    ValueError for tables the kernels would refuse."""
    base_off = np.ascontiguousarray(base_off, dtype=np.int64).reshape(-1)
    n = int(base_off.size)
    tabs = dict(base_off=base_off, base_len=np.ascontiguousarray(base_len, dtype=np.int64).reshape(-1),
                chan_of_seg=np.ascontiguousarray(chan_of_seg, dtype=np.int32).reshape(-1),
                blk_size=np.ascontiguousarray(blk_size, dtype=np.int32).reshape(-1),
                nblk=np.ascontiguousarray(nblk, dtype=np.int32).reshape(-1),
                first_m=np.ascontiguousarray(first_m, dtype=np.int32).reshape(-1))
    if any(v.size != n for v in tabs.values()):
        raise ValueError("base_off, base_len, chan_of_seg, blk_size, nblk and first_m must have one entry per row")
    if n > 65535:
        raise ValueError("at most 65535 rows per launch")
    b, nb = tabs["blk_size"].astype(np.int64), tabs["nblk"].astype(np.int64)
    if n and (b.min() < 1 or b.max() > LUNDEBY_STAGE):
        raise ValueError(f"block sizes must be 1 .. {LUNDEBY_STAGE} samples")
    if n and (nb.min() < 0 or nb.max() > LUNDEBY_MAX_BLOCKS):
        raise ValueError(f"block counts must be 0 .. {LUNDEBY_MAX_BLOCKS}")
    if n and tabs["first_m"].min() < 1:
        raise ValueError("first_m must be at least 1 block")
    if n and (tabs["base_len"].min() < 0 or tabs["base_len"].max() > LUNDEBY_MAX_LEN or np.any(nb * b > tabs["base_len"])):
        raise ValueError(f"rows must hold their nb * B samples and at most {LUNDEBY_MAX_LEN}")
    if n and tabs["chan_of_seg"].min() < 0:
        raise ValueError("chan_of_seg must index the start array")
    stride = int(nb.max()) + 1 if n else 1
    tabs["blk_off"] = np.arange(n, dtype=np.int64) * stride
    tabs["nseg"] = n
    tabs["stride"] = stride
    tabs["table_doubles"] = n * stride
    per_chunk = LUNDEBY_STAGE // np.maximum(b, 1)
    tabs["max_chunks"] = int(np.max(-(-(nb + 1) // per_chunk))) if n else 1
    return tabs


def multislope_slot_doubles(max_g: int) -> int:
    """Doubles of a Gram slot of ira_multislope_gram for grids of at most max_g decay times: the lower triangle over the
    g decays, the noise term and the constant 1."""
    return (int(max_g) + 2) * (int(max_g) + 3) // 2


def multislope_jobs(jobs, width: int, nseg: int, ngrids: int, nslots: int, max_g: int) -> np.ndarray:
    """A job table of ira_multislope_gram (width 3: row, grid slot, Gram slot) or ira_multislope_search (width 4: row,
    order, Gram slot, grid slot) as int32 (njobs, width), checked on the host: ValueError for an index out of range."""
    jobs = np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1, width)
    if not 1 <= int(max_g) <= MS_MAX_GRID:
        raise ValueError(f"a grid holds 1 .. {MS_MAX_GRID} decay times")
    if jobs.size:
        limits = (nseg, ngrids, nslots) if width == 3 else (nseg, MS_MAX_ORDER + 1, nslots, ngrids)
        lows = (0, 0, 0) if width == 3 else (0, 1, 0, 0)
        for col, (lo, hi) in enumerate(zip(lows, limits)):
            if jobs[:, col].min() < lo or jobs[:, col].max() >= hi:
                raise ValueError(f"column {col} of the job table must lie in [{lo}, {hi})")
    return jobs


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


@dataclass
class ChannelBatch:
    """A ragged batch of mono channels resident in HBM: flat float32 samples + per-channel offset/length."""
    x: "object"                  # torch.float32 (total,) on device
    off: np.ndarray              # int64 (B,) host
    length: np.ndarray           # int64 (B,) host
    off_dev: "object"
    len_dev: "object"
    peak: Optional[np.ndarray] = None       # int64 (B,) host, filled by Engine.peaks()
    peak_abs: Optional[np.ndarray] = None   # float32 (B,)
    ready: Optional[object] = None          # event recorded after the batch's arrays were enqueued for upload
    _peak_pending: Optional[tuple] = None   # Engine.peaks_begin(): pinned results + event, picked up by Engine.peaks()
    _tail: Optional[tuple] = None           # Engine.tail_table(): (key of the starts, table, event, stream it was made on)

    @property
    def count(self) -> int:
        return int(self.off.size)


class _TimedLib:
    """
    Transparent proxy over the ctypes library: when the engine's `events` list is set, every ira_* launch is
    bracketed by two HIP events recorded on the SAME stream the kernels are enqueued on, so per-call device
    time can be read back after a synchronise (bench.py's roofline uses this).
    """
    _PLAIN = {"ira_error_string", "ira_abi_version", "ira_ar_partial_doubles", "ira_ar_exact_doubles",
              "ira_energy_scratch_doubles", "ira_xcorr_scratch_doubles", "ira_echo_scratch_doubles"}

    def __init__(self, lib, eng):
        self._lib, self._eng, self._cache = lib, eng, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name in self._PLAIN or not name.startswith("ira_"):
            return fn
        if name not in self._cache:
            eng = self._eng

            def timed(*args, _fn=fn, _name=name):
                rec = eng.events
                if rec is None:
                    return _fn(*args)
                t = eng.torch
                stream = t.cuda.current_stream(eng.device)
                e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc = _fn(*args)
                e1.record(stream)
                rec.append((_name + eng.event_tag, e0, e1))
                return rc

            self._cache[name] = timed
        return self._cache[name]


class HostFuture:
    """Result of Engine.fetch(): a device tensor on its way into pinned host memory.  get() is valid once the
    stream it was enqueued on has reached the copy (Engine.sync(), or the event of the step it belongs to).
    The first get() (or the future's destruction) hands its slice of the fetch arena back to the engine."""

    def __init__(self, pinned, shape, owner=None, segment=None):
        self._pinned, self._shape, self._owner, self._segment = pinned, shape, owner, segment

    def _release(self):
        if self._owner is not None:
            self._owner._fetch_release(self._segment)
            self._owner = None

    def get(self) -> np.ndarray:
        out = self._pinned.numpy().reshape(self._shape).copy()
        self._release()
        return out

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


def _TORCH_DTYPES(t):
    return {"<i8": t.int64, "<i4": t.int32, "<f8": t.float64, "<f4": t.float32, "|u1": t.uint8, "<i2": t.int16}


_ENGINE = None


def get_engine() -> "Engine":
    """Process-wide engine on the current CUDA/HIP device.  Raises if there is no GPU or no libira.so."""
    global _ENGINE
    if _ENGINE is None:
        _ENGINE = Engine()
    return _ENGINE


class Engine:
    # ------------------------------------------------------------------ A/B switches and budgets
    # Class defaults; assign on an engine to take the alternative path (tests/test_gpu_longfft.py checks every default
    # path against its alternative).  The environment overrides of some of them are read in _init_state.
    #
    # A channel's transforms are its own.  Round 2 let two real signals of equal length from DIFFERENT channels share one
    # complex transform (z = x1 + i*x2) and the odd band of one channel share an inverse with the odd band of another:
    # cheaper by half, but then the last bits of a channel's spectrum depend on which channel happened to be its partner,
    # i.e. on batch composition and shard boundaries (SURVEY.md section 8e asks for byte-identical records for every
    # world size).  Now a single real signal of EVEN length rides a HALF-length complex transform instead (x[2m] + i
    # x[2m+1]: the same saving), bands are paired only within one channel, and an odd band out takes the half-length
    # inverse.  pair_across_channels = True restores round 2's pairing (A/B; results then agree to ~1e-16 of the larger
    # signal, not bit for bit).  pair_real_ffts = False additionally forbids pairing the bands of one channel.
    pair_real_ffts = True
    pair_across_channels = False
    # A real signal of EVEN (non-smooth) length L is transformed as the complex sequence x[2m] + i*x[2m+1] of length
    # L/2 (half the Bluestein convolution size) and split with a twiddle.  Set False for an A/B.
    half_real_ffts = True
    # The untangling X[k] = E[k] + W^k O[k] of such a half-length transform happens where Z[k] and Z[n - k] already meet:
    # in the second pass of the direct transform (smooth lengths), and in the dB / phase kernel for the Bluestein spectra of
    # the fr / filter blocks (packed spectra).  False restores round 3's separate split passes (A/B).
    fuse_half_split = True
    # Band inverses of smooth lengths: jobs whose bands span few bins (third-octave bands below ~800 Hz of a 10 s file)
    # skip the first pass and the n-point work array (ira_band_irfft_smooth, job_info_dev).  False = both passes for every
    # job (A/B).
    sparse_bands = True
    # Lengths of the form 2^a 3^b 5^c that split into two factors <= 1024 (480000, 2^19, ...) take the direct two-pass
    # mixed-radix transform (ira_rfft_smooth / ira_band_irfft_smooth) instead of Bluestein.  Set False for an A/B.
    smooth_ffts = True
    # Convolution sizes the Bluestein kernels take: 2^k and 3 * 2^k.  three_pow2_sizes = False restricts the choice to
    # powers of two (round 2's behaviour; A/B).
    three_pow2_sizes = True
    # round 5: the band inverses can leave the energies of their signals' EDC tiles for ira_edc_fits, which then reads a
    # band signal once less.  Measured (profiles/r05_tile_energies.txt, config 3): ira_edc_fits 6.66 -> 5.40 ms per step,
    # but the second pass pays 1.6 ms for forming the partials (a serial tail of every tile): 28.2 -> 28.6 ms of device
    # time.  OFF by default; IRA_BAND_TILE_ENERGIES=1 / this attribute is the A/B switch.
    band_tile_energies = False
    # Normal equations lose cond(A)^2 eps; above this cond(G) estimate the fit gets refinement steps (ira_ar_refine).
    # Rank-deficient Gram matrices (Cholesky pivot <= 0) get the minimum-norm solution lstsq returns (ira_ar_minnorm):
    # eigen-directions with lambda <= cut * lambda_max are dropped.  0 disables the fallback.
    ar_minnorm_cut = 1e-12
    # A/B: form the Gram matrix as a dense contraction on the FP64 matrix cores (IRA_AR_DENSE_GRAM) instead of the lag sums
    ar_dense_gram = False
    # A/B: the 256-thread solve kernel also for order <= 64 (default there since round 4: one wave per element, same bits)
    ar_workgroup_solve = False
    ar_refine_cond = 1e9          # on the estimate trace(G) ||G^-1|| (<= order * cond(G))
    ar_refine_steps = 2
    # Above this estimate (or when the float64 Cholesky breaks down) the normal equations are solved again in double-double
    # arithmetic (ira_ar_exact): refinement needs cond(G) eps << 1.  0 disables the path (A/B).
    ar_exact_cond = 1e13
    # Chirp-filter spectra depend only on (length, M): they are PLAN data, like twiddle tables, and are kept in LRU pools
    # of device slots -- one pool per (M, stream), all pools together within filter_cache_bytes -- so that repeated
    # lengths (every step of a batch job, every band pair of a file) do not rebuild them.  A pool starts at twice the
    # slots its first call needs and doubles when a call needs more; when the budget is full the pools used least
    # recently are dropped.  filter_cache_bytes = 0 disables the cache.
    filter_cache_bytes = 16 << 30
    workspace_budget_bytes = 48 << 30   # cap for the Bluestein work + filter arrays of one chunk

    def __init__(self, device: Optional[str] = None):
        import torch

        lib = _TimedLib(_lib.load(), self)
        if not torch.cuda.is_available():
            raise IraError("audio_analysis_amd needs an AMD GPU (torch.cuda.is_available() is False); "
                           "there is no CPU fallback for the product path.")
        self._init_state(torch, torch.device(device) if device is not None
                         else torch.device("cuda", torch.cuda.current_device()), lib)

    def _init_state(self, torch, device, lib) -> None:
        """Every attribute an engine has, and every environment switch it reads (the whole of construction but for the
        GPU check: tests/host_engine.py builds an engine on host memory through this)."""
        self.torch, self.device, self.lib = torch, device, lib
        self.events = None          # list of (name, start_event, end_event) while timing is on
        self.event_tag = ""
        self._tables: Dict[Tuple, object] = {}          # _cached: tables on the device, and host facts about sizes
        self._filter_pools: Dict[tuple, dict] = {}      # (M, stream) -> pool, see _filter_pool
        self._filter_tick = 0
        self._ring = self._ring_np = None               # pinned staging ring of to_dev, allocated by its first use
        self._ring_pos = 0
        self._fetch_arena = None                        # pinned arena of fetch, allocated by its first use
        self._fetch_seg, self._fetch_pos, self._fetch_out = 0, 0, [0] * self._FETCH_SEGMENTS
        self._side = None                               # side_stream()
        self._lanes = None                              # block_streams()
        self.last_band_info = ()
        self.last_band_info_half = ()
        env = os.environ.get
        # IRA_STREAMS: how many lanes block_streams() deals the report blocks onto (1 = the caller's stream only)
        self.num_lanes = max(1, min(4, int(env("IRA_STREAMS", "2"))))
        # which report blocks go to which lane (pipeline.FullReport.submit; None = its measured default).  IRA_LANE_DEAL, e.g.
        # "0,1|4,3,5,2", is the A/B switch of tools: 0 bands, 1 spectrum, 2 zplane, 3 decay, 4 modal, 5 stft
        self.lane_deal = ([[int(v) for v in part.split(",")] for part in env("IRA_LANE_DEAL").split("|")]
                          if env("IRA_LANE_DEAL") else None)
        # IRA_LANE_PRIO (A/B only), e.g. "-1,0": HIP stream priorities of the lanes (lower = served first)
        self._lane_prio = [int(v) for v in env("IRA_LANE_PRIO", "").split(",") if v.strip()]
        if env("IRA_BAND_TILE_ENERGIES") is not None:
            self.band_tile_energies = env("IRA_BAND_TILE_ENERGIES") == "1"
        if env("IRA_WORKSPACE_MB"):                       # tuning knob: long-FFT jobs per launch (see workspace_budget_bytes)
            self.workspace_budget_bytes = int(float(env("IRA_WORKSPACE_MB")) * (1 << 20))

    @contextmanager
    def tagged(self, tag: str):
        """Name the timed launches enqueued inside the block `<call><tag>` (bench.py's per-call device times); the tag in
        force before is back on ANY exit, so a refused call does not mislabel the launches after it."""
        saved, self.event_tag = self.event_tag, tag
        try:
            yield
        finally:
            self.event_tag = saved

    # ------------------------------------------------------------------ plumbing
    @property
    def stream(self) -> int:
        return int(self.torch.cuda.current_stream(self.device).cuda_stream)

    def collect_events(self):
        """Synchronise and return {call name: [milliseconds, ...]} for the launches recorded so far."""
        self.sync()
        out = {}
        for name, e0, e1 in (self.events or []):
            out.setdefault(name, []).append(float(e0.elapsed_time(e1)))
        if self.events is not None:
            self.events = []
        return out

    def sync(self) -> None:
        self.torch.cuda.current_stream(self.device).synchronize()

    # Small host arrays (offsets, lengths, job tables) go through a pinned staging ring and an ASYNC copy: a
    # pageable .to(device) blocks the host until the stream has drained, which would serialise host and GPU.
    _RING_BYTES = 32 << 20
    _ASYNC_LIMIT = 1 << 20

    def to_dev(self, a: np.ndarray):
        t = self.torch
        a = np.ascontiguousarray(a)
        nbytes = a.nbytes
        if nbytes == 0 or nbytes > self._ASYNC_LIMIT:
            return t.from_numpy(a).to(self.device, non_blocking=False)
        if self._ring is None:
            self._ring = t.empty(self._RING_BYTES, dtype=t.uint8).pin_memory()
            self._ring_np = self._ring.numpy()
        pos = (self._ring_pos + 63) & ~63
        if pos + nbytes > self._RING_BYTES:
            t.cuda.synchronize(self.device)  # every copy issued so far (on any stream) has left the ring before it wraps
            pos = 0
        self._ring_np[pos : pos + nbytes] = a.view(np.uint8).reshape(-1)
        self._ring_pos = pos + nbytes
        src = self._ring[pos : pos + nbytes].view(_TORCH_DTYPES(t)[a.dtype.str]).view(a.shape)
        # (round 5: the same copy as a bare hipMemcpyAsync (ctypes) into a device ring that mirrors this one -- no tensor
        # allocation, no dispatcher -- was built and measured: the same ~85 us of host time per call, which is the runtime's
        # own cost of a small asynchronous copy; 11.9-12.1 vs 11.9-12.3 ms per bundle step.  Removed.)
        return src.to(self.device, non_blocking=True)

    def job_tables(self, *arrays):
        """The job tables of ONE call (offsets, lengths, indices ... read only by the launches the calling method enqueues
        before it returns): several small host arrays -> ONE write into the pinned staging ring and ONE asynchronous H2D
        copy; returns the device views in order (None entries stay None).  They used to be one copy each: 65 copy-engine
        operations of ~5 us per report step (profiles/r02_*: __amd_rocclr_copyBuffer), each serialised with the kernels
        of its stream."""
        t = self.torch
        items = [(i, np.ascontiguousarray(a)) for i, a in enumerate(arrays) if a is not None]
        total = sum(((a.nbytes + 15) & ~15) for _, a in items)
        if not items or total == 0 or total > self._ASYNC_LIMIT or any(a.nbytes == 0 for _, a in items):
            return [None if a is None else self.to_dev(a) for a in arrays]
        blob = np.zeros(total, dtype=np.uint8)
        spans, pos = [], 0
        for i, a in items:
            blob[pos : pos + a.nbytes] = a.view(np.uint8).reshape(-1)
            spans.append((i, pos, a))
            pos += (a.nbytes + 15) & ~15
        dev = self.to_dev(blob)
        out = [None] * len(arrays)
        for i, pos, a in spans:
            out[i] = dev[pos : pos + a.nbytes].view(_TORCH_DTYPES(t)[a.dtype.str]).view(a.shape)
        return out

    def empty(self, n: int, dtype):
        return self.torch.empty(int(max(n, 1)), dtype=dtype, device=self.device)

    # Small results (fit records, statistics, roots) leave through a pinned arena with ASYNC copies, so that a step's
    # device->host traffic is enqueued with its kernels and read after ONE wait -- and so that the next step can be
    # enqueued behind it (audio_analysis_amd.pipeline.FullReport.submit / finish).  The arena is cut into segments that
    # are filled front to back; a segment is reused only when every future carved from it has been read (or dropped):
    # an unread result is never overwritten, however many steps are in flight or however large their records are.
    # When no segment is free the copy gets a private pinned allocation (slower, never wrong).
    _FETCH_BYTES = 96 << 20
    _FETCH_SEGMENTS = 6

    def _fetch_release(self, segment: int) -> None:
        self._fetch_out[segment] -= 1

    def fetch(self, tensor) -> HostFuture:
        t = self.torch
        tensor = tensor.contiguous()
        nbytes = int(tensor.numel()) * tensor.element_size()
        seg_bytes = self._FETCH_BYTES // self._FETCH_SEGMENTS
        if self._fetch_arena is None:
            self._fetch_arena = t.empty(self._FETCH_BYTES, dtype=t.uint8).pin_memory()
        pos = (self._fetch_pos + 63) & ~63
        seg = self._fetch_seg
        if nbytes <= seg_bytes and pos + nbytes > seg_bytes:
            # current segment is full: move on to the next one if everything carved from it has been consumed
            nxt = (seg + 1) % self._FETCH_SEGMENTS
            if self._fetch_out[nxt] == 0:
                seg, pos = nxt, 0
                self._fetch_seg = nxt
        if (nbytes > seg_bytes or pos + nbytes > seg_bytes
                or (pos == 0 and self._fetch_out[seg] != 0)):    # (only reachable on the very first wrap with stale futures)
            host = t.empty(tensor.shape, dtype=tensor.dtype).pin_memory()
            host.copy_(tensor, non_blocking=True)
            return HostFuture(host, tuple(tensor.shape))
        self._fetch_pos = pos + nbytes
        self._fetch_out[seg] += 1
        base = seg * seg_bytes + pos
        host = self._fetch_arena[base : base + nbytes].view(tensor.dtype).view(tensor.shape)
        host.copy_(tensor, non_blocking=True)
        return HostFuture(host, tuple(tensor.shape), self, seg)

    def side_stream(self):
        """High-priority stream for the tiny peak-pick launch whose result the HOST needs before it can lay out a
        step: it overtakes whatever the main stream still has queued from the previous step."""
        if self._side is None:
            self._side = self.torch.cuda.Stream(device=self.device, priority=-1)
        return self._side

    def block_streams(self):
        """
        Compute streams ("lanes") for independent report blocks (pipeline.FullReport).  The many small-grid,
        latency-bound kernels of one lane (curve fits, Cholesky solves, root finders, unwrap scans) run beside another
        lane's wide kernels instead of leaving most CUs idle, and the launch gaps of one lane are covered by the others.
        Every lane has its own chirp-filter plan pool (_filters); tables are uploaded synchronously (_table_to_dev).
        IRA_STREAMS=1 keeps everything on the caller's stream (A/B switch); default 2 (round 3, 256 x 10 s per step: 1 lane
        12.4 k, 2 lanes 13.4 k, 3 lanes 11.6-12.3 k IRs/s; round 1 measured 3 lanes best at 64 per step, when the small
        latency-bound kernels were a fifth of the step).
        """
        if self.num_lanes <= 1:
            return None
        if self._lanes is None or len(self._lanes) != self.num_lanes:
            prio = self._lane_prio
            self._lanes = tuple(self.torch.cuda.Stream(device=self.device, priority=(prio[i] if i < len(prio) else 0))
                                for i in range(self.num_lanes))
        return self._lanes

    def upload(self, channels: Sequence[np.ndarray]) -> ChannelBatch:
        """Host float32 channels -> one flat device buffer (H2D)."""
        lens = np.array([int(c.size) for c in channels], dtype=np.int64)
        off = exclusive_cumsum(lens)
        flat = np.empty(int(lens.sum()), dtype=np.float32)
        for c, o, n in zip(channels, off, lens):
            if c.ndim != 1:
                raise ValueError("expects 1D mono arrays")
            flat[o : o + n] = c.astype(np.float32, copy=False)
        return self.wrap(self.to_dev(flat), off, lens)

    def subset(self, b: ChannelBatch, idx: np.ndarray) -> ChannelBatch:
        """The channels idx of a batch as a batch of their own: same sample buffer, their offsets / lengths / peaks.
        (Its ready event is recorded behind the new offset/length uploads; the samples themselves are already resident:
        whoever knows the peaks has waited for the batch's upload.)"""
        idx = np.asarray(idx, dtype=np.int64)
        sub = self.wrap(b.x, b.off[idx], b.length[idx])
        if b.peak is not None:
            sub.peak = b.peak[idx].copy()
            sub.peak_abs = b.peak_abs[idx].copy() if b.peak_abs is not None else None
        return sub

    def wrap(self, x_dev, off: np.ndarray, lens: np.ndarray) -> ChannelBatch:
        off = np.ascontiguousarray(off, dtype=np.int64)
        lens = np.ascontiguousarray(lens, dtype=np.int64)
        d_off, d_len = self.job_tables(off, lens)
        b = ChannelBatch(x=x_dev, off=off, length=lens, off_dev=d_off, len_dev=d_len)
        b.ready = self.torch.cuda.Event()
        b.ready.record(self.torch.cuda.current_stream(self.device))
        return b

    # ------------------------------------------------------------------ tables (host NumPy -> device, cached)
    def _cached(self, key: tuple, make):
        """Plan data (tables, and what the library answers about a size) is made once per engine: make() on first use."""
        if key not in self._tables:
            self._tables[key] = make()
        return self._tables[key]

    def _table_to_dev(self, a: np.ndarray, precision: int = 64):
        """Plan data (windows, twiddles): uploaded once and COMPLETELY before use -- tables are shared by every stream."""
        tab = self.to_dev(a.astype(np.float32) if precision == 32 else a)
        self.sync()
        return tab

    def window(self, n: int, use_hann: bool, precision: int):
        return self._cached(("win", n, bool(use_hann), precision), lambda: self._table_to_dev(
            np.hanning(n).astype(np.float64) if use_hann else np.ones(n, dtype=np.float64), precision))

    def twiddle(self, n: int, precision: int):
        """exp(-2 pi i k / n), k < n/2, interleaved (re, im)."""
        return self._cached(("tw", n, precision), lambda: self._table_to_dev(_unit_roots(n // 2, n), precision))

    # ------------------------------------------------------------------ a2
    def _peak_pick(self, x_dev, d_off, d_len, n: int, max_len: int):
        """argmax|x| (int64) and max|x| (float32) of n segments, enqueued on the current stream: two device tensors."""
        t = self.torch
        pk, pa = self.empty(n, t.int64), self.empty(n, t.float32)
        check(self.lib.ira_peak_index(_ptr(x_dev), _ptr(d_off), _ptr(d_len), n, max_len, _ptr(pk), _ptr(pa), self.stream),
              "ira_peak_index")
        return pk, pa

    def _batch_peak_pick(self, b: ChannelBatch):
        return self._peak_pick(b.x, b.off_dev, b.len_dev, b.count, int(b.length.max()) if b.count else 0)

    def peaks_begin(self, b: ChannelBatch) -> None:
        """Enqueue the peak pick of a batch on the high-priority side stream (behind the batch's upload only) and its
        result's copy into pinned memory, WITHOUT waiting: the host can do other work while a freshly uploaded batch is
        still on its way.  peaks() picks the result up."""
        if b.peak is not None or b._peak_pending is not None:
            return
        t = self.torch
        side = self.side_stream()
        if b.ready is not None:
            side.wait_event(b.ready)
        with t.cuda.stream(side):
            pk, pa = self._batch_peak_pick(b)
            hk = t.empty(pk.shape, dtype=pk.dtype, pin_memory=True)
            ha = t.empty(pa.shape, dtype=pa.dtype, pin_memory=True)
            hk.copy_(pk, non_blocking=True)
            ha.copy_(pa, non_blocking=True)
            ev = t.cuda.Event()
            ev.record(side)
        b._peak_pending = (hk, ha, ev, pk, pa)

    def peaks(self, b: ChannelBatch) -> np.ndarray:
        """argmax|x| per channel (first max wins), synchronises once and caches on the batch."""
        if b.peak is None and b._peak_pending is not None:
            hk, ha, ev, _, _ = b._peak_pending
            ev.synchronize()
            b.peak = hk.numpy()[: b.count].copy()
            b.peak_abs = ha.numpy()[: b.count].copy()
            b._peak_pending = None
        if b.peak is None:
            pk, pa = self._batch_peak_pick(b)
            b.peak = pk.cpu().numpy()[: b.count].copy()
            b.peak_abs = pa.cpu().numpy()[: b.count].copy()
        return b.peak

    # ------------------------------------------------------------------ a3
    def edc_db(self, x_dev, seg_off: np.ndarray, seg_len: np.ndarray, eps: float, floor_db: float,
               want_f64: bool = False):
        """Schroeder EDC in dB for segments of x_dev.  Returns (edc flat f32 device, edc_off host int64[, f64])."""
        t = self.torch
        n = int(seg_off.size)
        if np.any(seg_len > 2047 * EDC_TILE):
            raise ValueError("segment too long for the EDC kernel (> 8.3 M samples)")
        edc_off = exclusive_cumsum(seg_len)
        out = self.empty(int(seg_len.sum()), t.float32)
        out64 = self.empty(int(seg_len.sum()), t.float64) if want_f64 else None
        scratch = self.empty(n * EDC_SCRATCH_DOUBLES, t.float64)
        # NOTE: device temporaries must stay referenced until the call is enqueued (the caching allocator
        # would otherwise hand the same block to the next to_dev()).
        d_off, d_len, d_eoff = self.job_tables(seg_off, seg_len, edc_off)
        check(self.lib.ira_edc_db(_ptr(x_dev), _ptr(d_off), _ptr(d_len), n, int(seg_len.max()), float(eps),
                                  float(floor_db), _ptr(out),
                                  _ptr(out64), _ptr(d_eoff), _ptr(scratch), self.stream), "ira_edc_db")
        if want_f64:
            return out, edc_off, out64
        return out, edc_off

    def edc_box_smooth(self, edc64_dev, off: np.ndarray, lens: np.ndarray, window: int, floor_db: float):
        """Box smoothing of unfloored float64 dB curves + floor + float32 cast (ira_edc_box_smooth)."""
        t = self.torch
        lens = np.ascontiguousarray(lens, dtype=np.int64)
        out = self.empty(int(lens.sum()), t.float32)
        d_off, d_len = self.job_tables(np.ascontiguousarray(off, np.int64), lens)
        check(self.lib.ira_edc_box_smooth(_ptr(edc64_dev), _ptr(d_off), _ptr(d_len), int(lens.size), int(lens.max()),
                                          int(window), float(floor_db), _ptr(out), self.stream), "ira_edc_box_smooth")
        return out

    # ------------------------------------------------------------------ a3-a6 fused
    def edc_fits(self, x_dev, seg_off: np.ndarray, seg_len: np.ndarray, eps: float, floor_db: float,
                 t_mul: float, t_div: float, ranges: Sequence[Tuple[float, float]], min_points: int,
                 cross: Sequence[float] = (), want_edc: bool = False, tiles=None):
        """Schroeder EDC crossings + decay-line fits straight from the samples (ira_edc_fits).
        Returns (fits (n, nranges, 8) f64 device | None, cross (n, ncross) f64 device | None, edc f32 device | None,
        edc_off host int64): the EDC curve is only written when want_edc.
        tiles = (part device, part_off int64, part_wgs int32, part_tiles int32 per segment): partial tile energies the producer of
        the segments left behind (band_irfft(want_tiles=True)); every such segment must END where its signal ends."""
        t = self.torch
        n = int(seg_off.size)
        seg_len = np.ascontiguousarray(seg_len, dtype=np.int64)
        if np.any(seg_len > 2047 * EDC_TILE):
            raise ValueError("segment too long for the EDC kernel (> 8.3 M samples)")
        edc_off = exclusive_cumsum(seg_len)
        fit, cr, c_ranges, c_cross, views = self._fit_outputs(n, ranges, cross)
        out = self.empty(int(seg_len.sum()), t.float32) if want_edc else None
        scratch = self.empty(n * EDC_SCRATCH_DOUBLES, t.float64)
        part, p_off, p_wgs, p_tiles = tiles if tiles is not None else (None, None, None, None)
        d_off, d_len, d_eoff, d_poff, d_pwgs, d_ptiles = self.job_tables(
            np.ascontiguousarray(seg_off, np.int64), seg_len, edc_off if want_edc else None,
            None if part is None else np.ascontiguousarray(p_off, np.int64),
            None if part is None else np.ascontiguousarray(p_wgs, np.int32),
            None if part is None else np.ascontiguousarray(p_tiles, np.int32))
        check(self.lib.ira_edc_fits(_ptr(x_dev), _ptr(d_off), _ptr(d_len), n, int(seg_len.max()) if n else 0,
                                    float(eps), float(floor_db), float(t_mul), float(t_div), c_ranges, len(ranges),
                                    int(min_points), c_cross, len(cross), _ptr(fit), _ptr(cr), _ptr(out),
                                    _ptr(d_eoff), _ptr(scratch), _ptr(part), _ptr(d_poff), _ptr(d_pwgs), _ptr(d_ptiles),
                                    self.stream),
              "ira_edc_fits")
        return views + (out, edc_off)

    def _scratch(self, sizer: str, *shape):
        """Float64 device scratch of the size the library's entry point `sizer` states for `shape` (a negative answer is
        its status code)."""
        nsc = int(getattr(self.lib, sizer)(*shape))
        check(min(nsc, 0), sizer)
        return self.empty(nsc, self.torch.float64)

    def _fit_outputs(self, n: int, ranges: Sequence[Tuple[float, float]], cross: Sequence[float]):
        """What ira_edc_fits and ira_curve_fits share: the record arrays fit (n, nranges, 8) and cr (n, ncross) (float64
        device, at least one record each), the fit ranges and crossing levels as C double arrays, and the result views
        (fits | None, cross | None)."""
        t = self.torch
        nr, nc = len(ranges), len(cross)
        fit = self.empty(n * max(nr, 1) * FIT_DOUBLES, t.float64)
        cr = self.empty(n * max(nc, 1), t.float64)
        views = (fit[: n * nr * FIT_DOUBLES].view(n, nr, FIT_DOUBLES) if nr else None,
                 cr[: n * nc].view(n, nc) if nc else None)
        return fit, cr, _lib.dbl_array([v for r in ranges for v in r]), _lib.dbl_array(list(cross)), views

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
        base_off = np.ascontiguousarray(base_off, dtype=np.int64)
        base_len = np.ascontiguousarray(base_len, dtype=np.int64)
        nseg = int(base_off.size)
        limits = np.ascontiguousarray(limits, dtype=np.int64)
        if limits.ndim != 2 or limits.shape[0] != nseg:
            raise ValueError("limits must be (nseg, nlim)")
        nlim = int(limits.shape[1])
        max_len = int(base_len.max()) if nseg else 0
        scratch = self._scratch("ira_energy_scratch_doubles", nseg, max_len, nlim)
        out = self.empty(nseg * (nlim + 2), t.float64)
        d_off, d_len, d_ch, d_lim = self.job_tables(base_off, base_len, np.ascontiguousarray(chan_of_seg, np.int32),
                                                    limits.reshape(-1))
        check(self.lib.ira_energy_windows(_ptr(x_dev), _ptr(d_off), _ptr(d_len), _ptr(d_ch), _ptr(onset_dev), nseg,
                                          max_len, _ptr(d_lim), nlim, _ptr(scratch), _ptr(out), self.stream),
              "ira_energy_windows")
        return out[: nseg * (nlim + 2)].view(nseg, nlim + 2)

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
        base_off = np.ascontiguousarray(base_off, dtype=np.int64)
        base_len = np.ascontiguousarray(base_len, dtype=np.int64)
        param_of_seg = np.ascontiguousarray(param_of_seg, dtype=np.int32)
        params = np.ascontiguousarray(params, dtype=np.float64)
        nseg = int(base_off.size)
        if params.ndim != 2 or params.shape[1] != ECHO_PARAM_DOUBLES or not 1 <= params.shape[0] <= ECHO_MAX_PARAMS:
            raise ValueError(f"params must be (1..{ECHO_MAX_PARAMS}, {ECHO_PARAM_DOUBLES})")
        if base_len.size != nseg or param_of_seg.size != nseg or len(chan_of_seg) != nseg:
            raise ValueError("base_off, base_len, chan_of_seg and param_of_seg must be (nseg,)")
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
        rec = self.empty(nseg * ECHO_DOUBLES, t.float64)
        curve = self.empty(nseg * ncurve, t.float32)
        d_off, d_len, d_ch, d_par = self.job_tables(base_off, base_len, np.ascontiguousarray(chan_of_seg, np.int32),
                                                    param_of_seg)
        with self.tagged("[stash]" if self.echo_stash else self.event_tag):
            check(self.lib.ira_echo_criterion(_ptr(x_dev), _ptr(d_off), _ptr(d_len), _ptr(d_ch), _ptr(d_par),
                                              _ptr(onset_dev), nseg, max_len, _lib.dbl_array(params.reshape(-1)),
                                              int(params.shape[0]), ncurve, _ptr(scratch),
                                              _ptr(stash), _ptr(rec), _ptr(curve), self.stream), "ira_echo_criterion")
        return rec[: nseg * ECHO_DOUBLES].view(nseg, ECHO_DOUBLES), curve[: nseg * ncurve].view(nseg, ncurve)

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
        off = np.ascontiguousarray(off, dtype=np.int64).reshape(-1)
        length = np.ascontiguousarray(length, dtype=np.int64).reshape(-1)
        weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        delta, step, kmax = int(delta), int(step), int(kmax)
        nch = int(off.size)
        if length.size != nch:
            raise ValueError("off and length must be (nch,)")
        if not 1 <= delta <= NED_MAX_DELTA:
            raise ValueError(f"delta must be 1..{NED_MAX_DELTA} samples, got {delta}")
        if weights.size != 2 * delta + 1 or not (np.all(np.isfinite(weights)) and np.all(weights > 0.0)):
            raise ValueError("weights must be 2 * delta + 1 finite values > 0")
        if not (1 <= step < 1 << 31 and 0 <= kmax <= 1 << 31):
            raise ValueError("step must be >= 1 and kmax 0..2^31")
        thresholds = [float(v) for v in thresholds]
        if len(thresholds) > NED_MAX_THRESHOLDS:
            raise ValueError(f"at most {NED_MAX_THRESHOLDS} thresholds")
        room = ned_positions(length, 0, step, kmax)
        prof_off = exclusive_cumsum(room)
        total = int(room.sum())
        prof = self.empty(total, t.float32)
        rec = self.empty(nch * NED_DOUBLES, t.float64)
        d_off, d_len, d_poff, d_w = self.job_tables(off, length, prof_off, weights)
        check(self.lib.ira_echo_density(_ptr(x_dev), _ptr(d_off), _ptr(d_len), _ptr(onset_dev), nch, _ptr(d_w), delta, step,
                                        kmax, _lib.dbl_array(thresholds), len(thresholds), _ptr(prof), _ptr(d_poff),
                                        _ptr(rec), self.stream), "ira_echo_density")
        return prof[:total], prof_off, rec[: nch * NED_DOUBLES].view(nch, NED_DOUBLES)

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
        off = np.ascontiguousarray(off, dtype=np.int64).reshape(-1)
        length = np.ascontiguousarray(length, dtype=np.int64).reshape(-1)
        weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        half, direct, direct_window, guard = int(half), int(direct), int(direct_window), int(guard)
        separation, background, tn, keep = int(separation), int(background), int(tn), int(keep)
        nch = int(off.size)
        if length.size != nch:
            raise ValueError("off and length must be (nch,)")
        if not 1 <= half <= REFL_MAX_HALF:
            raise ValueError(f"half must be 1..{REFL_MAX_HALF} samples, got {half}")
        if weights.size != 2 * half + 1 or not (np.all(np.isfinite(weights)) and np.all(weights > 0.0)):
            raise ValueError("weights must be 2 * half + 1 finite values > 0")
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
        lst = self.empty(nch * keep * REFL_FIELDS, t.float64)
        rec = self.empty(nch * REFL_DOUBLES, t.float64)
        d_off, d_len, d_eoff = self.job_tables(off, length, erow_off)
        d_w = self.to_dev(weights)
        check(self.lib.ira_reflections(_ptr(x_dev), _ptr(d_off), _ptr(d_len), _ptr(onset_dev), nch, _ptr(d_w), half, direct,
                                       direct_window, guard, separation, background, tn, float(rel), float(prom), keep,
                                       max_room, _ptr(erow), _ptr(d_eoff), _ptr(scratch), scratch_doubles, _ptr(lst),
                                       _ptr(rec), self.stream), "ira_reflections")
        return (erow[:total], erow_off, lst[: nch * keep * REFL_FIELDS].view(nch, keep, REFL_FIELDS),
                rec[: nch * REFL_DOUBLES].view(nch, REFL_DOUBLES))

    # ------------------------------------------------------------------ frequency-dependent-window response
    def fdw_response(self, x_dev, off: np.ndarray, length: np.ndarray, centre_dev, rho: np.ndarray, half: np.ndarray,
                     window: str):
        """Windowed Fourier sums around a centre sample, one window length per frequency point (ira_fdw_response, one
        call).  Channel c: length[c] samples at off[c] of x_dev, centred at centre_dev[c] (int64 device, read on the
        device; it may lie outside the channel); point j: rho[j] = f_j / fs in (0, 0.5] and the half width half[j] >= 1
        samples (terms k = -half .. half); window "hann" or "rect".  Returns (nch, J, FDW_FIELDS) float64 device: Re S0,
        Im S0, Re S1, Im S1, A = sum |v|, N = the terms inside the channel."""
        t = self.torch
        off = np.ascontiguousarray(off, dtype=np.int64).reshape(-1)
        length = np.ascontiguousarray(length, dtype=np.int64).reshape(-1)
        rho = np.ascontiguousarray(rho, dtype=np.float64).reshape(-1)
        half_in = np.asarray(half).reshape(-1)
        nch, npts = int(off.size), int(rho.size)
        if length.size != nch:
            raise ValueError("off and length must be (nch,)")
        if nch > 65535:
            raise ValueError("at most 65535 channels per launch")
        if half_in.size != npts:
            raise ValueError("rho and half must be (J,)")
        if npts > FDW_MAX_POINTS:
            raise ValueError(f"at most {FDW_MAX_POINTS} frequency points, got {npts}")
        if window not in FDW_WINDOWS:
            raise ValueError(f"window must be one of {FDW_WINDOWS}, got {window!r}")
        if npts and not (np.all(np.isfinite(rho)) and np.all(rho > 0.0) and np.all(rho <= 0.5)):
            raise ValueError("rho must be finite and in (0, 0.5]")
        if npts and not (np.all(half_in == np.rint(half_in)) and np.all(half_in >= 1) and np.all(half_in <= FDW_MAX_HALF)):
            raise ValueError(f"half must be whole numbers 1..{FDW_MAX_HALF}")
        half = np.ascontiguousarray(half_in, dtype=np.int32)
        if nch == 0 or npts == 0:                                   # nothing to launch (zero-size tables have no address)
            return self.empty(0, t.float64)[:0].view(nch, npts, FDW_FIELDS)
        scratch_doubles = fdw_scratch_doubles(nch, half)
        scratch = self.empty(scratch_doubles, t.float64)
        out = self.empty(nch * npts * FDW_FIELDS, t.float64)
        d_off, d_len, d_rho, d_half = self.job_tables(off, length, rho, half)
        c_rho = (_lib.f64 * npts)(*rho.tolist())
        c_half = (_lib.i32 * npts)(*half.tolist())
        with self.tagged(f"[{window}]"):
            check(self.lib.ira_fdw_response(_ptr(x_dev), _ptr(d_off), _ptr(d_len), _ptr(centre_dev), nch, c_rho, c_half,
                                            _ptr(d_rho), _ptr(d_half), npts, FDW_WINDOWS.index(window), _ptr(scratch),
                                            scratch_doubles, _ptr(out), self.stream), "ira_fdw_response")
        return out[: nch * npts * FDW_FIELDS].view(nch, npts, FDW_FIELDS)

    # ------------------------------------------------------------------ burst decay (constant-Q level-over-periods map)
    def burst_table(self, rho: np.ndarray, half: np.ndarray, window: str) -> BurstTable:
        """The wavelets g_j(k) = w(k) e^{-2 pi i k rho_j}, k = -half[j] .. half[j], of every point as (re, im) doubles, one
        point after the other (ira_burst_table, one call): weight and phasor exactly as ira_fdw_response forms them.  rho[j]
        in (0, 0.5], half[j] >= 1 samples, window "hann" or "rect"."""
        t = self.torch
        rho = np.ascontiguousarray(rho, dtype=np.float64).reshape(-1)
        half_in = np.asarray(half).reshape(-1)
        npts = int(rho.size)
        if half_in.size != npts:
            raise ValueError("rho and half must be (J,)")
        if npts > FDW_MAX_POINTS:
            raise ValueError(f"at most {FDW_MAX_POINTS} frequency points, got {npts}")
        if window not in FDW_WINDOWS:
            raise ValueError(f"window must be one of {FDW_WINDOWS}, got {window!r}")
        if npts and not (np.all(np.isfinite(rho)) and np.all(rho > 0.0) and np.all(rho <= 0.5)):
            raise ValueError("rho must be finite and in (0, 0.5]")
        if npts and not (np.all(half_in == np.rint(half_in)) and np.all(half_in >= 1) and np.all(half_in <= FDW_MAX_HALF)):
            raise ValueError(f"half must be whole numbers 1..{FDW_MAX_HALF}")
        half = np.ascontiguousarray(half_in, dtype=np.int32)
        offsets, doubles = burst_table_offsets(half), burst_table_doubles(half)
        if npts == 0:                                               # nothing to launch (zero-size tables have no address)
            return BurstTable(rho, half, window, offsets, 0, None, None, None)
        table = self.empty(doubles, t.float64)
        d_rho, d_half, d_off = self.job_tables(rho, half, offsets)
        c_rho = (_lib.f64 * npts)(*rho.tolist())
        c_half = (_lib.i32 * npts)(*half.tolist())
        with self.tagged(f"[{window}]"):
            check(self.lib.ira_burst_table(c_rho, c_half, _ptr(d_rho), _ptr(d_half), _ptr(d_off), npts,
                                           FDW_WINDOWS.index(window), _ptr(table), doubles, self.stream), "ira_burst_table")
        return BurstTable(rho, half, window, offsets, doubles, table, d_half, d_off)

    def burst_decay(self, x_dev, off: np.ndarray, length: np.ndarray, centre_dev, table: BurstTable, delta: np.ndarray) -> List:
        """The map S[c, j, m] = sum over k of g_j(k) * x_c[centre_c + delta[j, m] + k] (ira_burst_decay).  Channel c:
        length[c] samples at off[c] of x_dev, centred at centre_dev[c] (int64 device, read on the device); table from
        burst_table; delta (J, M) whole samples, non-decreasing along m, |delta| <= BURST_MAX_DELTA.  The batch is cut into
        calls of burst_channels_per_call(J, M) channels, so that one call writes at most BURST_MAX_OUT_BYTES.  Returns the
        list of the calls' outputs in channel order: (channels of the call, J, M, 2) float64 device, (Re S, Im S)."""
        t = self.torch
        off = np.ascontiguousarray(off, dtype=np.int64).reshape(-1)
        length = np.ascontiguousarray(length, dtype=np.int64).reshape(-1)
        nch, npts = int(off.size), int(table.half.size)
        if length.size != nch:
            raise ValueError("off and length must be (nch,)")
        delta_in = np.asarray(delta)
        if delta_in.ndim != 2 or delta_in.shape[0] != npts:
            raise ValueError("delta must be (J, M)")
        nsteps = int(delta_in.shape[1])
        if nsteps > BURST_MAX_STEPS:
            raise ValueError(f"at most {BURST_MAX_STEPS} steps, got {nsteps}")
        if delta_in.size and not (np.all(delta_in == np.rint(delta_in)) and np.all(np.abs(delta_in) <= BURST_MAX_DELTA)):
            raise ValueError(f"delta must be whole numbers of at most {BURST_MAX_DELTA} samples either way")
        if delta_in.size and np.any(np.diff(delta_in, axis=1) < 0):
            raise ValueError("delta must not decrease along the steps")
        delta = np.ascontiguousarray(delta_in, dtype=np.int32)
        if nch == 0 or npts == 0 or nsteps == 0:                    # nothing to launch
            return [self.empty(0, t.float64)[:0].view(nch, npts, nsteps, 2)]
        per_call = burst_channels_per_call(npts, nsteps)
        d_off, d_len, d_delta = self.job_tables(off, length, delta.reshape(-1))
        c_half = (_lib.i32 * npts)(*table.half.tolist())
        c_delta = (_lib.i32 * delta.size)(*delta.reshape(-1).tolist())
        outs = []
        with self.tagged(f"[{table.window}]"):
            for a in range(0, nch, per_call):
                n = min(per_call, nch - a)
                out = self.empty(n * npts * nsteps * 2, t.float64)
                check(self.lib.ira_burst_decay(_ptr(x_dev), _ptr(d_off[a:]), _ptr(d_len[a:]), _ptr(centre_dev[a:]), n, c_half,
                                               _ptr(table.half_dev), _ptr(table.offsets_dev), _ptr(table.table), table.doubles,
                                               c_delta, _ptr(d_delta), npts, nsteps, _ptr(out), self.stream),
                      "ira_burst_decay")
                outs.append(out[: n * npts * nsteps * 2].view(n, npts, nsteps, 2))
        return outs

    # ------------------------------------------------------------------ minimum phase / excess phase (real cepstrum)
    @staticmethod
    def _minphase_sizes(spec_off: np.ndarray, n_fft: np.ndarray):
        spec_off = np.ascontiguousarray(spec_off, dtype=np.int64).reshape(-1)
        n_in = np.asarray(n_fft).reshape(-1)
        if n_in.size != spec_off.size:
            raise ValueError("spec_off and n_fft must be (n,)")
        if spec_off.size > 65535:
            raise ValueError("at most 65535 channels per launch")
        n64 = n_in.astype(np.int64)
        if n_in.size and not (np.all(n_in == n64) and np.all(n64 >= MINPHASE_MIN_N) and np.all(n64 <= 1 << MINPHASE_MAX_LOG2)
                              and np.all(n64 & (n64 - 1) == 0)):
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
        centre = np.ascontiguousarray(centre, dtype=np.int64).reshape(-1)
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
        if bins_in.size and not (np.all(bins_in == np.rint(bins_in)) and np.all(bins_in >= 1)
                                 and np.all(bins_in <= (n_fft.astype(np.int64) // 2 - 1)[:, None])):
            raise ValueError("bins must be whole numbers 1 .. n_fft / 2 - 1")
        bins = np.ascontiguousarray(bins_in, dtype=np.int32)
        if n == 0 or npts == 0:                                     # nothing to launch (zero-size tables have no address)
            return self.empty(0, t.float64)[:0].view(n, npts, MINPHASE_FIELDS)
        out = self.empty(n * npts * MINPHASE_FIELDS, t.float64)
        d_so, d_nf, d_b = self.job_tables(spec_off, n_fft, bins.reshape(-1))
        check(self.lib.ira_minphase_gather(_ptr(spec_dev), _ptr(tspec_dev), _ptr(unwrapped_dev), _ptr(d_so), _ptr(d_nf),
                                           _ptr(d_b), _ptr(pmax_dev), n, npts, _ptr(out), self.stream), "ira_minphase_gather")
        return out[: n * npts * MINPHASE_FIELDS].view(n, npts, MINPHASE_FIELDS)

    def minphase_spectrum(self, g_dev, tspec_dev, spec_off: np.ndarray, n_fft: np.ndarray, pmax_dev) -> None:
        """M = e^G (cos phi_min, sin phi_min), phi_min = 2 Im T, in place of G; Im M = 0 at k = 0 and N/2
        (ira_minphase_spectrum)."""
        spec_off, n_fft = self._minphase_sizes(spec_off, n_fft)
        n = int(spec_off.size)
        if n:
            d_so, d_nf = self.job_tables(spec_off, n_fft)
            check(self.lib.ira_minphase_spectrum(_ptr(g_dev), _ptr(tspec_dev), _ptr(d_so), _ptr(d_nf), _ptr(pmax_dev), n,
                                                 int(n_fft.max()), self.stream), "ira_minphase_spectrum")

    # ------------------------------------------------------------------ dual-channel spectral sums (Welch H1 / H2)
    def cross_spectra(self, x_dev, x_off: np.ndarray, y_off: np.ndarray, n: np.ndarray, n_fft: int, hop: int,
                      use_hann: bool):
        """Auto- and cross-spectra of (reference, measurement) pairs summed over overlapping frames, and what follows from
        them (ira_xspec_accumulate, ira_xspec_finish).  Pair p: reference n[p] samples at x_off[p] of x_dev, measurement
        n[p] samples at y_off[p] (the pair's delay is in the offsets); K = 1 + (n[p] - n_fft) // hop frames, none when
        n[p] < n_fft.  The window is window(n_fft, use_hann, 64).  Returns (npairs, XSPEC_ROWS, n_fft // 2 + 1) float64
        device: Sxx, Syy, Re Sxy, Im Sxy, H1 (re, im), H2 (re, im), coherence, 20 log10 |H1|, phase."""
        t = self.torch
        x_off = np.ascontiguousarray(x_off, dtype=np.int64).reshape(-1)
        y_off = np.ascontiguousarray(y_off, dtype=np.int64).reshape(-1)
        n = np.ascontiguousarray(n, dtype=np.int64).reshape(-1)
        n_fft, hop = int(n_fft), int(hop)
        npairs = int(x_off.size)
        if y_off.size != npairs or n.size != npairs:
            raise ValueError("x_off, y_off and n must be (npairs,)")
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
            return self.empty(0, t.float64)[:0].view(0, XSPEC_ROWS, nbins)
        max_frames = int(xspec_frames(n, n_fft, hop).max())
        if max_frames >= 1 << 31:
            raise ValueError("too many frames for one launch")
        chunks = -(-max_frames // XSPEC_FRAMES)
        partial = self.empty(npairs * chunks * 4 * nbins, t.float64)
        out = self.empty(npairs * XSPEC_ROWS * nbins, t.float64)
        win, tw = self.window(n_fft, use_hann, 64), self.twiddle(n_fft, 64)
        d_xo, d_yo, d_n = self.job_tables(x_off, y_off, n)
        with self.tagged(f"[{n_fft}]"):
            check(self.lib.ira_xspec_accumulate(_ptr(x_dev), _ptr(d_xo), _ptr(d_yo), _ptr(d_n), npairs, max_frames, n_fft,
                                                hop, _ptr(win), _ptr(tw), _ptr(partial), self.stream),
                  "ira_xspec_accumulate")
            check(self.lib.ira_xspec_finish(_ptr(partial), _ptr(d_n), npairs, max_frames, n_fft, hop, _ptr(out),
                                            self.stream), "ira_xspec_finish")
        return out[: npairs * XSPEC_ROWS * nbins].view(npairs, XSPEC_ROWS, nbins)

    # ------------------------------------------------------------------ ISO 3382-1 inter-channel cross-correlation
    def xcorr_windows(self, x_dev, l_off: np.ndarray, r_off: np.ndarray, seg_len: np.ndarray, lchan_of_seg: np.ndarray,
                      rchan_of_seg: np.ndarray, onset_dev, limits: np.ndarray, max_lag: int):
        """Partitioned float64 lag sums between the two channels of stereo pairs (ira_xcorr_windows).  Segment j: left
        channel seg_len[j] samples at l_off[j] of x_dev, right channel at r_off[j]; it starts at
        o = min(onset_dev[lchan_of_seg[j]], onset_dev[rchan_of_seg[j]]), taken on the device; limits (nseg, nlim) int64
        ascending sample counts from o.  Returns (nseg, nlim + 1, 2 max_lag + 3) float64 device: per partition
        C(-max_lag .. +max_lag), El, Er."""
        t = self.torch
        l_off = np.ascontiguousarray(l_off, dtype=np.int64)
        r_off = np.ascontiguousarray(r_off, dtype=np.int64)
        seg_len = np.ascontiguousarray(seg_len, dtype=np.int64)
        nseg = int(l_off.size)
        limits = np.ascontiguousarray(limits, dtype=np.int64)
        if limits.ndim != 2 or limits.shape[0] != nseg or r_off.size != nseg or seg_len.size != nseg:
            raise ValueError("l_off, r_off, seg_len must be (nseg,) and limits (nseg, nlim)")
        nlim, max_lag = int(limits.shape[1]), int(max_lag)
        max_len = int(seg_len.max()) if nseg else 0
        scratch = self._scratch("ira_xcorr_scratch_doubles", nseg, max_len, nlim, max_lag)
        nrec = 2 * max_lag + 3
        out = self.empty(nseg * (nlim + 1) * nrec, t.float64)
        d_lo, d_ro, d_len, d_lc, d_rc, d_lim = self.job_tables(
            l_off, r_off, seg_len, np.ascontiguousarray(lchan_of_seg, np.int32),
            np.ascontiguousarray(rchan_of_seg, np.int32), limits.reshape(-1))
        with self.tagged(f"[T{max_lag}]"):
            check(self.lib.ira_xcorr_windows(_ptr(x_dev), _ptr(d_lo), _ptr(d_ro), _ptr(d_len), _ptr(d_lc), _ptr(d_rc),
                                             _ptr(onset_dev), nseg, max_len, _ptr(d_lim), nlim, max_lag, _ptr(scratch),
                                             _ptr(out), self.stream), "ira_xcorr_windows")
        return out[: nseg * (nlim + 1) * nrec].view(nseg, nlim + 1, nrec)

    # ------------------------------------------------------------------ IEC 60268-16 modulation transfer sums
    def mtf_sums(self, x_dev, seg_off: np.ndarray, seg_len: np.ndarray, w: np.ndarray):
        """Float64 modulation transfer sums of the squared signal (ira_mtf_sums).  Row j: seg_len[j] samples at seg_off[j] of
        x_dev; w (nseg, nf) float64 modulation frequencies in turns per sample (frequency / sample rate, per row), nf <= 16,
        0 <= w <= 0.5.  Returns (nseg, 2 nf + 1) float64 device: E = sum x^2, then A_i = sum x[n]^2 cos(2 pi w_i n) and
        B_i = sum x[n]^2 sin(2 pi w_i n) per frequency, n counted from the row's first sample."""
        t = self.torch
        seg_off = np.ascontiguousarray(seg_off, dtype=np.int64)
        seg_len = np.ascontiguousarray(seg_len, dtype=np.int64)
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
        out = self.empty(nseg * nrec, t.float64)
        d_off, d_len, d_w = self.job_tables(seg_off, seg_len, w.reshape(-1))
        check(self.lib.ira_mtf_sums(_ptr(x_dev), _ptr(d_off), _ptr(d_len), _ptr(d_w), nseg, max_len, nf, _ptr(scratch),
                                    _ptr(out), self.stream), "ira_mtf_sums")
        return out[: nseg * nrec].view(nseg, nrec)

    # ------------------------------------------------------------------ harmonic distortion from a deconvolved sweep
    def harmonic_peaks(self, h_dev, h_off: np.ndarray, n_search: np.ndarray):
        """The linear peak of circular responses: the first maximum of |h| over the first n_search[c] samples of channel c
        (ira_peak_index on a view of h; nothing returns to the host).  Returns (peak int64 device, |h[peak]| float32
        device), one entry per channel."""
        h_off = np.ascontiguousarray(h_off, dtype=np.int64)
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
        h_off = np.ascontiguousarray(h_off, dtype=np.int64)
        n_fft = np.ascontiguousarray(n_fft, dtype=np.int32)
        lags = np.ascontiguousarray(lags, dtype=np.int64).reshape(-1)
        window = np.ascontiguousarray(window, dtype=np.float64).reshape(-1)
        nch, k, seg, guard = int(h_off.size), int(lags.size), int(window.size), int(guard)
        if n_fft.shape != (nch,) or (nch and n_fft.min() < 1):
            raise ValueError("n_fft must hold one length >= 1 per channel")
        if not (1 <= guard < seg):
            raise ValueError("guard must be at least 1 sample and the window longer than it")
        out = self.empty(nch * k * seg, t.float32)
        if nch:
            d_off, d_n, d_lag, d_win = self.job_tables(h_off, n_fft, lags, window)
            check(self.lib.ira_harmonic_windows(_ptr(h_dev), _ptr(d_off), _ptr(d_n), _ptr(peak_dev), _ptr(d_lag),
                                                _ptr(d_win), nch, k, guard, seg, _ptr(out), self.stream),
                  "ira_harmonic_windows")
        return out[: nch * k * seg].view(nch * k, seg)

    def harmonic_band_powers(self, spec_dev, spec_off: np.ndarray, lo: np.ndarray, cnt: np.ndarray, nbins: int):
        """Mean band powers of half spectra (ira_harmonic_band_powers).  Row r: nbins complex float64 values at spec_off[r]
        (in complex values, as rfft_any returns them) of spec_dev; lo / cnt (K, J) int32, shared by every channel; row r
        belongs to harmonic r % K.  Returns (nrow // K, K, J) float64 device: the mean of re^2 + im^2 over the bins
        lo .. lo + cnt - 1, 0 where cnt = 0."""
        t = self.torch
        spec_off = np.ascontiguousarray(spec_off, dtype=np.int64)
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
        out = self.empty(nrow * j, t.float64)
        if nrow:
            d_so, d_lo, d_cnt = self.job_tables(spec_off, lo.reshape(-1), cnt.reshape(-1))
            check(self.lib.ira_harmonic_band_powers(_ptr(spec_dev), _ptr(d_so), _ptr(d_lo), _ptr(d_cnt), nrow, k, j, nbins,
                                                    _ptr(out), self.stream), "ira_harmonic_band_powers")
        return out[: nrow * j].view(nrow // k, k, j)

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
        rec = self.empty(n * LUNDEBY_DOUBLES, t.float64)
        lens = self.empty(n, t.int64)
        suffix = self.empty(rows["table_doubles"], t.float64)
        if n:
            _, d_len, d_ch, d_b, d_nb, d_m, d_boff = rows["dev"]
            check(self.lib.ira_lundeby_estimate(_ptr(d_len), _ptr(d_ch), _ptr(start_dev), _ptr(d_b), _ptr(d_nb), _ptr(d_m),
                                                _ptr(d_boff), n, _ptr(blk_dev), 1 if compensate else 0, _ptr(rec),
                                                _ptr(lens), _ptr(suffix), self.stream), "ira_lundeby_estimate")
        return rec[: n * LUNDEBY_DOUBLES].view(n, LUNDEBY_DOUBLES), lens[:n], suffix

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
        info = self.empty(2 * n, t.int32)
        rec = self.empty(n * MS_MAX_ORDER * MS_DOUBLES, t.float64)
        if n:
            _, d_len, d_ch, d_b, d_nb, _, d_boff = rows["dev"]
            check(self.lib.ira_multislope_points(_ptr(d_len), _ptr(d_ch), _ptr(start_dev), _ptr(d_b), _ptr(d_nb), _ptr(d_boff),
                                                 n, _ptr(blk_dev), float(fit_fraction), _ptr(d), _ptr(info), _ptr(rec),
                                                 self.stream), "ira_multislope_points")
        return d, info[: 2 * n].view(n, 2), rec[: n * MS_MAX_ORDER * MS_DOUBLES].view(n, MS_MAX_ORDER, MS_DOUBLES)

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

    # ------------------------------------------------------------------ a4/a5/a16
    def curve_fits(self, y_dev, off: np.ndarray, lens: np.ndarray, t_mul: float, t_div: float,
                   ranges: Sequence[Tuple[float, float]], min_points: int, cross: Sequence[float] = (),
                   rel_to_peak: bool = False, floor_db: float = -120.0, min_peak_above_floor: float = 0.0,
                   t_axis_dev=None, lens_dev=None):
        """Returns (fits (ncurves, nranges, 8) float64 device, cross (ncurves, ncross) float64 device).
        lens_dev (int64 device, (ncurves,)): the curves' lengths as a kernel left them on the device; they need not visit
        the host.  lens then only bounds them from above (it picks the workgroup size, which fixes the order of the
        regression sums)."""
        n = int(off.size)
        fit, cr, c_ranges, c_cross, views = self._fit_outputs(n, ranges, cross)
        if lens_dev is None:
            d_off, d_len = self.job_tables(off, lens)
        else:
            d_off, = self.job_tables(off)
            d_len = lens_dev
        check(self.lib.ira_curve_fits(_ptr(y_dev), _ptr(d_off), _ptr(d_len), n,
                                      int(lens.max()) if n else 0, float(t_mul), float(t_div), _ptr(t_axis_dev),
                                      c_ranges, len(ranges), int(min_points), c_cross, len(cross), 1 if rel_to_peak else 0,
                                      float(floor_db), float(min_peak_above_floor), _ptr(fit), _ptr(cr), self.stream),
              "ira_curve_fits")
        return views

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

    @staticmethod
    def stft_tail_ok(n_fft: int, precision: int) -> bool:
        """Configurations whose frame-major / log-bin STFT takes the table of tail_energy (stft6_kernel, stft5_kernel)."""
        return (int(n_fft), int(precision)) in ((4096, 32), (8192, 64))

    @staticmethod
    def _tail_args(tail, seg_off: np.ndarray, cols: np.ndarray, n_fft: int, hop: int):
        """The table's device pointers for an STFT call over the segments at seg_off, after the contract of
        ira_stft_logbin_tail has been checked on the host: same starts, no frame past the table's end."""
        if not np.array_equal(np.asarray(tail["start"]), np.asarray(seg_off, dtype=np.int64)):
            raise ValueError("the suffix-energy table was made for other segment starts")
        last = np.asarray(seg_off, dtype=np.int64) + (cols.astype(np.int64) - 1) * int(hop) + int(n_fft)
        if np.any((cols > 0) & (last > np.asarray(tail["end"]))):
            raise ValueError("a frame reads past the end the suffix-energy table was made for")
        return tail["tab"], tail["off_dev"]

    # ------------------------------------------------------------------ a11
    def stft_mag_db(self, x_dev, seg_off: np.ndarray, nframes: np.ndarray, n_fft: int, hop: int, use_hann: bool,
                    floor_db: float, precision: int = 32, frame_sel: Optional[List[np.ndarray]] = None,
                    frame_major: bool = False, tail=None):
        """
        STFT magnitude (dB) of segments starting at seg_off with nframes[s] valid frames each.
        Returns (out flat f32 device, out_off host int64); out[s] is a C-contiguous (n_fft/2+1, T_s) matrix.
        frame_sel: optional per-segment arrays of frame indices (then T_s = len(frame_sel[s])).
        frame_major=True asks for the transposed (T_s, n_fft/2+1) layout (ira_stft_mag_db_tf; see stft_frame_major_ok).
        tail: the table of tail_energy for these segments (same starts); the same bytes come back, sooner where the
        segments end in quiet tails.  Used by the frame-major calls ira_stft_mag_db_tf implements, without a frame
        selection (stft_tail_ok), ignored by every other.
        """
        t = self.torch
        n = int(seg_off.size)
        f = n_fft // 2 + 1
        if self.stft_generic_needed(n_fft):
            return self._stft_generic(x_dev, seg_off, nframes, int(n_fft), int(hop), use_hann, floor_db, frame_sel,
                                      frame_major)
        if frame_sel is not None:
            cols = np.array([int(s.size) for s in frame_sel], dtype=np.int32)
            sel_off = exclusive_cumsum(cols)
            if cols.sum():
                sel, sel_off_dev = self.job_tables(np.concatenate(frame_sel).astype(np.int32), sel_off)
            else:
                sel, sel_off_dev = self.empty(1, t.int32), self.to_dev(sel_off)
        else:
            cols = np.ascontiguousarray(nframes, dtype=np.int32)
            sel = None
            sel_off_dev = None
        sizes = cols.astype(np.int64) * f
        out_off = exclusive_cumsum(sizes)
        out = self.empty(int(sizes.sum()), t.float32)
        d_off, d_cols, d_ooff = self.job_tables(seg_off, cols, out_off)
        use_tail = tail is not None and frame_major and frame_sel is None and self.stft_tail_ok(n_fft, precision) and n > 0
        name = "ira_stft_mag_db_tf_tail" if use_tail else "ira_stft_mag_db_tf" if frame_major else "ira_stft_mag_db"
        extra = ()
        if use_tail:
            d_tab, d_toff = self._tail_args(tail, seg_off, cols, n_fft, hop)
            consts = self.empty(1, t.float64)           # IRA_STFT_CONSTS_DOUBLES(0); alive until the call is enqueued
            extra = (_ptr(d_tab), _ptr(d_toff), _ptr(consts))
        with self.tagged(f"[f{precision},n{n_fft}{',sel' if frame_sel is not None else ''}]"):
            check(getattr(self.lib, name)(
                _ptr(x_dev), _ptr(d_off), _ptr(d_cols), n, int(cols.max()) if n else 0, int(n_fft), int(hop),
                _ptr(self.window(n_fft, use_hann, precision)), _ptr(self.twiddle(n_fft, precision)), int(precision),
                float(floor_db), _ptr(out), _ptr(d_ooff), _ptr(sel), _ptr(sel_off_dev), *extra, self.stream), name)
        return out, out_off, cols

    def stft_logbin(self, x_dev, seg_off: np.ndarray, nframes: np.ndarray, n_fft: int, hop: int, use_hann: bool,
                    floor_db: float, k_base: int, first: np.ndarray, count: np.ndarray, tail=None):
        """Fused float64 STFT + log-bin aggregation (ira_stft_logbin; n_fft 8192): (curves device, curves_off host).
        tail: the table of tail_energy for these segments (same starts): the same bytes (ira_stft_logbin_tail), sooner where
        the segments end in quiet tails."""
        t = self.torch
        n = int(seg_off.size)
        nbins = int(first.size)
        cols = np.ascontiguousarray(nframes, dtype=np.int32)
        sizes = cols.astype(np.int64) * nbins
        out_off = exclusive_cumsum(sizes)
        out = self.empty(int(sizes.sum()), t.float32)
        d_off, d_cols, d_ooff, d_f, d_c = self.job_tables(seg_off, cols, out_off, first.astype(np.int32),
                                                           count.astype(np.int32))
        name, extra = "ira_stft_logbin", ()
        if tail is not None and n > 0:
            d_tab, d_toff = self._tail_args(tail, seg_off, cols, n_fft, hop)
            name = "ira_stft_logbin_tail"
            consts = self.empty(1 + (nbins + 1) // 2, t.float64)   # IRA_STFT_CONSTS_DOUBLES; alive until the call is enqueued
            extra = (_ptr(d_tab), _ptr(d_toff), _ptr(consts))
        with self.tagged(f"[f64,n{n_fft}]"):
            check(getattr(self.lib, name)(_ptr(x_dev), _ptr(d_off), _ptr(d_cols), n, int(cols.max()) if n else 0,
                                          int(n_fft), int(hop), _ptr(self.window(n_fft, use_hann, 64)),
                                          _ptr(self.twiddle(n_fft, 64)), 64, float(floor_db), int(k_base), _ptr(d_f),
                                          _ptr(d_c), nbins, _ptr(out), _ptr(d_ooff), *extra, self.stream), name)
        return out, out_off

    @staticmethod
    def stft_generic_needed(n_fft: int) -> bool:
        """Frame sizes the register / LDS STFT kernels do not take (they need a power of two in [64, 16384]): the reference
        accepts any positive n_fft (numpy.fft.rfft of arbitrary length, spectrogram.py:150), e.g. `--nfft 6000`."""
        n = int(n_fft)
        return n < 64 or n > 16384 or (n & (n - 1)) != 0

    def _stft_generic(self, x_dev, seg_off, nframes, n_fft: int, hop: int, use_hann: bool, floor_db: float, frame_sel,
                      frame_major: bool):
        """STFT of an arbitrary frame size through the arbitrary-length transforms: every frame is one element of
        ira_rfft_any / ira_rfft_smooth (float64, Hann window of length n_fft = numpy.hanning(n_fft), frames of equal length
        ride two per complex transform), then ira_spectrum_mag_phase's dB conversion (the same max(|X|, 10^(floor/20))
        -> 20 log10 -> float32 as a11).  The natural result is frame-major (T, F); the (F, T) layout of the reference is
        produced by a per-segment transposed copy (plumbing, only when a caller asks for it)."""
        t = self.torch
        n = int(seg_off.size)
        f = n_fft // 2 + 1
        if frame_sel is not None:
            frames = [np.asarray(s_, dtype=np.int64) for s_ in frame_sel]
        else:
            frames = [np.arange(int(c), dtype=np.int64) for c in nframes]
        cols = np.array([fr.size for fr in frames], dtype=np.int32)
        sizes = cols.astype(np.int64) * f
        out_off = exclusive_cumsum(sizes)
        total_frames = int(cols.sum())
        if total_frames == 0:
            return self.empty(1, t.float32), out_off, cols
        xoff = np.concatenate([int(seg_off[i]) + fr * int(hop) for i, fr in enumerate(frames)])
        lengths = np.full(total_frames, n_fft, dtype=np.int32)
        spec, spec_off = self.rfft_any(x_dev, xoff, lengths, bool(use_hann))
        mag, _ = self.spectrum_mag_phase(spec, spec_off, lengths, float(floor_db), want_phase=False)
        if frame_major:
            return mag, out_off, cols
        out = self.empty(int(sizes.sum()), t.float32)
        for i in range(n):
            c = int(cols[i])
            if c:
                o = int(out_off[i])
                out[o : o + c * f].view(f, c).copy_(mag[o : o + c * f].view(c, f).t())
        return out, out_off, cols

    @staticmethod
    def stft_logbin_ok(n_fft: int) -> bool:
        return int(n_fft) == 8192

    @staticmethod
    def stft_frame_major_ok(n_fft: int, precision: int) -> bool:
        """Configurations that deliver the frame-major (T, F) layout directly: ira_stft_mag_db_tf's, and every frame size
        that goes through the arbitrary-length path (_stft_generic)."""
        return (int(n_fft), int(precision)) in ((4096, 32), (8192, 64)) or Engine.stft_generic_needed(n_fft)

    # ------------------------------------------------------------------ a9/a17: arbitrary-length f64 DFTs
    def conv_size_for(self, need: int) -> int:
        """Smallest supported convolution size M >= need (a linear convolution of `need` distinct lags)."""
        return conv_size(need, self.three_pow2_sizes)

    def _query_pair(self, name: str, *args, refusal_is_none: bool = False):
        """(a, b) as the library entry point `name` answers them through two int32 pointers; a refusal raises, or is None."""
        a, b = ctypes.c_int32(0), ctypes.c_int32(0)
        rc = getattr(self.lib, name)(*args, ctypes.byref(a), ctypes.byref(b))
        if rc != 0 and refusal_is_none:
            return None
        check(rc, name)
        return a.value, b.value

    def _two_pass_tables(self, key: tuple, split):
        """The twiddle tables of a two-pass transform of n1 * n2 points, (n1, n2) = split(): exp(-2 pi i k / period) for
        the n1-point and the n2-point column transforms and for the step between the passes (cached under key)."""
        def make():
            n1, n2 = split()
            return tuple(self._table_to_dev(_unit_roots(count, period))
                         for count, period in ((n1, n1), (n2, n2), (n2, n1 * n2)))

        return self._cached(key, make)

    def long_tables(self, m: int):
        return self._two_pass_tables(("long", int(m)), lambda: self._query_pair("ira_fft_split", int(m)))

    def smooth_split(self, n: int):
        """(n1, n2) if the library has a direct transform for length n, else None (cached); None when smooth_ffts is off."""
        ask = lambda: self._query_pair("ira_fft_smooth_split", int(n), refusal_is_none=True) if n < (1 << 31) else None
        return self._cached(("smooth?", int(n)), ask) if self.smooth_ffts else None

    def smooth_tables(self, n: int):
        return self._two_pass_tables(("smooth", int(n)), lambda: self.smooth_split(n))

    def _filter_pool(self, m: int, need_slots: int):
        """The pool for size m on the current stream with room for need_slots filters of one call, or None."""
        t = self.torch
        slot_doubles = 2 * int(m)
        limit = int(self.filter_cache_bytes // (8 * slot_doubles))
        if limit < need_slots:
            return None
        key = (int(m), int(self.stream))
        self._filter_tick += 1
        pool = self._filter_pools.get(key)
        if pool is not None and pool["cap"] >= need_slots:
            pool["last"] = self._filter_tick
            return pool
        cap = max(2 * need_slots, 32, 2 * pool["cap"] if pool is not None else 0)
        cap = min(cap, limit)
        self._filter_pools.pop(key, None)                  # a pool that grows starts again (its filters are rebuilt on demand)
        total = lambda: sum(q["cap"] * 16 * k[0] for k, q in self._filter_pools.items())
        while self._filter_pools and total() + cap * 8 * slot_doubles > self.filter_cache_bytes:
            victim = min(self._filter_pools, key=lambda k: self._filter_pools[k]["last"])
            del self._filter_pools[victim]
        pool = dict(buf=self.empty(cap * slot_doubles, t.float64), slot_of={}, length_of=[None] * cap, tick=0,
                    used=[0] * cap, cap=cap, last=self._filter_tick)
        self._filter_pools[key] = pool
        return pool

    def forget_filters(self) -> None:
        """Forget which chirp-filter spectra the pools hold (their buffers stay): the next call of every length rebuilds
        its filter.  bench.py's `value_new_lengths` calls this before every step -- the rate of a job whose fr / filter
        segment lengths never repeat (they are data dependent: N - argmax|x|), against the pooled rate of a job that sees
        the same lengths again."""
        for pool in self._filter_pools.values():
            cap = pool["cap"]
            pool["slot_of"], pool["length_of"], pool["used"] = {}, [None] * cap, [0] * cap

    def _filters(self, lengths: np.ndarray, m: int):
        """Chirp-filter spectra for the distinct lengths in `lengths`; returns (bfilt device, bidx int32 host)."""
        t = self.torch
        uniq, inv = np.unique(lengths.astype(np.int32), return_inverse=True)
        t1, t2, tf = self.long_tables(m)
        slot_doubles = 2 * int(m)
        pool = self._filter_pool(m, int(uniq.size))
        if pool is None:                          # does not fit the budget: build a private array for this call
            bf = self.empty(int(uniq.size) * slot_doubles, t.float64)
            d_l = self.to_dev(uniq.astype(np.int32))
            check(self.lib.ira_bluestein_filter(_ptr(d_l), int(uniq.size), int(m), _ptr(t1), _ptr(t2), _ptr(tf),
                                                _ptr(bf), self.stream), "ira_bluestein_filter")
            return bf, inv.astype(np.int32)
        cap = pool["cap"]
        pool["tick"] += 1
        tick = pool["tick"]
        slots = np.empty(uniq.size, dtype=np.int32)
        missing = []
        for j, ln in enumerate(uniq.tolist()):
            s = pool["slot_of"].get(ln)
            if s is None:
                missing.append(j)
            else:
                slots[j] = s
                pool["used"][s] = tick
        if missing:
            # victims: least recently used slots not needed by this call
            order = sorted(range(cap), key=lambda s: pool["used"][s])
            victims = [s for s in order if pool["used"][s] != tick][: len(missing)]
            for j, s in zip(missing, victims):
                old_len = pool["length_of"][s]
                if old_len is not None:
                    del pool["slot_of"][old_len]
                ln = int(uniq[j])
                pool["slot_of"][ln] = s
                pool["length_of"][s] = ln
                pool["used"][s] = tick
                slots[j] = s
            # build the missing filters slot by slot runs (contiguous slots in one launch where possible)
            todo = sorted((int(slots[j]), int(uniq[j])) for j in missing)
            i = 0
            while i < len(todo):
                k = i
                while k + 1 < len(todo) and todo[k + 1][0] == todo[k][0] + 1:
                    k += 1
                run = todo[i : k + 1]
                d_l = self.to_dev(np.array([ln for _, ln in run], dtype=np.int32))
                dst = pool["buf"][run[0][0] * slot_doubles:]
                check(self.lib.ira_bluestein_filter(_ptr(d_l), len(run), int(m), _ptr(t1), _ptr(t2), _ptr(tf), _ptr(dst),
                                                    self.stream), "ira_bluestein_filter")
                i = k + 1
        return pool["buf"], slots[inv].astype(np.int32)

    _pair_bands = staticmethod(pair_bands)              # (its home is engine_plan; tests reach it here)

    def _switches(self) -> Switches:
        """The A/B attributes the planner reads, as they stand now (a Switches field is an Engine attribute of its name)."""
        return Switches(**{f.name: getattr(self, f.name) for f in fields(Switches)})

    def _launch_tables(self, tables: Dict[str, Optional[np.ndarray]], **more) -> Dict[str, object]:
        """The job tables of one planned launch (and what the engine adds to them) in ONE upload: name -> device view."""
        tables = dict(tables, **more)
        return dict(zip(tables, self.job_tables(*tables.values())))

    def rfft_any(self, x_dev, xoff: np.ndarray, lengths: np.ndarray, use_hann: bool,
                 data_len: Optional[np.ndarray] = None, win_len: Optional[np.ndarray] = None):
        """Half spectra of arbitrary-length segments: (spec, spec_off); see _rfft_any."""
        spec, spec_off, _ = self._rfft_any(x_dev, xoff, lengths, use_hann, data_len, win_len, False)
        return spec, spec_off

    def rfft_any_packed(self, x_dev, xoff: np.ndarray, lengths: np.ndarray, use_hann: bool):
        """The same for a caller whose only consumer is spectrum_mag_phase(packed=...): (spec, spec_off, packed) -- even-length
        elements that ride a half-length Bluestein transform stay PACKED (see _rfft_any); packed is None when none is."""
        return self._rfft_any(x_dev, xoff, lengths, use_hann, None, None, True)

    def _rfft_any(self, x_dev, xoff: np.ndarray, lengths: np.ndarray, use_hann: bool,
                  data_len: Optional[np.ndarray], win_len: Optional[np.ndarray], packed_ok: bool):
        """
        Half spectra (complex f64) of x[xoff[e] : xoff[e]+L[e]] (* hanning) for every element.
        data_len / win_len (optional, per element): numpy.fft.rfft(x[:d] * hanning(w)[:d], n=L) -- d samples are read
        (d < L zero-pads, d > L truncates) under the Hann window of length w (reference group_delay.py:95-109).
        NumPy defines that product for w >= d (and w = 1) only, and no caller passes another w; for 1 < w < d the window's
        cosine 0.5 + 0.5 cos(pi (2 i + 1 - w) / (w - 1)) simply continues past i = w - 1 (w = 3: 0, 1, 0, 1, ...) -- not a
        zero-extended window.  That is what the kernels do and what tests/longfft_ref.py states; w < 1 is invalid.
        Returns (spec float64 device viewed as (total_bins, 2), spec_off int64 host in complex elements, packed) -- always
        three values; the public wrappers are rfft_any (two) and rfft_any_packed (three).
        packed_ok: the caller's consumer is spectrum_mag_phase(packed=...) -- even-length elements that ride a half-length
        Bluestein transform may then stay PACKED: spec_off[e] holds the L/2 values Z = DFT(x[2m] + i x[2m+1]) instead of
        the L/2 + 1 bins, and the third return value marks them (int32 per element; None when nothing is packed).
        Which element takes which transform, and every job table, is engine_plan.plan_rfft's; this is its launch loop.
        """
        t = self.torch
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        xoff = np.ascontiguousarray(xoff, dtype=np.int64)
        if data_len is not None or win_len is not None:
            data_len = np.ascontiguousarray(lengths if data_len is None else data_len, dtype=np.int32)
            win_len = np.ascontiguousarray(lengths if win_len is None else win_len, dtype=np.int32)
        spec_off, launches, packed = plan_rfft(xoff, lengths, data_len, win_len, packed_ok, self._switches(),
                                               self.smooth_split)
        spec = self.empty(int((lengths.astype(np.int64) // 2 + 1).sum()) * 2, t.float64)
        hann = 1 if use_hann else 0
        for ln in launches:
            work = self.empty(ln.work, t.float64)
            zpair = spec if ln.packed else (self.empty(ln.zpair, t.float64) if ln.zpair else None)
            if ln.family == SMOOTH:
                t1, t2, tf = self.smooth_tables(ln.size)
                d = self._launch_tables(ln.tables)
                check(self.lib.ira_rfft_smooth(_ptr(x_dev), _ptr(d["xo"]), ln.size, ln.count, hann, _ptr(t1), _ptr(t2),
                                               _ptr(tf), _ptr(work), _ptr(spec), _ptr(d["so"]), _ptr(d["x2"]),
                                               _ptr(d["so2"]), _ptr(zpair), _ptr(d["zo"]), _ptr(d["dl"]), _ptr(d["wl"]),
                                               _ptr(d["dl2"]), _ptr(d["wl2"]), 1 if ln.half else 0, self.stream),
                      "ira_rfft_smooth")
            else:
                t1, t2, tf = self.long_tables(ln.size)
                bf, bidx = self._filters(ln.lengths, ln.size)
                d = self._launch_tables(ln.tables, bi=bidx)
                if ln.second_pads_as_first:
                    d["dl2"], d["wl2"] = d["dl"], d["wl"]
                check(self.lib.ira_rfft_any(_ptr(x_dev), _ptr(d["xo"]), _ptr(d["l"]), ln.count, hann, ln.size, _ptr(t1),
                                            _ptr(t2), _ptr(tf), _ptr(bf), _ptr(d["bi"]), _ptr(work), _ptr(spec),
                                            _ptr(d["so"]), _ptr(d["x2"]), _ptr(d["so2"]), _ptr(zpair), _ptr(d["zo"]),
                                            int(ln.lengths.max()), _ptr(d["dl"]), _ptr(d["wl"]), _ptr(d["dl2"]),
                                            _ptr(d["wl2"]), _ptr(d["il"]), 1 if ln.packed else 0, self.stream),
                      "ira_rfft_any")
        return spec, spec_off, packed

    def band_tile_layout(self, nt: int, half_out: bool):
        """(tiles, workgroups) of the partial tile energies ira_band_irfft_smooth leaves per signal (ira.h; cached)."""
        return self._cached(("tiles", int(nt), bool(half_out)), lambda: self._query_pair(
            "ira_band_tile_layout", int(nt), 1 if half_out else 0))

    def _band_tile_blocks(self, launches, nentries: int):
        """Where the smooth-length launches of a band_irfft call leave the partial tile energies of their signals: one
        block of 2 x tiles x workgroups doubles per job, launch after launch in ONE buffer.  Returns (part float64
        device | None, first double of every launch's blocks, (part_off, part_wgs, part_tiles) per entry)."""
        part_off = np.full(nentries, -1, dtype=np.int64)
        part_wgs = np.zeros(nentries, dtype=np.int32)
        part_tiles = np.zeros(nentries, dtype=np.int32)
        bases, total = [], 0
        for ln in launches:
            tiles, wgs = self.band_tile_layout(ln.size, ln.half)
            bases.append(total)
            blk = tiles * wgs
            first = total + np.arange(ln.count, dtype=np.int64) * (2 * blk)
            two = ln.partner >= 0
            for entries, at in ((ln.jobs, first), (ln.partner[two], first[two] + blk)):
                part_off[entries], part_wgs[entries], part_tiles[entries] = at, wgs, tiles
            total += ln.count * 2 * blk
        part = self.empty(total, self.torch.float64) if total else None
        return part, bases, (part_off, part_wgs, part_tiles)

    def band_irfft(self, spec_dev, spec_off: np.ndarray, lengths: np.ndarray, band_params: np.ndarray,
                   freq_val: np.ndarray, y_dev, y_off: np.ndarray, want_tiles: bool = False):
        """
        Masked inverse transforms, ONE BAND PER ENTRY: entry j filters the half spectrum at spec_off[j] (length
        lengths[j], bin step freq_val[j]) with the 8-double mask record band_params[j] and writes lengths[j]
        float32 samples at y_off[j].  Two bands of the SAME spectrum are inverse-transformed together (y1 + i*y2; see
        ira_band_irfft in include/ira.h); a band left over takes a half-length inverse when its length allows it (smooth
        family, even length) and a full-length one otherwise.  (pair_across_channels = True: round 2's pairing of entries
        with the same length and bin step from different channels.)
        want_tiles (round 5): the smooth-length inverses also leave the partial energies of every band signal's EDC tiles;
        returns (part float64 device, part_off int64 per entry (-1: none, e.g. Bluestein lengths), part_wgs and part_tiles
        int32 per entry) for edc_fits(tiles=...), else None.
        The pairing, the launches and their job tables are engine_plan.plan_band_irfft's; this is its launch loop.
        """
        t = self.torch
        self.last_band_info = []          # the job_info records of this call's launches (tests, diagnostics) ...
        self.last_band_info_half = []     # ... and whether the launch was the half-length (single band) one
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        launches = plan_band_irfft(np.ascontiguousarray(spec_off, dtype=np.int64), lengths,
                                   np.ascontiguousarray(band_params, dtype=np.float64).reshape(-1, 8),
                                   np.ascontiguousarray(freq_val, dtype=np.float64),
                                   np.ascontiguousarray(y_off, dtype=np.int64), self._switches(), self.smooth_split)
        part = tiles_out = None
        if want_tiles and self.band_tile_energies:
            part, bases, per_entry = self._band_tile_blocks([ln for ln in launches if ln.family == SMOOTH],
                                                            int(lengths.size))
            if part is not None:
                tiles_out = (part,) + per_entry
        for li, ln in enumerate(launches):                  # (the smooth launches come first: li indexes bases)
            work = self.empty(ln.work, t.float64)
            if ln.family == SMOOTH:
                t1, t2, tf = self.smooth_tables(ln.size)
                d = self._launch_tables(ln.tables)
                # round 4: narrow bands skip the first pass (ira.h, job_info_dev); sparse_bands = False is the A/B
                info = self.empty(4 * ln.count, t.int32) if self.sparse_bands else None
                check(self.lib.ira_band_irfft_smooth(_ptr(spec_dev), _ptr(d["so"]), ln.size, ln.count, _ptr(d["bp"]),
                                                     _ptr(d["fv"]), _ptr(t1), _ptr(t2), _ptr(tf), _ptr(work), _ptr(y_dev),
                                                     _ptr(d["y1"]), _ptr(d["y2"]), _ptr(d["so2"]), 1 if ln.half else 0,
                                                     _ptr(info), (_ptr(part) + 8 * bases[li]) if part is not None else None,
                                                     self.stream), "ira_band_irfft_smooth")
                self.last_band_info.append(info)
                self.last_band_info_half.append(ln.half)
            else:
                t1, t2, tf = self.long_tables(ln.size)
                bf, bidx = self._filters(ln.lengths, ln.size)
                d = self._launch_tables(ln.tables, bi=bidx)
                check(self.lib.ira_band_irfft(_ptr(spec_dev), _ptr(d["so"]), _ptr(d["l"]), ln.count, _ptr(d["bp"]),
                                              _ptr(d["fv"]), ln.size, _ptr(t1), _ptr(t2), _ptr(tf), _ptr(bf),
                                              _ptr(d["bi"]), _ptr(work), _ptr(y_dev), _ptr(d["y1"]), _ptr(d["y2"]),
                                              _ptr(d["so2"]), self.stream), "ira_band_irfft")
        return tiles_out

    def spectrum_mag_phase(self, spec_dev, spec_off: np.ndarray, lengths: np.ndarray, floor_db: float,
                           want_phase: bool, packed: Optional[np.ndarray] = None):
        """mag_db (f32) [+ wrapped phase f64] laid out at the same per-element bin offsets as the spectra.  packed (int32 per
        element, from rfft_any(packed_ok=True)): elements whose spectrum is still the packed half-length transform."""
        t = self.torch
        n = int(spec_off.size)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        total = int((lengths.astype(np.int64) // 2 + 1).sum())
        mag = self.empty(total, t.float32)
        ph = self.empty(total, t.float64) if want_phase else None
        d_so, d_l, d_pk = self.job_tables(spec_off, lengths, None if packed is None else np.ascontiguousarray(packed, np.int32))
        check(self.lib.ira_spectrum_mag_phase(_ptr(spec_dev), _ptr(d_so), _ptr(d_l), n, int(lengths.max()),
                                              float(floor_db), _ptr(mag), _ptr(d_so), _ptr(ph), _ptr(d_so), _ptr(d_pk),
                                              self.stream), "ira_spectrum_mag_phase")
        return mag, ph

    def spectrum_finish(self, spec_dev, off: np.ndarray, lengths: np.ndarray, floor_db: float = -120.0,
                        packed: Optional[np.ndarray] = None, want_mag: bool = True, want_phase: bool = False,
                        unwrap: bool = True, degrees: bool = True, as_float64: bool = False, want_wrapped: bool = False,
                        stats: Optional[tuple] = None):
        """spectrum_mag_phase, phase_unwrap and spectrum_stats as ONE launch (ira_spectrum_finish): every output sits at the
        spectra's own bin offsets.  Returns dict(mag, phase, wrapped, stats): float32 dB (want_mag), the phase as phase_unwrap
        gives it (want_phase: float32, in degrees if asked, or float64 radians with as_float64), the wrapped float64 angles
        (want_wrapped) and, with stats = (freq_val, f_min, f_max, probe_hz), the (n, 8) records of spectrum_stats; None for
        what was not asked for."""
        t = self.torch
        n = int(off.size)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        total = int((lengths.astype(np.int64) // 2 + 1).sum())
        mag = self.empty(total, t.float32) if want_mag else None
        phase = self.empty(total, t.float64 if as_float64 else t.float32) if want_phase else None
        wrapped = self.empty(total, t.float64) if want_wrapped else None
        rec = self.empty(n * 8, t.float64) if stats is not None else None
        freq_val, f_min, f_max, probe_hz = stats if stats is not None else (None, 0.0, 0.0, 0.0)
        d_o, d_l, d_pk, d_fv = self.job_tables(off, lengths,
                                               None if packed is None else np.ascontiguousarray(packed, np.int32),
                                               None if freq_val is None else np.ascontiguousarray(freq_val, np.float64))
        check(self.lib.ira_spectrum_finish(_ptr(spec_dev), _ptr(d_o), _ptr(d_l), n, float(floor_db), _ptr(d_pk), _ptr(mag),
                                           _ptr(d_o), 1 if unwrap else 0, 1 if degrees else 0,
                                           0 if as_float64 else _ptr(phase), _ptr(phase) if as_float64 else 0,
                                           _ptr(wrapped), _ptr(d_fv), float(f_min), float(f_max), float(probe_hz),
                                           _ptr(rec), self.stream), "ira_spectrum_finish")
        return dict(mag=mag, phase=phase, wrapped=wrapped, stats=None if rec is None else rec[: n * 8].view(n, 8))

    def phase_unwrap(self, phase_dev, off: np.ndarray, lengths: np.ndarray, unwrap: bool, degrees: bool,
                     as_float64: bool = False):
        """float32 (optionally degrees) unwrapped phase, or with as_float64 the float64 radians."""
        t = self.torch
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        total = int((lengths.astype(np.int64) // 2 + 1).sum())
        out = self.empty(total, t.float64 if as_float64 else t.float32)
        d_o, d_l = self.job_tables(off, lengths)
        check(self.lib.ira_phase_unwrap(_ptr(phase_dev), _ptr(d_o), _ptr(d_l), int(off.size), 1 if unwrap else 0,
                                        1 if degrees else 0, 0 if as_float64 else _ptr(out), _ptr(d_o),
                                        _ptr(out) if as_float64 else 0, self.stream), "ira_phase_unwrap")
        return out

    def log_smooth(self, mag_dev, off: np.ndarray, stride: np.ndarray, k_lo: np.ndarray, nsel: np.ndarray,
                   fstep: np.ndarray, window: int, bins_per_octave: int, through_float32: bool) -> bool:
        """Log-frequency smoothing of dB curves in place (ira_log_smooth_db).  Grid geometry exactly as the reference
        computes it on the host: log2 of the first / last selected float32 frequency, count = max(8, ceil(span * bpo)) + 1
        with bpo >= 16.  Returns False (nothing done) when a grid is too large for the kernel."""
        n = int(np.asarray(off).size)
        k_lo = np.ascontiguousarray(k_lo, dtype=np.int32)
        nsel = np.ascontiguousarray(nsel, dtype=np.int32)
        fstep = np.ascontiguousarray(fstep, dtype=np.float64)
        f_first = (k_lo.astype(np.float64) * fstep).astype(np.float32).astype(np.float64)
        f_last = ((k_lo.astype(np.float64) + nsel - 1) * fstep).astype(np.float32).astype(np.float64)
        with np.errstate(divide="ignore"):
            a, b = np.log2(f_first), np.log2(f_last)
        bpo = int(max(16, bins_per_octave))
        count = (np.maximum(8, np.ceil((b - a) * bpo)).astype(np.int64) + 1).astype(np.int32)
        if n == 0:
            return True
        if int(count.max()) > 2048 or not np.all(np.isfinite(a)):
            return False
        d = self.job_tables(np.ascontiguousarray(off, np.int64), np.ascontiguousarray(stride, np.int32), k_lo, nsel, fstep,
                             a, b, count)
        check(self.lib.ira_log_smooth_db(_ptr(mag_dev), *[_ptr(x) for x in d], n, int(count.max()), int(window),
                                         1 if through_float32 else 0, self.stream), "ira_log_smooth_db")
        return True

    def order_stats(self, values_dev, off: np.ndarray, count: np.ndarray, ranks: np.ndarray):
        """sorted(segment)[rank] for every (segment, rank): float64 device tensor (nseg, nranks); ranks is (nseg, nranks)."""
        t = self.torch
        ranks = np.ascontiguousarray(ranks, dtype=np.int64)
        nseg, nr = ranks.shape
        out = self.empty(nseg * nr, t.float64)
        d_o, d_c, d_r = self.job_tables(np.ascontiguousarray(off, np.int64), np.ascontiguousarray(count, np.int32),
                                        ranks.reshape(-1))
        check(self.lib.ira_order_stats(_ptr(values_dev), _ptr(d_o), _ptr(d_c), int(nseg), _ptr(d_r), int(nr), _ptr(out),
                                       self.stream), "ira_order_stats")
        return out[: nseg * nr].view(nseg, nr)

    def diffusion(self, x_dev, xoff: np.ndarray, nframes: np.ndarray, win: int, hop: int, max_lag: int,
                  thr_rms: float, gauss_expected: float):
        """Per-window max|autocorr| and echo density (float32 device, flat) + host offsets (see ira_diffusion)."""
        t = self.torch
        n = int(xoff.size)
        nframes = np.ascontiguousarray(nframes, dtype=np.int32)
        out_off = exclusive_cumsum(nframes)
        total = int(nframes.astype(np.int64).sum())
        ac, ed = self.empty(total, t.float32), self.empty(total, t.float32)
        d_xo, d_nf, d_oo = self.job_tables(np.ascontiguousarray(xoff, np.int64), nframes, out_off)
        check(self.lib.ira_diffusion(_ptr(x_dev), _ptr(d_xo), _ptr(d_nf), n, int(nframes.max()), int(win), int(hop),
                                     int(max_lag), float(thr_rms), float(gauss_expected), _ptr(ac), _ptr(ed),
                                     _ptr(d_oo), self.stream), "ira_diffusion")
        return ac, ed, out_off

    def diffusion_stereo(self, x_dev, loff: np.ndarray, roff: np.ndarray, nframes: np.ndarray, win: int, hop: int,
                         max_lag: int):
        """Per-window corr0 and IACC max of channel pairs (see ira_diffusion_stereo)."""
        t = self.torch
        n = int(loff.size)
        nframes = np.ascontiguousarray(nframes, dtype=np.int32)
        out_off = exclusive_cumsum(nframes)
        total = int(nframes.astype(np.int64).sum())
        c0, ia = self.empty(total, t.float32), self.empty(total, t.float32)
        d_lo, d_ro, d_nf, d_oo = self.job_tables(np.ascontiguousarray(loff, np.int64), np.ascontiguousarray(roff, np.int64),
                                                 nframes, out_off)
        check(self.lib.ira_diffusion_stereo(_ptr(x_dev), _ptr(d_lo), _ptr(d_ro), _ptr(d_nf), n, int(nframes.max()),
                                            int(win), int(hop), int(max_lag), _ptr(c0), _ptr(ia), _ptr(d_oo),
                                            self.stream), "ira_diffusion_stereo")
        return c0, ia, out_off

    def group_delay(self, phase64_dev, off: np.ndarray, n_fft: np.ndarray, bin_step: np.ndarray, sample_rate_hz: float):
        """-numpy.gradient(phase, w) on the rad/sample axis of an n_fft-point rFFT (see ira_group_delay)."""
        t = self.torch
        n = int(off.size)
        nbins = (np.ascontiguousarray(n_fft, dtype=np.int64) // 2 + 1).astype(np.int32)
        gd = self.empty(int(nbins.astype(np.int64).sum()), t.float64)
        # Which formula numpy.gradient takes (uniform spacing iff every diff of the axis is bit-identical) depends on the
        # transform length, the bin step and the sample rate alone: decided once per distinct triple on the host, with the
        # reference's own expression (group_delay.py:113-124), instead of a sweep over every bin of every channel per call.
        bin_step = np.ascontiguousarray(bin_step, np.float64)
        known = np.empty(n, dtype=np.int32)
        def nonuniform(nb, step, rate):
            d = np.diff(2.0 * np.pi * ((np.arange(nb, dtype=np.float64) * step) / rate))
            return int(d.size > 0 and not bool(np.all(d == d[0])))

        for i in range(n):
            key = (int(nbins[i]), float(bin_step[i]), float(sample_rate_hz))
            known[i] = self._cached(("gd nonuniform",) + key, lambda: nonuniform(*key))
        d_o, d_n, d_v, flags = self.job_tables(np.ascontiguousarray(off, np.int64), nbins, bin_step, known)
        check(self.lib.ira_group_delay(_ptr(phase64_dev), _ptr(d_o), _ptr(d_n), n, int(nbins.max()), _ptr(d_v),
                                       float(sample_rate_hz), _ptr(flags), 1, _ptr(gd), self.stream), "ira_group_delay")
        return gd

    def spectrum_stats(self, mag_dev, off: np.ndarray, lengths: np.ndarray, freq_val: np.ndarray, f_min: float,
                       f_max: float, probe_hz: float = 1000.0):
        t = self.torch
        n = int(off.size)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        out = self.empty(n * 8, t.float64)
        d_o, d_l, d_fv = self.job_tables(off, lengths, np.ascontiguousarray(freq_val, np.float64))
        check(self.lib.ira_spectrum_stats(_ptr(mag_dev), _ptr(d_o), _ptr(d_l), n, _ptr(d_fv), float(f_min),
                                          float(f_max), float(probe_hz), _ptr(out), self.stream), "ira_spectrum_stats")
        return out[: n * 8].view(n, 8)

    # ------------------------------------------------------------------ a14 / a15
    def waterfall_rel(self, mag_dev, mag_off: np.ndarray, nslices: np.ndarray, k_lo: int, nsel: int,
                      slice_max: bool, dyn_db: float):
        """(S_e, nsel) relative-dB slices per element; returns (out f32 device, out_off host)."""
        t = self.torch
        n = int(mag_off.size)
        nslices = np.ascontiguousarray(nslices, dtype=np.int32)
        sizes = nslices.astype(np.int64) * int(nsel)
        out_off = exclusive_cumsum(sizes)
        out = self.empty(int(sizes.sum()), t.float32)
        d_mo, d_ns, d_oo = self.job_tables(mag_off, nslices, out_off)
        check(self.lib.ira_waterfall_rel(_ptr(mag_dev), _ptr(d_mo), _ptr(d_ns), n, int(k_lo), int(nsel),
                                         1 if slice_max else 0, float(dyn_db), _ptr(out), _ptr(d_oo), self.stream),
              "ira_waterfall_rel")
        return out, out_off

    def logbin_aggregate(self, mag_dev, mag_off: np.ndarray, nframes: np.ndarray, k_base: int, first: np.ndarray,
                         count: np.ndarray, frame_major_rows: int = 0):
        """(nbins, T_e) float32 log-bin curves per element; returns (out device, out_off host).
        frame_major_rows = F when mag holds the (T, F) matrices of stft_mag_db(..., frame_major=True)."""
        t = self.torch
        n = int(mag_off.size)
        nbins = int(first.size)
        nframes = np.ascontiguousarray(nframes, dtype=np.int32)
        sizes = nframes.astype(np.int64) * nbins
        out_off = exclusive_cumsum(sizes)
        out = self.empty(int(sizes.sum()), t.float32)
        d_mo, d_nf, d_oo, d_f, d_c = self.job_tables(mag_off, nframes, out_off, first.astype(np.int32),
                                                     count.astype(np.int32))
        check(self.lib.ira_logbin_aggregate(_ptr(mag_dev), _ptr(d_mo), _ptr(d_nf), n, int(nframes.max()), int(k_base),
                                            _ptr(d_f), _ptr(d_c), nbins, _ptr(out), _ptr(d_oo), int(frame_major_rows),
                                            self.stream), "ira_logbin_aggregate")
        return out, out_off

    # ------------------------------------------------------------------ a19-a21: AR pole fit
    def ar_fit(self, x_dev, xoff: np.ndarray, lengths: np.ndarray, divisor: Optional[np.ndarray], order: int,
               ridge: float = 0.0, x_is_f64: bool = False):
        """AR coefficients (nb, order+1) float64 device + info (nb, 4: status, pivots, cond estimate) for segments of x_dev."""
        t = self.torch
        n = int(xoff.size)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        max_len = int(lengths.max())
        per = int(self.lib.ira_ar_partial_doubles(int(order), max_len))
        if per <= 0:
            raise ValueError("AR order must satisfy 1 <= order <= 1024 < segment length")
        part = self.empty(n * per, t.float64)
        gs = self.empty(n * order * order, t.float64) if order > 128 else None
        coeffs = self.empty(n * (order + 1), t.float64)
        info = self.empty(n * 4, t.float64)
        d_xo, d_l, d_div = self.job_tables(np.ascontiguousarray(xoff, np.int64), lengths,
                                            np.ascontiguousarray(divisor, np.float64) if divisor is not None else None)
        flags = (1 if self.ar_dense_gram else 0) | (2 if self.ar_workgroup_solve else 0)   # IRA_AR_DENSE_GRAM | IRA_AR_WORKGROUP_SOLVE
        x32, x64 = (0, _ptr(x_dev)) if x_is_f64 else (_ptr(x_dev), 0)      # the samples are float32 or float64
        check(self.lib.ira_ar_gram(x32, x64, _ptr(d_xo),
                                   _ptr(d_l), _ptr(d_div), n, max_len, int(order), _ptr(part), flags, self.stream),
              "ira_ar_gram")
        check(self.lib.ira_ar_solve(_ptr(part), _ptr(d_l), n, max_len, int(order), float(ridge), _ptr(gs),
                                    _ptr(coeffs), _ptr(info), flags, self.stream), "ira_ar_solve")
        if self.ar_exact_cond > 0.0 and not self.ar_dense_gram:
            # conditional on the device: only elements whose float64 Cholesky broke down or whose condition estimate says
            # cond(G) eps is no longer small are solved again, in double-double arithmetic (ira_ar_exact)
            ddp = self.empty(n * int(self.lib.ira_ar_exact_doubles(int(order), max_len, 0)), t.float64)
            dds = self.empty(n * int(self.lib.ira_ar_exact_doubles(int(order), max_len, 1)), t.float64)
            check(self.lib.ira_ar_exact(x32, x64, _ptr(d_xo),
                                        _ptr(d_l), _ptr(d_div), n, max_len, int(order), float(ridge), _ptr(part), _ptr(ddp),
                                        _ptr(dds), _ptr(coeffs), _ptr(info), float(self.ar_exact_cond), self.stream),
                  "ira_ar_exact")
        if ridge == 0.0 and order <= 512 and self.ar_minnorm_cut > 0.0 and not self.ar_dense_gram:
            # conditional on the device: only elements whose Cholesky failed (rank-deficient Gram matrix) do any work
            scratch2 = self.empty(n * 2 * order * order, t.float64)
            check(self.lib.ira_ar_minnorm(_ptr(part), _ptr(d_l), n, max_len, int(order), _ptr(scratch2), _ptr(coeffs),
                                          _ptr(info), float(self.ar_minnorm_cut), self.stream), "ira_ar_minnorm")
        if ridge == 0.0 and self.ar_refine_steps > 0:
            # conditional on the device: only elements whose pivots show cond(G) > threshold do any work
            nchunks = -(-(max_len - int(order)) // 4096)
            grad = self.empty(n * nchunks * (order + 1), t.float64)
            check(self.lib.ira_ar_refine(x32, x64, _ptr(d_xo),
                                         _ptr(d_l), _ptr(d_div), n, max_len, int(order), _ptr(part), _ptr(gs),
                                         _ptr(coeffs), _ptr(info), _ptr(grad), float(self.ar_refine_cond),
                                         int(self.ar_refine_steps), flags, self.stream), "ira_ar_refine")
        return coeffs[: n * (order + 1)].view(n, order + 1), info[: n * 4].view(n, 4)

    def poly_roots(self, coeffs_dev, npoly: int, ncoef: int, trail_eps: float = 1e-14):
        """Roots (npoly, ncoef-1, 2) float64 device + counts int32 device."""
        t = self.torch
        roots = self.empty(npoly * (ncoef - 1) * 2, t.float64)
        cnt = self.empty(npoly, t.int32)
        check(self.lib.ira_poly_roots(_ptr(coeffs_dev), int(npoly), int(ncoef), float(trail_eps), _ptr(roots),
                                      _ptr(cnt), self.stream), "ira_poly_roots")
        return roots[: npoly * (ncoef - 1) * 2].view(npoly, ncoef - 1, 2), cnt[:npoly]

    def fir_numerator(self, coeffs_dev, order: int, x_dev, xoff: np.ndarray, lengths: np.ndarray,
                      divisor: Optional[np.ndarray], zero_order: int):
        t = self.torch
        n = int(xoff.size)
        b = self.empty(n * (zero_order + 1), t.float64)
        d_xo, d_l, d_div = self.job_tables(np.ascontiguousarray(xoff, np.int64), np.ascontiguousarray(lengths, np.int32),
                                            np.ascontiguousarray(divisor, np.float64) if divisor is not None else None)
        check(self.lib.ira_fir_numerator(_ptr(coeffs_dev), int(order), _ptr(x_dev), _ptr(d_xo), _ptr(d_l), _ptr(d_div),
                                         n, int(zero_order), _ptr(b), self.stream), "ira_fir_numerator")
        return b[: n * (zero_order + 1)].view(n, zero_order + 1)

    # ------------------------------------------------------------------ section 8f rank 4: deconvolution
    def deconv_divide(self, yspec_dev, yspec_off: np.ndarray, xspec_dev, xspec_off: np.ndarray, n_fft: np.ndarray,
                      regularization_relative: float) -> None:
        """Y <- Y conj(X) / (|X|^2 + eps) in place (see ira_deconv_divide)."""
        t = self.torch
        n = int(yspec_off.size)
        n_fft = np.ascontiguousarray(n_fft, dtype=np.int32)
        pmax = self.empty(n, t.float64)
        # device copies stay referenced until the launch is enqueued (a temporary would hand its block back to the
        # allocator, and the next to_dev would overwrite it before the kernel reads it)
        d_yo, d_xo, d_nf = self.job_tables(np.ascontiguousarray(yspec_off, np.int64),
                                           np.ascontiguousarray(xspec_off, np.int64), n_fft)
        check(self.lib.ira_deconv_divide(_ptr(yspec_dev), _ptr(d_yo), _ptr(xspec_dev), _ptr(d_xo), _ptr(d_nf), n,
                                         int(n_fft.max()), float(regularization_relative), _ptr(pmax), self.stream),
              "ira_deconv_divide")

    def deconv_finish(self, h_dev, h_off: np.ndarray, n_out: np.ndarray, group: np.ndarray, remove_dc: bool,
                      normalise_peak: bool, target_peak: float) -> None:
        """DC removal per channel and one peak normalisation per file, in place (see ira_deconv_finish)."""
        t = self.torch
        n = int(h_off.size)
        n_out = np.ascontiguousarray(n_out, dtype=np.int32)
        group = np.ascontiguousarray(group, dtype=np.int32)
        ngroups = int(group.max()) + 1 if n else 0
        mean, peak = self.empty(n, t.float32), self.empty(ngroups, t.int32)
        d_ho, d_no, d_gr = self.job_tables(np.ascontiguousarray(h_off, np.int64), n_out, group)
        check(self.lib.ira_deconv_finish(_ptr(h_dev), _ptr(d_ho), _ptr(d_no), _ptr(d_gr), n, ngroups,
                                         int(n_out.max()) if n else 0, 1 if remove_dc else 0, 1 if normalise_peak else 0,
                                         float(target_peak), _ptr(mean), _ptr(peak), self.stream), "ira_deconv_finish")

    def segment_peaks(self, x_dev, off: np.ndarray, lens: np.ndarray, with_index: bool = False):
        """max|x| (float32 values as float64) of arbitrary segments; with_index: (values, argmax|x| int64, the first
        maximum of a segment)."""
        n = int(off.size)
        d_o, d_l = self.job_tables(np.ascontiguousarray(off, np.int64), np.ascontiguousarray(lens, np.int64))
        pk, pa = self._peak_pick(x_dev, d_o, d_l, n, int(np.max(lens)) if n else 0)
        values = pa.cpu().numpy()[:n].astype(np.float64)
        return (values, pk.cpu().numpy()[:n].astype(np.int64)) if with_index else values
