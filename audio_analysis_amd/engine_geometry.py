"""
Geometry of the measure kernels, restated for the host in pure NumPy (neither torch nor the library is imported): the
constants that mirror IRA_* defines of include/ira.h, the sizes and layouts the kernels derive from their arguments, and
the table checks that several launchers of engine_measure.py share.  engine.py re-exports every name.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

from .engine_plan import exclusive_cumsum

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
MLS_MIN_ORDER, MLS_MAX_ORDER = 2, 21  # IRA_MLS_MIN_ORDER, IRA_MLS_MAX_ORDER
EQ_TILE_LOG2 = 11             # IRA_EQ_TILE_LOG2: levels of the pyramid a pass of ira_eq_pyramid builds from one LDS tile
EQ_TILE = 1 << EQ_TILE_LOG2   # IRA_EQ_TILE
EQ_MAX_MEMBERS = 256          # IRA_EQ_MAX_MEMBERS: channels one averaged row holds
EQ_MAX_SMOOTHING = 48         # the narrowest smoothing, 1/48 octave
EQ_SCRATCH_BYTES = 4 << 30    # equalise_cut: the device scratch of one sub-batch of rows stays under this
EDR_FRAMES = 16               # IRA_EDR_FRAMES: frames per chunk of ira_edr_power and per store run of a row (include/ira_edr.h)
EDR_BLOCK = 64                # IRA_EDR_BLOCK: frames per block of the backward sum, counted from the end
EDR_MAX_ROWS = 256            # IRA_EDR_MAX_ROWS
EDR_SERIAL = 16               # IRA_EDR_SERIAL: rows of up to this many bins are summed in ascending order by one thread
EDR_DOUBLES = 4               # IRA_EDR_DOUBLES: S(0), N, max P, the first frame of that maximum
EDR_MIN_FFT, EDR_MAX_FFT = 256, 8192
MLS_MAX_PERIODS = 1024        # IRA_MLS_MAX_PERIODS
MLS_TILE_LOG2 = 12            # IRA_MLS_TILE_LOG2: the tile order T of ira_mls_hadamard
MLS_FOLD_THREADS = 256        # IRA_MLS_FOLD_THREADS
MLS_FOLD_BLOCKS = 128         # IRA_MLS_FOLD_BLOCKS: the most workgroups of ira_mls_fold along a channel
MLS_SCRATCH_BYTES = 4 << 30   # mls.mls_device: the workspace of one chain of calls stays under this (256 channels at order 21)
# feedback taps per order: a[n] = XOR over t of a[n - t]; each set gives the full period 2^m - 1 (tests walk them)
MLS_TAPS = {2: (2, 1), 3: (3, 2), 4: (4, 3), 5: (5, 3), 6: (6, 5), 7: (7, 6), 8: (8, 6, 5, 4), 9: (9, 5), 10: (10, 7),
            11: (11, 9), 12: (12, 6, 4, 1), 13: (13, 4, 3, 1), 14: (14, 5, 3, 1), 15: (15, 14), 16: (16, 15, 13, 4),
            17: (17, 14), 18: (18, 11), 19: (19, 6, 2, 1), 20: (20, 17), 21: (21, 19)}


def flat(a, dtype) -> Optional[np.ndarray]:
    """A table as the kernels read it: contiguous, of this dtype, one dimension; None (a table a call does without) stays."""
    return None if a is None else np.ascontiguousarray(a, dtype=dtype).reshape(-1)


def same_rows(message: str, *tables) -> int:
    """The rows of tables that hold one entry per row; ValueError(message) when they differ in size."""
    n = int(np.size(tables[0]))
    if any(np.size(v) != n for v in tables[1:]):
        raise ValueError(message)
    return n


def whole_numbers(a, lo, hi) -> bool:
    """Every entry is a whole number in lo .. hi (a bound may be an array that broadcasts); true of no entries."""
    a = np.asarray(a)
    return not a.size or bool(np.all(a == np.rint(a)) and np.all(a >= lo) and np.all(a <= hi))


def segment_tables(base_off, base_len, chan_of_seg) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The triple that places a segment in a sample buffer, in the kernels' types: int64, int64 and (the channel) int32."""
    return flat(base_off, np.int64), flat(base_len, np.int64), flat(chan_of_seg, np.int32)


def point_grid(rho: np.ndarray, half, window: str) -> np.ndarray:
    """The check of a grid of frequency points (rho float64 (J,), as flat gives it): ValueError unless half has J entries,
    J <= FDW_MAX_POINTS, window is one of FDW_WINDOWS, every rho is finite and in (0, 0.5] and every half a whole number
    1 .. FDW_MAX_HALF.  Returns half as int32 (J,)."""
    half = np.asarray(half).reshape(-1)
    npts = same_rows("rho and half must be (J,)", rho, half)
    if npts > FDW_MAX_POINTS:
        raise ValueError(f"at most {FDW_MAX_POINTS} frequency points, got {npts}")
    if window not in FDW_WINDOWS:
        raise ValueError(f"window must be one of {FDW_WINDOWS}, got {window!r}")
    if npts and not (np.all(np.isfinite(rho)) and np.all(rho > 0.0) and np.all(rho <= 0.5)):
        raise ValueError("rho must be finite and in (0, 0.5]")
    if not whole_numbers(half, 1, FDW_MAX_HALF):
        raise ValueError(f"half must be whole numbers 1..{FDW_MAX_HALF}")
    return flat(half, np.int32)


def window_weights(weights, half: int, name: str) -> np.ndarray:
    """The 2 * half + 1 weights of a window as float64 (W,), all finite and > 0 (`name`: the caller's word for half)."""
    weights = flat(weights, np.float64)
    if weights.size != 2 * half + 1 or not (np.all(np.isfinite(weights)) and np.all(weights > 0.0)):
        raise ValueError(f"weights must be 2 * {name} + 1 finite values > 0")
    return weights


def xspec_frames(n, n_fft: int, hop: int) -> np.ndarray:
    """K = 1 + (n - n_fft) // hop frames of n samples, 0 when n < n_fft (int64, elementwise)."""
    n = np.asarray(n, dtype=np.int64)
    return np.where(n >= n_fft, 1 + (n - n_fft) // hop, 0).astype(np.int64)


def edr_layout(frames, nrows: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The two layouts of the energy decay relief for segments of `frames` frames and nrows rows -> (Tpad, p_off, c_off,
    total doubles of P).  P(m, j) of segment s lies at p_off[s] + j * Tpad[s] + m with Tpad = ceil(T / EDR_FRAMES) *
    EDR_FRAMES (every p_off a multiple of EDR_FRAMES: a store run of a row is 128 bytes and 128-byte aligned in a buffer
    that is); the float32 curve L(m, j) at c_off[s] + j * T[s] + m, unpadded.  All int64."""
    frames = np.asarray(frames, dtype=np.int64).reshape(-1)
    tpad = -(-frames // EDR_FRAMES) * EDR_FRAMES
    return tpad, exclusive_cumsum(tpad * int(nrows)), exclusive_cumsum(frames * int(nrows)), int(tpad.sum()) * int(nrows)


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
    half = flat(half, np.int64)
    return exclusive_cumsum(2 * half + 1).astype(np.int64)


def burst_table_doubles(half) -> int:
    """Doubles of the wavelet table (ira_burst_table_doubles restated; both calls check it): (re, im) per entry, 2 H + 1
    entries per point."""
    half = flat(half, np.int64)
    return 2 * int(np.sum(2 * half + 1))


def burst_channels_per_call(npts: int, nsteps: int, max_out_bytes: int = BURST_MAX_OUT_BYTES) -> int:
    """Channels one ira_burst_decay call of Engine.burst_decay takes: as many as keep its output of 16 bytes per (channel,
    point, step) within BURST_MAX_OUT_BYTES, at least one, at most the 65535 of a launch."""
    return int(max(1, min(65535, max_out_bytes // max(1, 16 * int(npts) * int(nsteps)))))


def minphase_scratch_bytes(n_fft) -> np.ndarray:
    """Device scratch of the minimum-phase chain per channel of transform size N, in bytes: X, G and T (16 (N/2 + 1) each),
    the cepstrum (4 N), the wrapped and the unwrapped excess phase (8 (N/2 + 1) each) and a transform's work array (8 N):
    44 N + 64, 92 MB at N = 2^21."""
    return 44 * np.asarray(n_fft, dtype=np.int64) + 64


def minphase_cut(n_fft, scratch_bytes: int = MINPHASE_SCRATCH_BYTES) -> List[Tuple[int, int]]:
    """[(first, end), ..]: consecutive channels cut into sub-batches whose scratch (minphase_scratch_bytes) stays under
    MINPHASE_SCRATCH_BYTES; a channel that alone exceeds it is a sub-batch of its own."""
    return cut_under(minphase_scratch_bytes(n_fft).reshape(-1), scratch_bytes)


def cut_under(need: np.ndarray, budget: int) -> List[Tuple[int, int]]:
    """[(first, end), ..]: consecutive entries of need (bytes each) cut into runs whose sum stays under budget; an entry
    that alone exceeds it is a run of its own."""
    cuts, first, total = [], 0, 0
    for i, b in enumerate(need.tolist()):
        if i > first and total + b > budget:
            cuts.append((first, i))
            first, total = i, 0
        total += b
    if need.size:
        cuts.append((first, int(need.size)))
    return cuts


def equalise_layout(n_fft: int) -> Tuple[np.ndarray, np.ndarray]:
    """(offsets, lengths) of the levels of a row's pyramid, int64 each (eq_level of ira_equalise.hip): n_0 = N/2 + 1,
    n_(j+1) = (n_j + 1) >> 1 until n_j = 1, level j at n_0 + .. + n_(j-1) doubles from the row's start.  log2(N) + 1 levels,
    N + log2(N) doubles a row."""
    lens = [int(n_fft) // 2 + 1]
    while lens[-1] > 1:
        lens.append((lens[-1] + 1) >> 1)
    lens = np.asarray(lens, dtype=np.int64)
    return exclusive_cumsum(lens), lens


def equalise_row_doubles(n_fft: int) -> int:
    off, lens = equalise_layout(n_fft)
    return int(off[-1] + lens[-1])


def equalise_windows(n_fft: int, smoothing: int) -> Tuple[np.ndarray, np.ndarray]:
    """(lo, hi) int32 (N/2 + 1,) of 1/b-octave smoothing, b = smoothing: lo_k = ceil(k 2^(-1/(2b))), hi_k = min(floor(k
    2^(1/(2b))), N/2), float64 NumPy; b = 0: lo = hi = k."""
    b, half = int(smoothing), int(n_fft) // 2
    if not 0 <= b <= EQ_MAX_SMOOTHING:
        raise ValueError(f"smoothing must be a whole number 0 .. {EQ_MAX_SMOOTHING} (1/b octave, 0 = none), got {smoothing}")
    k = np.arange(half + 1, dtype=np.float64)
    if b == 0:
        return k.astype(np.int32), k.astype(np.int32)
    lo = np.ceil(k * 2.0 ** (-1.0 / (2.0 * b)))
    hi = np.minimum(np.floor(k * 2.0 ** (1.0 / (2.0 * b))), float(half))
    return lo.astype(np.int32), hi.astype(np.int32)


def equalise_tables(n_fft: int, sample_rate_hz: float, f_low: float, f_high: float, transition_octaves: float, reg_in_db: float,
                    reg_out_db: float, tilt_db_per_octave: float) -> Tuple[np.ndarray, np.ndarray]:
    """(t, beta) float64 (N/2 + 1,): the target t_k = 10^(tilt log2(f_k / 1000) / 20), t_0 = t_1, and the regularisation
    beta_k = 10^(beta_dB / 10), beta_dB = reg_in + w (reg_out - reg_in), w = 0.5 (1 - cos pi u), u = clamp(log2(f_low /
    f_k) / transition, 0, 1) below the band and clamp(log2(f_k / f_high) / transition, 0, 1) above it; w = 1 at k = 0."""
    half = int(n_fft) // 2
    f = np.arange(half + 1, dtype=np.float64) * float(sample_rate_hz) / float(n_fft)
    f[0] = f[1]
    t = 10.0 ** (float(tilt_db_per_octave) * np.log2(f / 1000.0) / 20.0)
    below = np.clip(np.log2(float(f_low) / f) / float(transition_octaves), 0.0, 1.0)
    above = np.clip(np.log2(f / float(f_high)) / float(transition_octaves), 0.0, 1.0)
    u = np.where(f < float(f_low), below, above)
    w = 0.5 * (1.0 - np.cos(np.pi * u))
    w[0] = 1.0
    beta = 10.0 ** ((float(reg_in_db) + w * (float(reg_out_db) - float(reg_in_db))) / 10.0)
    return t, beta


def equalise_taper(taps: int, fade: float) -> np.ndarray:
    """v float64 (taps,): 1 up to n0 = taps - rint(fade taps), from n0 on 0.5 (1 + cos(pi (n - n0 + 1) / (taps - n0 + 1)))."""
    taps = int(taps)
    n0 = taps - int(np.rint(float(fade) * taps))
    v = np.ones(taps, dtype=np.float64)
    n = np.arange(n0, taps, dtype=np.float64)
    v[n0:] = 0.5 * (1.0 + np.cos(np.pi * (n - n0 + 1.0) / float(taps - n0 + 1)))
    return v


def equalise_scratch_bytes(n_fft: int, members) -> np.ndarray:
    """Device scratch of the equalisation chain per row of `members` channels at transform size N, in bytes: the members'
    spectra (8 N each), the pyramid (8 N), S (4 N), c and G (8 N each), the cepstrum (4 N), T (8 N), g (4 N), F (8 N) and a
    transform's work array (8 N): (8 members + 60) N + 1024."""
    return (8 * np.asarray(members, dtype=np.int64) + 60) * int(n_fft) + 1024


def equalise_cut(n_fft: int, members, scratch_bytes: int = EQ_SCRATCH_BYTES) -> List[Tuple[int, int]]:
    """[(first, end), ..]: consecutive whole rows cut into sub-batches whose scratch (equalise_scratch_bytes) stays under
    EQ_SCRATCH_BYTES; a row that alone exceeds it is a sub-batch of its own."""
    return cut_under(equalise_scratch_bytes(n_fft, members).reshape(-1), scratch_bytes)


def mls_taps(order: int, taps=None) -> Tuple[int, ...]:
    """The feedback taps of an order as a descending tuple: MLS_TAPS[order], or the caller's -- distinct whole numbers
    1 .. order with order among them.  ValueError for an order outside MLS_MIN_ORDER .. MLS_MAX_ORDER."""
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not MLS_MIN_ORDER <= order <= MLS_MAX_ORDER:
        raise ValueError(f"order must be a whole number {MLS_MIN_ORDER}..{MLS_MAX_ORDER}, got {order!r}")
    if taps is None:
        return MLS_TAPS[int(order)]
    try:
        tp = tuple(sorted({int(t) for t in taps if int(t) == t}, reverse=True))
        ok = len(tp) == len(tuple(taps))
    except (TypeError, ValueError):
        ok, tp = False, ()
    if not ok or len(tp) < 2 or tp[0] != order or tp[-1] < 1:
        raise ValueError(f"taps must be distinct whole numbers 1..{order} with {order} among them, got {taps!r}")
    return tp


def _mls_recurrence(seed: np.ndarray, count: int, order: int, taps: Tuple[int, ...]) -> np.ndarray:
    """v[n] = XOR over t of v[n - t] from the first `order` values on, `count` values in all.  Over GF(2) the feedback
    polynomial satisfies p(x)^(2^j) = p(x^(2^j)), so v[n] = XOR over t of v[n - t 2^j] as well once n >= order 2^j: with the
    largest such j a run of min(taps) 2^j values follows from the known ones in one vector operation."""
    v = np.empty(max(count, order), dtype=seed.dtype)
    v[:order] = seed
    known = order
    while known < count:
        step = 1 << ((known // order).bit_length() - 1)
        run = min(taps[-1] * step, count - known)
        acc = v[known - taps[0] * step : known - taps[0] * step + run].copy()
        for t in taps[1:]:
            acc ^= v[known - t * step : known - t * step + run]
        v[known : known + run] = acc
        known += run
    return v[:count]


def mls_bits(order: int, taps=None) -> np.ndarray:
    """One period of the sequence's bits, uint8 (2^order - 1,): a[n] = XOR over the taps t of a[n - t], a[0 .. order - 1] = 1.
    The period is full when the taps are those of a primitive polynomial (mls_tables checks it)."""
    tp = mls_taps(order, taps)
    return _mls_recurrence(np.ones(order, dtype=np.uint8), (1 << order) - 1, order, tp)


_MLS_TABLES: Dict[Tuple, Tuple[np.ndarray, np.ndarray]] = {}


def mls_tables(order: int, taps=None) -> Tuple[np.ndarray, np.ndarray]:
    """(G, out), int32 (P,) each, read-only, made once per (order, taps) -- the tables of ira_mls_fold and ira_mls_finish:
      G[j]   = 1 << j for j < order, the XOR over t of G[j - t] after (the sequence's bits a[n + j] as a combination of the
               state bits a[n .. n + order - 1])
      S[i]   = sum over q < order of a[i + q] << q                        (the state at time i)
      out[k] = S[(P - k) mod P]
    With w[G[j]] = Y[j] the transform W = FWHT(w) holds c[k] = sum over n of s[n] Y[(n + k) mod P] at W[out[k]].
    ValueError unless S is a permutation of 1 .. P, i.e. the taps give the full period."""
    tp = mls_taps(order, taps)
    key = (int(order), tp)
    if key not in _MLS_TABLES:
        m, p = int(order), (1 << int(order)) - 1
        a = _mls_recurrence(np.ones(m, dtype=np.uint8), p + m, m, tp)
        state = np.zeros(p, dtype=np.int32)
        for q in range(m):
            state |= a[q : q + p].astype(np.int32) << q
        if not np.array_equal(np.bincount(state, minlength=p + 1)[1:], np.ones(p, dtype=np.int64)):
            raise ValueError(f"taps {tp} do not give the full period {p} at order {m}")
        g = _mls_recurrence(np.int32(1) << np.arange(m, dtype=np.int32), p, m, tp)
        out = state[(p - np.arange(p)) % p]
        g.setflags(write=False)
        out.setflags(write=False)
        _MLS_TABLES[key] = (g, out)
    return _MLS_TABLES[key]


def mls_fold_blocks(order: int) -> int:
    """Workgroups of ira_mls_fold along a channel: ceil(P / MLS_FOLD_THREADS), at most MLS_FOLD_BLOCKS."""
    return min(-(-((1 << int(order)) - 1) // MLS_FOLD_THREADS), MLS_FOLD_BLOCKS)


def mls_scratch_bytes(nb: int, order: int) -> int:
    """Device bytes of one chain of the three MLS calls on nb channels (the formula of include/ira.h): the workspace of
    2^order doubles a channel and the fold's partial sums, a pair of doubles per channel and workgroup."""
    return 8 * int(nb) * ((1 << int(order)) + 2 * mls_fold_blocks(order))


def mls_sum_chain(order: int, periods: int) -> int:
    """The longest chain of additions behind E or D of ira_mls_fold: a thread's own terms (ceil(P / (B MLS_FOLD_THREADS))
    samples, R residual squares each), 6 levels of the wave's tree, 3 additions over the 4 waves, B over the workgroups."""
    b = mls_fold_blocks(order)
    per_thread = -(-((1 << int(order)) - 1) // (b * MLS_FOLD_THREADS))
    return per_thread * max(1, int(periods)) + 6 + 3 + b


def mls_pass_plan(order: int) -> List[Tuple[int, int]]:
    """The passes of ira_mls_hadamard as (first bit, bits): the low min(order, MLS_TILE_LOG2) bits in LDS tiles, then the
    bits above in passes of up to 8 (a tile of 2^a points x 2^(12 - a) columns keeps runs of 16 doubles); 9 bits go 5 + 4."""
    plan = [(0, min(int(order), MLS_TILE_LOG2))]
    lo, rem = MLS_TILE_LOG2, int(order) - MLS_TILE_LOG2
    while rem > 0:
        a = rem if rem <= 8 else (rem + 1) // 2
        plan.append((lo, a))
        lo, rem = lo + a, rem - a
    return plan


def lundeby_layout(base_off, base_len, chan_of_seg, blk_size, nblk, first_m) -> Dict[str, object]:
    """Host side of the Lundeby row tables (pure NumPy): the tables in the kernels' types, every row's table offset
    blk_off = j * (max nb + 1), table_doubles = nseg * (max nb + 1) (what ira_lundeby_scratch_doubles answers) and
    max_chunks = max over the rows of ceil((nb + 1) / (4096 // B)), the grid width of the two sample passes.
    ValueError for tables the kernels would refuse."""
    base_off, base_len, chan_of_seg = segment_tables(base_off, base_len, chan_of_seg)
    tabs = dict(base_off=base_off, base_len=base_len, chan_of_seg=chan_of_seg, blk_size=flat(blk_size, np.int32),
                nblk=flat(nblk, np.int32), first_m=flat(first_m, np.int32))
    n = same_rows("base_off, base_len, chan_of_seg, blk_size, nblk and first_m must have one entry per row", *tabs.values())
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
