"""
Planning of the arbitrary-length transforms (Engine.rfft_any / Engine.band_irfft): which transform family every
element takes, which elements share a transform, the convolution sizes, the cut into launches that fit the workspace
budget, and the host job tables of every launch.  NumPy only: no tensor, stream or library handle -- the engine walks
the launches in order, allocates, uploads each launch's tables and calls the library (engine.py).

`sw` is a Switches record (the engine's A/B attributes at the time of the call); `smooth_split(n)` answers (n1, n2) when
the library has a direct transform of length n and None otherwise (Engine.smooth_split).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

SMOOTH, BLUESTEIN = "smooth", "bluestein"


@dataclass
class Switches:
    pair_real_ffts: bool
    pair_across_channels: bool
    half_real_ffts: bool
    fuse_half_split: bool
    sparse_bands: bool
    three_pow2_sizes: bool
    workspace_budget_bytes: int


@dataclass
class Launch:
    """One library call.  `tables` holds the host job tables under the names of the call's arguments (None = the argument
    is NULL); sizes are in float64 elements."""
    family: str                            # SMOOTH: direct two-pass transform; BLUESTEIN: chirp convolution
    size: int                              # transform length (SMOOTH) / convolution size M (BLUESTEIN)
    jobs: np.ndarray                       # entry of every job (its first signal), in table order
    partner: np.ndarray                    # the entry that rides the same transform, -1 = none
    tables: Dict[str, Optional[np.ndarray]]
    work: int                              # the work array
    zpair: int = 0                         # rfft: scratch of the jobs that carry two signals
    half: bool = False                     # SMOOTH: every job of the launch is a half-length transform
    lengths: Optional[np.ndarray] = None   # BLUESTEIN: transform length per job (its chirp filters; int32)
    packed: bool = False                   # BLUESTEIN rfft: the half-length results stay packed IN the spectrum array
    second_pads_as_first: bool = False     # BLUESTEIN rfft: dl2 / wl2 are the device tables dl / wl

    @property
    def count(self) -> int:
        return int(self.jobs.size)


def exclusive_cumsum(sizes) -> np.ndarray:
    """int64 offsets of consecutive blocks of the given sizes: 0, s0, s0 + s1, ..."""
    sizes = np.asarray(sizes, dtype=np.int64)
    off = np.zeros(sizes.size, dtype=np.int64)
    if sizes.size > 1:
        off[1:] = np.cumsum(sizes[:-1])
    return off


def conv_size(need: int, three_pow2: bool = True) -> int:
    """Smallest Bluestein convolution size the library takes (ira_fft_split: 2^k, or 3 * 2^k when allowed) that holds
    `need` distinct lags; at least 16."""
    need = max(int(need), 16)
    m = 1 << int(need - 1).bit_length()
    if three_pow2 and m >= 128 and 3 * (m >> 2) >= need:
        m = 3 * (m >> 2)
    return m


def chunks_of(idx: np.ndarray, bytes_per_job: int, budget: int):
    step = max(1, int(budget // max(1, bytes_per_job)))
    for i in range(0, idx.size, step):
        yield idx[i : i + step]


def chunks_by_size(need: np.ndarray, three_pow2: bool, budget: int):
    """Group element indices by the convolution size they need, then cut each group to the workspace budget."""
    ms = np.array([conv_size(int(v), three_pow2) for v in need], dtype=np.int64)
    for m in sorted(set(ms.tolist())):
        # work + (worst case) one filter per element
        for idx in chunks_of(np.nonzero(ms == m)[0], 16 * m * 2, budget):
            yield int(m), idx


def pair_by_key(idx: np.ndarray, keys: np.ndarray):
    """Pairs of entries of idx whose keys are equal; leftovers are paired with -1.  Order-stable.
    (Array arithmetic: run lengths of the sorted keys, even positions of a run lead a pair -- the metrics pipeline calls
    this for 256 channels per step, and a Python loop per entry was part of what bounds the bundle configuration.)"""
    idx = np.asarray(idx, dtype=np.int64)
    if idx.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    order = idx[np.argsort(keys[idx], kind="stable")]
    sk = keys[order]
    new_run = np.r_[True, sk[1:] != sk[:-1]]
    run_start = np.flatnonzero(new_run)
    run_id = np.cumsum(new_run) - 1
    pos = np.arange(order.size) - run_start[run_id]                  # position inside the run
    run_len = np.diff(np.r_[run_start, order.size])[run_id]
    lead = (pos % 2) == 0
    has_partner = lead & (pos + 1 < run_len)
    first = order[lead]
    nxt = np.r_[order[1:], -1]
    second = np.where(has_partner, nxt, -1)[lead]
    return first.astype(np.int64), second.astype(np.int64)


def pair_bands(keys: np.ndarray, width: np.ndarray):
    """Like pair_by_key over all entries, but a group of odd size leaves its entry of smallest `width` alone (the first
    of them on a tie) and pairs the others in order."""
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    starts = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]]) if order.size else np.zeros(0, dtype=np.int64)
    sizes = np.diff(np.r_[starts, order.size])
    if order.size and np.all(sizes == sizes[0]):
        # every group has the same size (every channel of a report has the same bands): array arithmetic, same output
        # order as the loop below (a group's pairs, then its lone entry)
        g, sz = int(starts.size), int(sizes[0])
        grp = order.reshape(g, sz)
        if sz % 2 == 0:
            return grp[:, 0::2].reshape(-1).astype(np.int64), grp[:, 1::2].reshape(-1).astype(np.int64)
        lone_pos = np.argmin(width[grp], axis=1)                     # the first minimum, like argmin over the group
        keep = np.ones((g, sz), dtype=bool)
        keep[np.arange(g), lone_pos] = False
        rest = grp[keep].reshape(g, sz - 1)
        lone = grp[np.arange(g), lone_pos][:, None]
        first = np.concatenate([rest[:, 0::2], lone], axis=1).reshape(-1)
        second = np.concatenate([rest[:, 1::2], np.full((g, 1), -1, dtype=order.dtype)], axis=1).reshape(-1)
        return first.astype(np.int64), second.astype(np.int64)
    first, second = [], []
    i = 0
    while i < order.size:
        j = i
        while j < order.size and keys[order[j]] == keys[order[i]]:
            j += 1
        grp = order[i:j]
        lone = -1
        if grp.size % 2:
            lone = int(grp[int(np.argmin(width[grp]))])
            grp = grp[grp != lone]
        first.extend(grp[0::2].tolist()); second.extend(grp[1::2].tolist())
        if lone >= 0:
            first.append(lone); second.append(-1)
        i = j
    return np.asarray(first, dtype=np.int64), np.asarray(second, dtype=np.int64)


def _half_length_ok(n: int, sw: Switches, smooth_split: Callable) -> bool:
    """An even smooth length whose half is smooth too can ride a half-length complex transform."""
    return n % 2 == 0 and n >= 128 and sw.half_real_ffts and smooth_split(n // 2) is not None


# ---------------------------------------------------------------------------------------------- forward transforms
def _pairs_of_equal_length(idx: np.ndarray, lengths: np.ndarray, sw: Switches):
    """Two real signals of equal length share a complex transform only across channels (round 2's pairing, A/B)."""
    if sw.pair_real_ffts and sw.pair_across_channels and idx.size > 1:
        return pair_by_key(idx, lengths)
    return idx.astype(np.int64), np.full(idx.size, -1, dtype=np.int64)


def _second_signal_tables(j1, j2, half, jlen, xoff, spec_off):
    """(x2, so2, zo, zpair elements) of a launch whose jobs may carry a second signal: the odd samples of a half-length
    job (x[2m] + i x[2m+1]), or the partner of a paired one, whose spectrum goes to so2.  Every such job has jlen complex
    values of scratch at zo.  All None / 0 when no job carries one."""
    paired = j2 >= 0
    two = paired | half
    if not two.any():
        return None, None, None, 0
    safe = np.maximum(j2, 0)
    x2 = np.where(half, xoff[j1] + 1, np.where(paired, xoff[safe], -1)).astype(np.int64)
    so2 = np.where(paired, spec_off[safe], 0).astype(np.int64)
    zlen = np.where(two, jlen.astype(np.int64), 0)
    return x2, so2, (np.cumsum(zlen) - zlen).astype(np.int64), int(zlen.sum()) * 2


def plan_rfft(xoff: np.ndarray, lengths: np.ndarray, data_len: Optional[np.ndarray], win_len: Optional[np.ndarray],
              packed_ok: bool, sw: Switches, smooth_split: Callable) -> Tuple[np.ndarray, List[Launch], Optional[np.ndarray]]:
    """
    The launches of Engine._rfft_any for elements of the given int32 lengths at the int64 sample offsets xoff (data_len /
    win_len: both int32 arrays, or both None).  Returns (spec_off int64 in complex elements, launches, packed): the
    smooth lengths first, one group of launches per distinct length, then the Bluestein launches by ascending
    convolution size.  packed (int32 per element) marks the elements whose spectrum stays the packed half-length
    transform; None when there is none (always, unless packed_ok).
    """
    n = int(lengths.size)
    padded = data_len is not None
    spec_off = exclusive_cumsum(lengths.astype(np.int64) // 2 + 1)
    launches: List[Launch] = []

    def pads(j1, j2, second=True):
        if not padded:
            return None, None, None, None
        safe = np.maximum(j2, 0)
        return (data_len[j1], win_len[j1]) + ((data_len[safe], win_len[safe]) if second else (None, None))

    # ---- smooth lengths: direct two-pass transform, one call per distinct length ------------------------------------
    # Even lengths whose half is smooth too ride a HALF-length complex transform each (interleave mode); the rest one
    # full-length transform each -- or, with pair_across_channels, two per transform as in round 2.
    rest = np.ones(n, dtype=bool)
    for L in np.unique(lengths):
        L = int(L)
        half_ok = not sw.pair_across_channels and _half_length_ok(L, sw, smooth_split)
        if not (half_ok or smooth_split(L) is not None):
            continue
        grp = np.nonzero(lengths == L)[0]
        rest[grp] = False
        nt = L // 2 if half_ok else L                            # transform length
        # round 4: with an even n1 the untangling of the half-length transform is part of its second pass
        # (mirror-pair tiles, ira_rfft_smooth without zpair scratch); fuse_half_split = False is the A/B
        fused = half_ok and sw.fuse_half_split and smooth_split(nt)[0] % 2 == 0
        for idx in chunks_of(grp, 32 * nt, sw.workspace_budget_bytes):
            j1, j2 = _pairs_of_equal_length(idx, lengths, sw)    # (a half-length job is never paired)
            if fused:
                x2, so2, zo, zpair = None, None, None, 0
            else:
                x2, so2, zo, zpair = _second_signal_tables(j1, j2, np.full(j1.size, half_ok), np.full(j1.size, nt),
                                                           xoff, spec_off)
                if half_ok:
                    so2 = spec_off[j1].astype(np.int64)          # the split pass of the direct transform writes there
            dl, wl, dl2, wl2 = pads(j1, j2, second=not half_ok)
            launches.append(Launch(SMOOTH, nt, j1, j2, dict(xo=xoff[j1], so=spec_off[j1], x2=x2, so2=so2, zo=zo, dl=dl,
                                                            wl=wl, dl2=dl2, wl2=wl2),
                                   work=int(j1.size) * 2 * nt, zpair=zpair, half=half_ok))
    packed = np.zeros(n, dtype=np.int32)
    if not rest.any():
        return spec_off, launches, None
    rest_idx = np.nonzero(rest)[0]
    # ---- everything else: Bluestein, grouped by the convolution size ------------------------------------------------
    # Jobs: "half" = one real signal of EVEN length carried as x[2m] + i*x[2m+1] (a complex transform of L/2: half
    # the convolution size); "pair" = two signals of equal length as x1 + i*x2; "single".
    lr = lengths[rest_idx]
    if sw.half_real_ffts and not padded:
        is_half = (lr % 2 == 0) & (lr >= 8)
    else:
        is_half = np.zeros(rest_idx.size, dtype=bool)
    p1, p2 = _pairs_of_equal_length(rest_idx[~is_half], lengths, sw)
    nh = int(is_half.sum())
    e1 = np.concatenate([rest_idx[is_half].astype(np.int64), p1])
    e2 = np.concatenate([np.full(nh, -1, dtype=np.int64), p2])
    half = np.concatenate([np.ones(nh, dtype=bool), np.zeros(p1.size, dtype=bool)])
    jlen = np.where(half, lengths[e1] // 2, lengths[e1]).astype(np.int32)        # transform length of the job
    # lags the convolution must keep apart: 2 l - 1 when all l outputs of a complex transform are wanted (half and
    # paired jobs), l + l/2 for a single real signal (outputs k <= l/2 only)
    jl64 = jlen.astype(np.int64)
    need = np.where(half | (e2 >= 0), 2 * jl64 - 1, jl64 + jl64 // 2)
    for lm, sel in chunks_by_size(need, sw.three_pow2_sizes, sw.workspace_budget_bytes):
        j1, j2, jh, jl = e1[sel], e2[sel], half[sel], jlen[sel]
        keep_packed = bool(packed_ok and sw.fuse_half_split and jh.any() and not (j2 >= 0).any())
        if keep_packed:
            # the half-length transforms land in the spectrum array itself (L/2 values in the element's L/2 + 1 slots)
            # and stay packed: the dB / phase kernel untangles them as it reads them
            x2 = np.where(jh, xoff[j1] + 1, -1).astype(np.int64)
            so2, zo, zpair = np.zeros(j1.size, dtype=np.int64), spec_off[j1].astype(np.int64), 0
            packed[j1[jh]] = 1
        else:
            x2, so2, zo, zpair = _second_signal_tables(j1, j2, jh, jl, xoff, spec_off)
        dl, wl, dl2, wl2 = pads(j1, j2)
        il = None
        if not padded and jh.any():
            dl = jl
            wl = np.where(jh, lengths[j1], jl).astype(np.int32)       # the Hann window belongs to the REAL signal
            il = jh.astype(np.int32)
        launches.append(Launch(BLUESTEIN, lm, j1, j2, dict(xo=xoff[j1], l=jl, so=spec_off[j1], x2=x2, so2=so2, zo=zo,
                                                           dl=dl, wl=wl, dl2=dl2, wl2=wl2, il=il),
                               work=int(sel.size) * 2 * lm, zpair=zpair, lengths=jl, packed=keep_packed,
                               second_pads_as_first=not padded and dl is not None))
    return spec_off, launches, (packed if (packed_ok and packed.any()) else None)


# ---------------------------------------------------------------------------------------------- band inverses
def band_pairs(spec_off: np.ndarray, lengths: np.ndarray, band_params: np.ndarray, freq_val: np.ndarray, sw: Switches):
    """(j1, j2): which entries of a band_irfft call share an inverse transform (j2 = -1: none)."""
    # pair key: same transform length AND same float64 bin step (AND same spectrum when cross-channel pairing is off)
    cols = [lengths.astype(np.float64), freq_val]
    if not sw.pair_across_channels:
        cols.append(spec_off.astype(np.float64))
    _, key = np.unique(np.stack(cols, axis=1), axis=0, return_inverse=True)
    if sw.pair_real_ffts and sw.sparse_bands:
        # the band left over in a group of odd size is the NARROWEST one (round 4): alone it is a narrow job of the
        # half-length inverse and skips the first pass, paired with a wide neighbour it would not
        kind, width = band_params[:, 0], np.full(lengths.size, np.inf)
        width[kind == 1.0] = band_params[kind == 1.0, 4]
        width[kind == 3.0] = band_params[kind == 3.0, 4] - band_params[kind == 3.0, 1]
        width[(kind != 1.0) & (kind != 2.0) & (kind != 3.0)] = 0.0
        return pair_bands(key.reshape(-1), width)
    if sw.pair_real_ffts:
        return pair_by_key(np.arange(lengths.size), key.reshape(-1))
    return np.arange(lengths.size, dtype=np.int64), np.full(lengths.size, -1, dtype=np.int64)


def plan_band_irfft(spec_off: np.ndarray, lengths: np.ndarray, band_params: np.ndarray, freq_val: np.ndarray,
                    y_off: np.ndarray, sw: Switches, smooth_split: Callable) -> List[Launch]:
    """
    The launches of Engine.band_irfft for entries (spec_off int64, lengths int32, band_params (n, 8) float64, freq_val
    float64, y_off int64): the smooth lengths first -- per length the full-length launches of its pairs, then the
    half-length ones of its single bands -- then the Bluestein launches by ascending convolution size.
    """
    j1, j2 = band_pairs(spec_off, lengths, band_params, freq_val, sw)
    jl = lengths[j1]
    safe = np.maximum(j2, 0)
    has2 = j2 >= 0
    el_par = np.zeros((j1.size, 2, 8), dtype=np.float64)
    el_par[:, 0, :] = band_params[j1]
    el_par[has2, 1, :] = band_params[safe[has2]]
    el_so2 = np.where(has2, spec_off[safe], spec_off[j1]).astype(np.int64)
    el_y2 = np.where(has2, y_off[safe], -1).astype(np.int64)

    def tables(sel, **more):
        return dict(so=spec_off[j1][sel], **more, bp=np.ascontiguousarray(el_par[sel]),
                    fv=np.ascontiguousarray(freq_val[j1][sel]), y1=np.ascontiguousarray(y_off[j1][sel]),
                    y2=np.ascontiguousarray(el_y2[sel]))

    launches: List[Launch] = []
    rest = np.ones(j1.size, dtype=bool)
    for L in np.unique(jl):
        L = int(L)
        full_ok = smooth_split(L) is not None
        half_ok = _half_length_ok(L, sw, smooth_split)
        for halves in (False, True):
            # single bands take the half-length inverse when the length allows it, pairs the full-length one
            if not (half_ok if halves else full_ok):
                continue
            grp = np.nonzero((jl == L) & rest & ((~has2) if halves else (has2 | (not half_ok))))[0]
            rest[grp] = False
            nt = L // 2 if halves else L
            for sel in chunks_of(grp, 16 * nt, sw.workspace_budget_bytes):
                t = tables(sel, so2=None if halves else np.ascontiguousarray(el_so2[sel]))
                launches.append(Launch(SMOOTH, nt, j1[sel], j2[sel], t, work=int(sel.size) * 2 * nt, half=halves))
    rest_idx = np.nonzero(rest)[0]
    for lm, sub in chunks_by_size(2 * jl[rest_idx].astype(np.int64) - 1, sw.three_pow2_sizes, sw.workspace_budget_bytes):
        sel = rest_idx[sub]
        t = tables(sel, l=jl[sel], so2=np.ascontiguousarray(el_so2[sel]))
        launches.append(Launch(BLUESTEIN, lm, j1[sel], j2[sel], t, work=int(sel.size) * 2 * lm, lengths=jl[sel]))
    return launches
