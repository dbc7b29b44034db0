"""
What tests/test_gpu_mls_kernels.py launches and how it judges the answers, with a NumPy emulation of the kernels of
audio_analysis_amd/csrc/ira_mls.hip as they are written, so that tests/test_mls_kernels_ref_cpu.py can show on a machine
without a GPU that an honest kernel passes every case and that named wrong kernels fall at named cases.  Helper module,
like minphase_kernels_ref.py: it holds no tests.

What is here
  * the case tables HADAMARD_CASES, FOLD_CASES, FINISH_CASES and MASK_CASES -- the GPU file parametrises over them and the
    CPU file names its rejecting cases from them, so the two cannot drift apart;
  * rows / fold_input / finish_input / probe_rows: the inputs of a case, from its seed;
  * check_hadamard / check_probes / check_fold / check_finish / check_guard: the assertions, on whatever produced the
    answer;
  * rounds / schedule: how had_tile_stages splits the stages first .. last - 1 into rounds, derived from the constants
    alone (T = IRA_MLS_TILE_LOG2 from include/ira.h, four register bits, the coalesced base 8, engine.mls_pass_plan);
  * emulate / emu_fold / emu_finish: the kernels thread by thread -- tiles of 2^T consecutive doubles with zero fill past
    `total`, the element-of-register map had_elem, the LDS slot map, the exchanges, the further pass's address
    (e >> cbits) << lo | e & (2^cbits - 1) and its hi / run split of the block index; the fold's grid-stride loop, xor
    butterfly, four waves and ascending workgroups; the finish's stride loop.  `wrong` selects one named deviation.

Every launch buffer is modelled the way tests/guard_buffers.py lays it out: sentinel words behind the last element, so a
store a wrong kernel makes past its segment is seen exactly as the device test would see it.
"""
import re
from pathlib import Path

import numpy as np

import mls_ref as R
from guard_buffers import GUARD, sentinel, words

REPO = Path(__file__).resolve().parent.parent


def _header(name):
    return int(re.search(rf"#define IRA_MLS_{name} (\d+)\b", (REPO / "include" / "ira.h").read_text()).group(1))


T = _header("TILE_LOG2")                          # 12: the tile order
TILE = 1 << T
REG_BITS = 4                                      # index bits a round holds in registers
REGS = 1 << REG_BITS
THREADS = TILE // REGS
COAL = 8                                          # the round whose layout is the coalesced one: element j * THREADS + t
FOLD_THREADS, FOLD_BLOCKS, MAX_PERIODS = _header("FOLD_THREADS"), _header("FOLD_BLOCKS"), _header("MAX_PERIODS")
WAVE = 64
ORDERS = tuple(range(_header("MIN_ORDER"), _header("MAX_ORDER") + 1))

# ------------------------------------------------------------------------------------------------------- the case tables
# (order, nb): every order at 1 and 3 rows (the batch of 3 holds the NaN row), 65 rows while that stays small, the three-pass
# order at 1 and 2
HADAMARD_CASES = tuple((m, nb) for m in ORDERS for nb in ((1, 3, 65) if m <= T + 1 else (1, 3) if m < ORDERS[-1] else (1, 2)))
# (order, periods, nb).  Orders 16, 17 and 21 give a thread 2, 4 and 64 samples; 1024 is the most periods a call takes;
# 65 and 130 channels reach the second and third workgroup of the sums kernel
FOLD_CASES = (tuple((m, r, 4) for m in (2, 5, T + 1) for r in (1, 2, 5)) + tuple((m, r, 4) for m in (16, 17) for r in (1, 2))
              + ((21, 1, 2), (21, 2, 2), (2, 1024, 4), (2, 1023, 4), (5, 1024, 4), (5, 1023, 4), (3, 2, 65), (3, 2, 130)))
FINISH_CASES = (tuple((m, r, 3) for m in (2, 5, T + 1) for r in (1, 2, 5))
                + ((16, 2, 3), (16, 1024, 3), (21, 1, 1), (21, 1024, 1), (5, 1024, 3)))
MASK_CASES = ((5, 2), (T + 1, 2))                 # (order, nb): tables with bit m set in a third of their entries
BEGINS = (1, 3, 0, 7)                             # with the gaps of the layout: every alignment of the loads


def rows(rng, nb, order):
    """Random float64 rows over many binades with signed zeros and denormals; the last row of a batch of 3 holds a NaN."""
    n = 1 << order
    w = rng.standard_normal((nb, n)) * np.exp2(rng.integers(-40, 40, (nb, n)).astype(np.float64))
    w[:, 0] = 0.0
    w[:, 1 % n] = -0.0
    if n >= 8:
        w[:, 5] = 5e-324
        w[:, 6] = -2.5e-310
        w[:, 7] = 0.0
    if nb == 3:
        w[2, n // 2] = np.nan
    return w


def hadamard_input(order, nb):
    return rows(np.random.default_rng(100 * order + nb), nb, order)


def fold_input(order, periods, nb):
    """(channels, begins) of a fold case."""
    p = (1 << order) - 1
    rng = np.random.default_rng(10 * order + periods + (0 if nb == 4 else 1000 * nb))
    begins = [BEGINS[c % 4] for c in range(nb)]
    return [rng.standard_normal(b + periods * p + 2).astype(np.float32) for b in begins], begins


def finish_input(order, periods, nb):
    rng = np.random.default_rng(7 * order + periods)
    wt = rng.standard_normal((nb, 1 << order)) * np.exp2(rng.integers(-30, 30, (nb, 1 << order)).astype(np.float64))
    if nb > 1:
        wt[1, 3] = np.nan
    return wt


def stray(table, order, seed):
    """The table with bit `order` set in a seeded third of its entries: the same values under the kernels' mask."""
    t = np.array(table, dtype=np.int32)
    t[np.random.default_rng(seed).random(t.size) < 1.0 / 3.0] |= np.int32(1 << order)
    return t


# ---------------------------------------------------------------------------------------------------------- the probes
def probe_indices(order):
    """1, every power of two below 2^m, 2^m - 1."""
    return sorted({1, (1 << order) - 1} | {1 << b for b in range(order)})


def probe_rows(order, indices):
    w = np.zeros((len(indices), 1 << order))
    w[np.arange(len(indices)), indices] = 1.0
    return w


def walsh_row(order, i):
    """(-1)^popcount(i & k), k < 2^m: the transform of the unit impulse at i, exactly."""
    x = np.arange(1 << order, dtype=np.int64) & i
    for s in (16, 8, 4, 2, 1):
        x ^= x >> s
    return 1.0 - 2.0 * (x & 1)


def broken_stages(g, order, i):
    """The bits b whose butterfly relation W[k ^ 2^b] = (-1)^(bit b of i) W[k] fails in the transform g of the unit impulse
    at i.  A missing stage, or one run twice, leaves the impulse unspread along its bit: zeros at the partners."""
    out = []
    for b in range(order):
        v = g.reshape(-1, 2, 1 << b)
        if not np.array_equal(v[:, 1], (-1.0 if (i >> b) & 1 else 1.0) * v[:, 0]):
            out.append(b)
    return out


def check_probes(got, order, indices, what="probes"):
    """Every probe's transform is its Walsh row to the bit.  A wrong stage spoils every probe, so on failure the message
    gives the lowest bit whose probe differs and, from that probe, the stages whose butterfly relation fails."""
    bad = [(i, g) for i, g in zip(indices, got) if not np.array_equal(words(g), words(walsh_row(order, i)))]
    if bad:
        single = [i.bit_length() - 1 for i, _ in bad if i & (i - 1) == 0]
        i, g = bad[0]
        raise AssertionError(f"{what} order {order}: the impulses at {[i for i, _ in bad]} do not give their Walsh rows; "
                             f"lowest bit whose probe differs: {min(single) if single else 'none (only the all-ones probe)'}; "
                             f"stages broken in the probe at {i}: {broken_stages(g, order, i)}")


# ---------------------------------------------------------------------------------------------------------- the checks
def check_guard(tail, what):
    """The elements behind a segment still hold the sentinel (what Flat.split asserts of every guard and gap)."""
    tail = np.ascontiguousarray(tail)
    bad = words(tail) != words(sentinel(1, tail.dtype))[0]
    assert not bad.any(), f"{what}: {int(bad.sum())} elements written outside the segments"


def check_hadamard(got, w, order):
    nb = w.shape[0]
    ref = R.fwht(w)
    same = (words(got) == words(ref)) | (np.isnan(got) & np.isnan(ref))
    assert same.all(), f"order {order}, nb {nb}: {int((~same).sum())} values differ, first at {int(np.argmax(~same))}"
    if nb == 3:
        assert np.isnan(got[2]).all() and np.isfinite(got[:2]).all()       # the NaN fills its row and no other


def sum_chain(order, periods):
    """The longest chain of additions behind E or D, from the kernel's block sizes: a thread's own terms, the wave tree
    (6), the 4 waves (3), the workgroups of the channel.  ceil(P / (B 256)) R + 6 + 3 + B."""
    p = (1 << order) - 1
    blocks = min(-(-p // FOLD_THREADS), FOLD_BLOCKS)
    return blocks, -(-p // (blocks * FOLD_THREADS)) * periods + 6 + 3 + blocks


def check_fold(rows_, sums, chans, begins, order, periods, g, show=print):
    """Y through G and w[0] = +0.0 to the bit; E and D within gamma(chain) of the long-double sums of their float64
    terms.  Returns the worst (E, D) error over its bound."""
    p = (1 << order) - 1
    _, chain = sum_chain(order, periods)
    worst = [0.0, 0.0]
    for c, (x, b) in enumerate(zip(chans, begins)):
        y = R.fold(x, b, p, periods)
        assert np.array_equal(words(rows_[c]), words(R.scatter(y, g, order))), f"channel {c}: Y through G"
        assert words(rows_[c, :1])[0] == 0                                     # w[0] = +0.0
        e_ld, d_ld, e_abs, d_abs = R.sums_ld(x, b, p, periods)
        e_err, d_err = abs(np.longdouble(sums[c, 0]) - e_ld), abs(np.longdouble(sums[c, 1]) - d_ld)
        e_rel = float(e_err / (R.gamma(chain) * e_abs))
        d_rel = float(d_err / (R.gamma(chain) * d_abs)) if periods > 1 else 0.0
        if c < 4:
            show(f"order {order} R {periods} channel {c}: E err/bound {e_rel:.3f}"
                 + (f", D err/bound {d_rel:.3f}" if periods > 1 else ""))
        assert e_err <= R.gamma(chain) * e_abs, f"channel {c}: E"
        assert d_err <= R.gamma(chain) * d_abs, f"channel {c}: D"
        if periods == 1:
            assert sums[c, 1] == 0.0
        worst = [max(worst[0], e_rel), max(worst[1], d_rel)]
    return tuple(worst)


def check_finish(got, wt, out, order, periods):
    for c in range(wt.shape[0]):
        ref = R.finish(wt[c], out, order, periods)[1]
        same = (words(got[c]) == words(ref)) | (np.isnan(got[c]) & np.isnan(ref))
        assert same.all(), f"channel {c}: {int((~same).sum())} samples differ"


# ------------------------------------------------------------------------------------------------- the transform, emulated
HADAMARD_WRONG = ("drop_top", "guard_dropped", "descending", "unclamped_base", "ignore_hi", "row_shift_12", "store_whole_tile")


def had_slot(e):
    return e ^ ((e >> 4) & 31)


def had_elem(t, j, base):
    """The tile element in register j of thread t while the register index holds the tile's bits base .. base + 3."""
    return ((t >> base) << (base + REG_BITS)) | (j << base) | (t & ((1 << base) - 1))


def _slots(base):
    t, j = np.arange(THREADS)[:, None], np.arange(REGS)[None, :]
    return had_slot(had_elem(t, j, base)).reshape(-1)


def rounds(first, last, wrong=None):
    """[(round base, [register bits staged])] of had_tile_stages(first, last): a round starts at the next bit q, its base
    clamped to the coalesced one, and takes the bits up to base + 3 or last - 1."""
    out, q = [], first
    while q < last:
        base = q if q < COAL or wrong == "unclamped_base" else COAL
        end = min(base + REG_BITS, last)
        regs = [r for r in range(REG_BITS)
                if q <= base + r and (base + r < end or (wrong == "guard_dropped" and r == REG_BITS - 1))]
        if wrong == "drop_top" and len(regs) < REG_BITS:
            regs = regs[:-1]                                   # a partial round loses its top stage
        if wrong == "descending":
            regs = regs[::-1]
        out.append((base, regs))
        q = end
    return out


def schedule(order, plan=None):
    """[(pass, round base, absolute bits staged in that round)] of ira_mls_hadamard at this order."""
    from audio_analysis_amd.engine import mls_pass_plan
    out = []
    for k, (lo, a) in enumerate(plan or mls_pass_plan(order)):
        first, last = (0, a) if k == 0 else (T - a, T)
        out += [(k, base, [lo + base + r - first for r in regs]) for base, regs in rounds(first, last)]
    return out


def _stage(v, r):
    """had_stage<r> on registers v (tiles, THREADS, REGS), in place."""
    s = v.reshape(v.shape[0], THREADS, REGS >> (r + 1), 2, 1 << r)
    lo, hi = s[..., 0, :].copy(), s[..., 1, :].copy()
    s[..., 0, :] = lo + hi
    s[..., 1, :] = lo - hi


def _exchange(v, lds, frm, to):
    n = v.shape[0]
    lds[:, _slots(frm)] = v.reshape(n, -1)
    return np.ascontiguousarray(lds[:, _slots(to)]).reshape(n, THREADS, REGS)


def tile_stages(v, first, last, wrong=None):
    """had_tile_stages on registers v (tiles, THREADS, REGS) in the coalesced layout; returns the registers after."""
    # the clamp's absence indexes LDS past the tile: model a larger array of sentinels so the reads have something to find
    lds = sentinel(v.shape[0] * TILE * (8 if wrong == "unclamped_base" else 1), np.float64).reshape(v.shape[0], -1)
    cur = COAL
    for base, regs in rounds(first, last, wrong):
        if base != cur:
            v = _exchange(v, lds, cur, base)
        cur = base
        for r in regs:
            _stage(v, r)
    if cur != COAL:
        v = _exchange(v, lds, cur, COAL)
    return v


def _to_regs(tiles):
    """(n, TILE) in element order -> registers of the coalesced layout: element j * THREADS + t in register j of thread t."""
    return np.ascontiguousarray(tiles.reshape(-1, REGS, THREADS).transpose(0, 2, 1))


def _from_regs(v):
    return v.transpose(0, 2, 1).reshape(-1, TILE)


def _low_pass(buf, total, bits, wrong):
    n = -(-total // TILE)
    idx = np.arange(n * TILE)
    v = _to_regs(np.where(idx < total, buf[: n * TILE], 0.0))
    v = _from_regs(tile_stages(v, 0, bits, wrong)).reshape(-1)
    keep = idx < (n * TILE if wrong == "store_whole_tile" else total)
    buf[: n * TILE][keep] = v[keep]


def _high_pass(buf, nb, order, lo, a, wrong):
    cbits = T - a
    runs = lo - cbits
    bx = np.arange(1 << (order - T), dtype=np.int64)
    hi, run = bx >> runs, bx & ((1 << runs) - 1)
    if wrong == "ignore_hi":
        hi = np.zeros_like(hi)
    e = np.arange(TILE, dtype=np.int64)
    at = ((e >> cbits) << lo) | (e & ((1 << cbits) - 1))
    for y in range(nb):
        row = (y << (T if wrong == "row_shift_12" else order)) + (hi << (lo + a)) + (run << cbits)
        idx = row[:, None] + at[None, :]
        buf[idx] = _from_regs(tile_stages(_to_regs(buf[idx]), cbits, T, wrong))


def emulate(w, order, wrong=None, plan=None):
    """ira_mls_hadamard on rows w (nb, 2^m): (the rows after, the GUARD elements behind them)."""
    from audio_analysis_amd.engine import mls_pass_plan
    nb = w.shape[0]
    total = nb << order
    buf = sentinel(-(-total // TILE) * TILE + TILE, np.float64)
    buf[:total] = w.reshape(-1)
    with np.errstate(all="ignore"):
        for k, (lo, a) in enumerate(plan or mls_pass_plan(order)):
            if k == 0:
                _low_pass(buf, total, a, wrong)
            else:
                _high_pass(buf, nb, order, lo, a, wrong)
    return buf[:total].reshape(nb, -1).copy(), buf[total : total + GUARD].copy()


# ----------------------------------------------------------------------------------------------- fold and finish, emulated
FOLD_WRONG = ("block_stride", "uncapped_blocks", "unmasked")
FINISH_WRONG = ("no_stride", "unmasked")


def _wave_sum(v):
    """ira::wave_sum over the last axis of 64 lanes: v += v[lane ^ o], o = 32, 16 .. 1."""
    lane = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v


def emu_fold(chans, begins, order, periods, g, wrong=None, spare=0):
    """ira_mls_fold: (workspace rows (nb + spare, 2^m), sums (nb, 2), the GUARD elements behind the workspace).  Rows no
    thread wrote hold the sentinel."""
    nb, p = len(chans), (1 << order) - 1
    blocks, _ = sum_chain(order, periods)
    stride = FOLD_THREADS * (1 if wrong == "block_stride" else blocks)
    wbuf = sentinel(((nb + spare) << order) + GUARD, np.float64)
    uncapped = -(-p // FOLD_THREADS)
    part = sentinel(2 * nb * uncapped + GUARD, np.float64)
    g = np.asarray(g, dtype=np.int64)
    n0 = (np.arange(blocks)[:, None] * FOLD_THREADS + np.arange(FOLD_THREADS)[None, :]).reshape(-1)
    with np.errstate(all="ignore"):
        for e, (x, b) in enumerate(zip(chans, begins)):
            src = np.asarray(x, dtype=np.float32)[b:].astype(np.float64)
            se, sd = np.zeros(n0.size), np.zeros(n0.size)
            for i in range(-(-p // stride)):
                n = n0 + i * stride
                live = n < p
                n = n[live]
                y = np.zeros(n.size)
                for r in range(periods):
                    y = y + src[r * p + n]
                if periods > 1:
                    q = y / float(periods)
                    acc = sd[live]
                    for r in range(periods):
                        d = src[r * p + n] - q
                        acc = acc + d * d
                    sd[live] = acc
                se[live] = se[live] + y * y
                wbuf[(e << order) + (g[n] if wrong == "unmasked" else g[n] & p)] = y
            wbuf[e << order] = 0.0
            for s, col in ((se, 0), (sd, 1)):
                waves = _wave_sum(s.reshape(blocks, FOLD_THREADS // WAVE, WAVE))[..., 0]
                tot = waves[:, 0]
                for v in range(1, FOLD_THREADS // WAVE):
                    tot = tot + waves[:, v]
                part[2 * (e * blocks + np.arange(blocks)) + col] = tot
        nblk = uncapped if wrong == "uncapped_blocks" else blocks
        sums = np.zeros((nb, 2))
        for e in range(nb):
            for k in range(nblk):
                sums[e] = sums[e] + part[2 * (e * nblk + k) : 2 * (e * nblk + k) + 2]
    total = (nb + spare) << order
    return wbuf[:total].reshape(nb + spare, -1).copy(), sums, wbuf[total:].copy()


def emu_finish(wt, out, order, periods, wrong=None, nb=None):
    """ira_mls_finish on the first nb rows of wt (all of them by default; a spare row may lie behind): [P float32 per
    channel]; a sample no thread wrote holds the sentinel."""
    p = (1 << order) - 1
    blocks, _ = sum_chain(order, periods)
    out = np.asarray(out, dtype=np.int64)
    flat = np.ascontiguousarray(wt).reshape(-1)
    scale = float(1 << order) * float(periods)
    k0 = np.arange(blocks * FOLD_THREADS)
    res = []
    with np.errstate(all="ignore"):
        for e in range(wt.shape[0] if nb is None else nb):
            h = sentinel(p, np.float32)
            for i in range(1 if wrong == "no_stride" else -(-p // k0.size)):
                k = k0 + i * k0.size
                k = k[k < p]
                at = (e << order) + (out[k] if wrong == "unmasked" else out[k] & p)
                h[k] = ((flat[np.minimum(at, flat.size - 1)] - flat[e << order]) / scale).astype(np.float32)
            res.append(h)
    return res
