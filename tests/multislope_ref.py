"""Reference for the multi-slope kernels (ira_multislope.hip): a long-double NumPy restatement of the algorithm the docstring
of audio_analysis_amd/analyse/multislope.py pins, written from that text and sharing no code with the module or the kernels
(imported by name, like lundeby_ref.py; tests/test_multislope_cpu.py pins it on a machine without a GPU).

Besides the results, search() returns its DECISION MARGIN:
  lead    the relative cost lead (c_other - c_winner) / c_other of the winner over the best other admissible candidate;
  reject  over the winner's own pivots and coefficients, over every candidate rejected by a pivot, and over every candidate
          rejected by a coefficient whose cost undercuts the winner's: the relative distance of what decided from its
          threshold (a pivot p against 1e-12 diag: |p / (1e-12 diag) - 1|; a coefficient against 0: |a_k| sqrt(G_kk / J),
          the root-mean-square share of its term in the fitted curve, which is 1 for a perfect fit; for a rejected
          candidate the largest such distance among its non-positive coefficients);
  ratio   the distance |T_k / (min_ratio T_i) - 1| of every min_ratio comparison from equality.
Integer outputs of a float64 kernel (indices, the noise flag, the "no candidate" bit) are only comparable on inputs whose
margins are at least MARGIN: a condition on the input.
"""
import math

import numpy as np

LD = np.longdouble
LONGDOUBLE_OK = bool(np.finfo(LD).eps < 2e-19)
MARGIN = 1e-6
MAX_BLOCKS = 4096
MIN_BLOCKS = 32
R = 3
PIVOT = LD(10) ** -12
S_SILENT, S_SHORT, S_ZERO, S_NON_FINITE = 1, 2, 4, 16
LN1E6 = np.log(LD(10)) * 6


def need_longdouble():
    import pytest
    if not LONGDOUBLE_OK:
        pytest.skip("np.longdouble has no 64-bit mantissa on this machine: no reference more precise than float64")


def block_size(fs, length):
    return max(-(-int(fs) // 1000), -(-int(length) // MAX_BLOCKS))


def block_energies(y, b):
    e = np.asarray(y, np.float32).astype(LD) ** 2
    nb = e.size // b
    return e[: nb * b].reshape(nb, b).sum(axis=1), e[nb * b:].sum()


def suffix_sums(E, tail):
    """d[j] = tail + E[nb - 1] + ... + E[j]"""
    return (np.cumsum(np.concatenate([[LD(tail)], np.asarray(E, LD)[::-1]]))[1:])[::-1]


def row_points(y, fs, fit_fraction=0.9, b=None):
    """Step 1 and the row status of step 8 for a row y (float32, from its start index on): dict(status, L, B, nb, J, d)."""
    y = np.asarray(y, np.float32)
    L = int(y.size)
    b = int(b) if b else block_size(fs, L)
    nb = L // b
    out = dict(status=0, L=L, B=b, nb=nb, J=0, d=None)
    if nb < MIN_BLOCKS:
        out["status"] = S_SHORT
        return out
    E, tail = block_energies(y, b)
    if not (np.all(np.isfinite(E.astype(np.float64))) and np.isfinite(float(tail))):
        out["status"] = S_NON_FINITE
        return out
    d = suffix_sums(E, tail)
    J = max(1, int(math.floor(float(fit_fraction) * nb)))
    out.update(J=J, d=d)
    if d[0] == 0:
        out["status"] = S_SILENT
    elif d[J - 1] == 0:
        out["status"] = S_ZERO
    return out


def basis(grid, fs, L, B, J, d):
    """u (J, g + 1): the g decays of the grid (seconds), then the noise term."""
    t = (np.arange(J, dtype=np.int64) * int(B)).astype(LD)
    lam = LN1E6 / (np.asarray(grid, np.float64).astype(LD) * LD(fs))
    with np.errstate(under="ignore"):
        phi = np.exp(-lam[None, :] * t[:, None]) - np.exp(-lam * LD(L))[None, :]
    nu = (LD(L) - t) / LD(L)
    return np.concatenate([phi, nu[:, None]], axis=1) / np.asarray(d, LD)[:J, None]


def gram(u):
    """(G (g + 1, g + 1), b (g + 1))"""
    with np.errstate(under="ignore"):
        return u.T @ u, u.sum(axis=0)


def _candidates(T, S, min_ratio, mg):
    """(N, S) index tuples in lexicographic order; every ratio comparison counts towards mg['ratio']"""
    T = np.asarray(T, np.float64).astype(LD)
    g = T.size
    if g >= 2:
        i, k = np.triu_indices(g, 1)
        with np.errstate(all="ignore"):
            dist = np.abs((T[k] / (LD(min_ratio) * T[i]) - 1).astype(np.float64))
        if dist.size:
            mg["ratio"] = min(mg["ratio"], float(dist.min()))
    ok = T[None, :] >= LD(min_ratio) * T[:, None]                      # ok[i, k]: k may follow i
    ok &= np.arange(g)[None, :] > np.arange(g)[:, None]
    cur = np.arange(g, dtype=np.int64)[:, None]
    for _ in range(S - 1):
        rows = []
        for tup in cur:
            nxt = np.flatnonzero(ok[tup[-1]])
            if nxt.size:
                rows.append(np.concatenate([np.repeat(tup[None, :], nxt.size, axis=0), nxt[:, None]], axis=1))
        cur = np.concatenate(rows, axis=0) if rows else np.zeros((0, cur.shape[1] + 1), np.int64)
    return cur


def _solve(G, b, V):
    """Batched Cholesky solve of the normal equations of the functions V (N, M).  Returns pivots_ok (N,), pivot distance
    (N,) (the smallest |p / (1e-12 diag) - 1| of the candidate's pivots up to and including the first failing one), a (N, M),
    b^T a (N,); a and b^T a are meaningless where a pivot failed."""
    N, M = V.shape
    Lm = [[None] * M for _ in range(M)]
    y = [None] * M
    alive = np.ones(N, bool)
    pdist = np.full(N, np.inf)
    with np.errstate(all="ignore"):
        for r in range(M):
            for c in range(r):
                s = G[V[:, r], V[:, c]].copy()
                for k in range(c):
                    s -= Lm[r][k] * Lm[c][k]
                Lm[r][c] = s / Lm[c][c]
            diag = G[V[:, r], V[:, r]]
            p = diag.copy()
            for k in range(r):
                p -= Lm[r][k] * Lm[r][k]
            dist = np.abs((p / (PIVOT * diag) - 1).astype(np.float64))
            dist = np.where(np.isfinite(dist), dist, np.inf)
            pdist = np.where(alive, np.minimum(pdist, dist), pdist)
            alive &= p > PIVOT * diag
            Lm[r][r] = np.sqrt(np.where(alive, p, LD(1)))
            s = b[V[:, r]].copy()
            for k in range(r):
                s -= Lm[r][k] * y[k]
            y[r] = s / Lm[r][r]
        a = [None] * M
        for r in range(M - 1, -1, -1):
            s = y[r].copy()
            for k in range(r + 1, M):
                s -= Lm[k][r] * a[k]
            a[r] = s / Lm[r][r]
        a = np.stack(a, axis=1) if N else np.zeros((0, M), LD)
        bta = (b[V] * a).sum(axis=1)
    return alive, pdist, a, bta


def search(G, b, T, J, S, min_ratio=1.5):
    """Step 4 on a Gram matrix over the grid T (seconds, ascending) plus the noise term.  dict: found, idx (tuple), noise,
    T (float64 tuple), a (long double (S,)), a_nu, c, margin (dict lead / reject / ratio), candidates (with both variants)."""
    G, b = np.asarray(G, LD), np.asarray(b, LD)
    T = np.asarray(T, np.float64)
    g = T.size
    mg = dict(lead=math.inf, reject=math.inf, ratio=math.inf)
    cand = _candidates(T, S, min_ratio, mg)
    out = dict(found=False, idx=(), noise=False, T=(), a=None, a_nu=LD(0), c=LD("nan"), margin=mg, candidates=2 * cand.shape[0])
    if cand.shape[0] == 0:
        return out
    recs = []
    for variant, V in ((0, np.concatenate([cand, np.full((cand.shape[0], 1), g, np.int64)], axis=1)), (1, cand)):
        alive, pdist, a, bta = _solve(G, b, V)
        with np.errstate(all="ignore"):
            c = np.maximum(LD(J) - bta, LD(0))
            pos = np.all((a > 0) & np.isfinite(a.astype(np.float64)), axis=1)
            rel = np.abs(a) * np.sqrt(G[V, V] / LD(J))
        recs.append(dict(variant=variant, alive=alive, pdist=pdist, a=a, c=c, ok=alive & pos, rel=rel.astype(np.float64)))
    # the winner: smallest cost, then lexicographic order, the noise variant first
    inf = LD(np.inf)
    flat = np.stack([np.where(rc["ok"], rc["c"], inf) for rc in recs], axis=1).reshape(-1)
    k = int(np.argmin(flat))                                            # the first of equal minima: (n, variant) order
    best = (flat[k], k // 2, recs[k % 2]) if np.isfinite(float(flat[k])) else None
    for rc in recs:                                                     # pivot rejections count whatever their cost
        dead = ~rc["alive"]
        if dead.any():
            mg["reject"] = min(mg["reject"], float(rc["pdist"][dead].min()))
    if best is None:
        for rc in recs:                                                 # every candidate rejected: each rejection must be robust
            neg = rc["alive"] & ~rc["ok"]
            if neg.any():
                worst = np.where(rc["a"][neg] > 0, 0.0, rc["rel"][neg]).max(axis=1)
                mg["reject"] = min(mg["reject"], float(worst.min()))
        return out
    cw, nw, rw = best
    mg["reject"] = min(mg["reject"], float(rw["pdist"][nw]), float(rw["rel"][nw].min()))
    others = []
    for rc in recs:
        m = rc["ok"].copy()
        if rc is rw:
            m[nw] = False
        if m.any():
            others.append(rc["c"][m].min())
        neg = rc["alive"] & ~rc["ok"] & (rc["c"] < cw)
        if neg.any():
            worst = np.where(rc["a"][neg] > 0, 0.0, rc["rel"][neg]).max(axis=1)
            mg["reject"] = min(mg["reject"], float(worst.min()))
    if others:
        c2 = min(others)
        mg["lead"] = float((c2 - cw) / c2) if c2 > 0 else 0.0
    idx = tuple(int(i) for i in cand[nw])
    a = rw["a"][nw]
    out.update(found=True, idx=idx, noise=rw["variant"] == 0, T=tuple(float(T[i]) for i in idx), a=a[:S].copy(),
               a_nu=a[S] if rw["variant"] == 0 else LD(0), c=cw)
    return out


def margin_ok(mg):
    return mg["lead"] >= MARGIN and mg["reject"] >= MARGIN and mg["ratio"] >= MARGIN


def level0(t_min=0.05, t_max=20.0, G=64):
    """(grid float64, h_0)"""
    if G == 1:
        return np.array([t_min], np.float64), 0.0
    k = np.arange(G).astype(LD)
    grid = LD(t_min) * (LD(t_max) / LD(t_min)) ** (k / LD(G - 1))
    return grid.astype(np.float64), float(np.log(LD(t_max) / LD(t_min)) / LD(G - 1))


def refined(Ts, step):
    """The ascending union of T exp(k step), k = -R .. R, rounded to float64 (a grid is float64 data); k = 0 is T itself."""
    vals = []
    for T in Ts:
        for k in range(-R, R + 1):
            vals.append(float(T) if k == 0 else float(LD(float(T)) * np.exp(LD(k) * LD(float(step)))))
    return np.unique(np.array(vals, np.float64))


def fit_points(d, J, L, B, fs, grid, S, min_ratio=1.5):
    """Steps 2 to 4 on given points."""
    G, b = gram(basis(grid, fs, L, B, J, d))
    return search(G, b, grid, J, S, min_ratio)


def chain(pts, fs, max_order=3, t_min=0.05, t_max=20.0, G=64, refine_levels=3, min_ratio=1.5):
    """Step 5 on the points of row_points (status 0): {order: [search result per level]}; a level after one without a winner
    repeats found=False.  Each result also carries 'grid' (the float64 grid it searched) and 'step' (that grid's step)."""
    grid0, h = level0(t_min, t_max, G)
    G0, b0 = gram(basis(grid0, fs, pts["L"], pts["B"], pts["J"], pts["d"]))
    out = {}
    for S in range(1, max_order + 1):
        res = search(G0, b0, grid0, pts["J"], S, min_ratio)
        res.update(grid=grid0, step=h)
        levels, step = [res], h
        for _ in range(refine_levels):
            step = step / (R + 1)
            prev = levels[-1]
            if not prev["found"]:
                levels.append(dict(prev))
                continue
            grid = refined(prev["T"], step)
            res = fit_points(pts["d"], pts["J"], pts["L"], pts["B"], fs, grid, S, min_ratio)
            res.update(grid=grid, step=step)
            levels.append(res)
        out[S] = levels
    return out


def rms_db(c, J):
    return float((LD(10) / np.log(LD(10))) * np.sqrt(LD(c) / LD(J)))


def finish(res, pts, fs):
    """Step 6 from a search result: dict(rms_db, start_db (S,), noise_db, turn_s (S - 1,), turn_db (S - 1,)), float64."""
    S = len(res["idx"])
    L, d0 = LD(pts["L"]), pts["d"][0]
    lam = [LN1E6 / (LD(t) * LD(fs)) for t in res["T"]]
    a = res["a"]
    start = [float(10 * np.log10(a[s] * (1 - np.exp(-lam[s] * L)) / d0)) for s in range(S)]
    noise = float(10 * np.log10(res["a_nu"] / d0)) if res["a_nu"] > 0 else -math.inf
    turn_s, turn_db = [], []
    for s in range(S - 1):
        tx = np.log(a[s] / a[s + 1]) / (lam[s] - lam[s + 1])
        if tx > 0:
            turn_s.append(float(tx / LD(fs)))
            turn_db.append(float(10 * np.log10(a[s] * np.exp(-lam[s] * tx) / d0)))
        else:
            turn_s.append(math.nan)
            turn_db.append(math.nan)
    return dict(rms_db=rms_db(res["c"], pts["J"]), start_db=start, noise_db=noise, turn_s=turn_s, turn_db=turn_db)


def preferred(rms_by_order, accept=0.15):
    for s in sorted(rms_by_order):
        if rms_by_order[s] <= accept:
            return s
    return max(rms_by_order) if rms_by_order else 0


def model_points(L, B, J_of, fs, Ts, a, a_nu):
    """Exact model curve d[j] = sum a_s phi_{T_s}(j B) + a_nu nu(j B) for j < nb, long double."""
    nb = L // B
    t = (np.arange(nb, dtype=np.int64) * B).astype(LD)
    d = LD(a_nu) * (LD(L) - t) / LD(L)
    for T, c in zip(Ts, a):
        lam = LN1E6 / (LD(T) * LD(fs))
        d = d + LD(c) * (np.exp(-lam * t) - np.exp(-lam * LD(L)))
    return d


def multi_decay_noise(fs, seconds, rts, levels_db, noise_db, seed):
    """Gaussian noise under a sum of exponential energy envelopes (reverberation times rts, start levels levels_db relative
    to the first) plus a stationary floor noise_db below the first envelope's start (None: no floor).  Independent noise per
    envelope: the energies add in expectation."""
    rng = np.random.default_rng(seed)
    n = int(round(fs * seconds))
    t = np.arange(n) / float(fs)
    x = np.zeros(n)
    for rt, lev in zip(rts, levels_db):
        x += rng.standard_normal(n) * 10.0 ** (lev / 20.0) * 10.0 ** (-3.0 * t / rt)
    if noise_db is not None:
        x += rng.standard_normal(n) * 10.0 ** (noise_db / 20.0)
    return (0.5 * x).astype(np.float32)
