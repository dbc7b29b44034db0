"""
Early-reflection detection restated in NumPy from the docstring of audio_analysis_amd.analyse.reflections, in float64
(exactly the pinned order of every sum) or long double (the exact-side witness): helper module, it holds no tests and
shares no code with the module.

For a channel x (float32) of L samples with onset o, half window d (W = 2 d + 1), weights w (float64):
  h2[i] = x[i]^2 (0 outside [0, L));  e[n] = sum_k w[k] h2[n - d + k], from 0.0, k ascending, one rounding per multiply
  and per add;  row j = e[o + j], j < R = min(L - o, Rmax), Rmax = D + Tn + B (L for an unbounded Tn).
  n0 = first index of the maximum of e over [o, min(L, o + D));  Ed = e[n0].
  candidates n in [n0 + G, min(L, n0 + Tn + 1)):  e[n] > e[m] for m in [n - S, n);  e[n] >= e[m] for m in (n, min(n + S,
  L - 1)];  e[n] >= Ed rel;  e[n] cnt >= prom Bsum, Bsum the sequential sum (m ascending, from 0.0) of e[m] over
  [max(n - B, n0 + G), n - S) and then (n + S, min(n + B, L - 1)], cnt its number of terms.
  kept: the min(M, keep) candidates of largest e (the earlier index on equal e), in ascending time; per kept reflection
  n, e[n], Bsum, cnt, m = first index of max |x| over [max(n - d, 0), min(n + d, L - 1)], x[m].
  record: n0, Ed, M, kept, first candidate (-1), Edir = sum h2 over [max(n0 - Dw, 0), min(n0 + Dw, L - 1)], Erest = sum
  h2 over (n0 + Dw, L), the number of non-finite row entries.  L <= o: n0 = o, Ed = NaN, nothing else.

`margins` collects the relative margin |a - b| / max(|a|, |b|) of the comparisons taken -- every sample of the search range
against its greatest neighbour within S on either side (what decides rules 1 and 2; exact ties left out), rules 3 and 4 of the samples that reach them, and the
selection's cut -- so that a test can show the decisions lie far above float64 rounding.
"""
import math

import numpy as np

LD = np.longdouble
UNBOUNDED = 1 << 40


def count_of(ms, fs):
    return max(1, int(math.floor(ms * fs / 1000.0 + 0.5)))


def half_window(smooth_ms, fs):
    return max(1, int(math.floor(smooth_ms * fs / 2000.0 + 0.5)))


def tn_of(max_time_ms, fs):
    return UNBOUNDED if max_time_ms is None else int(math.ceil(max_time_ms * fs / 1000.0))


def weights(d, window):
    w = 2 * d + 1
    if window == "rect":
        return np.ones(w, dtype=np.float64)
    assert window == "hann"
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * (k + 1.0) / (w + 1.0)) for k in range(w)], dtype=np.float64)


def onset_index(x, onset_db=-20.0):
    """First n <= peak with x[n]^2 >= x[peak]^2 * 10^(onset_db / 10) (float64), 0 for an empty channel."""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return 0
    e = x * x
    p = int(np.argmax(np.abs(x)))
    return int(np.argmax(e[: p + 1] >= e[p] * 10.0 ** (onset_db / 10.0)))


def row_room(length, D, Tn, B):
    """Entries the host sizes a channel's row for: R of onset 0."""
    return min(length, length if Tn >= UNBOUNDED else D + Tn + B)


def envelope(x, d, window, dtype=np.float64):
    """e[n], n < L: a loop over k with e += w[k] * h2 shifted (zeros outside the channel take part: x + 0 == x)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = x.size
    w = weights(d, window).astype(dtype)
    h2 = np.zeros(n + 2 * d, dtype=dtype)
    h2[d : d + n] = x.astype(dtype) ** 2
    e = np.zeros(n, dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(2 * d + 1):
            e += w[k] * h2[k : k + n]
    return e


def energies(x, n0, Dw, dtype=LD):
    """(Edir, Erest, their numbers of terms): the sums of h2 over [max(n0 - Dw, 0), min(n0 + Dw, L - 1)] and (n0 + Dw, L)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    h2 = x.astype(dtype) ** 2
    a, b = max(n0 - Dw, 0), min(n0 + Dw, x.size - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        return h2[a : b + 1].sum(dtype=dtype), h2[b + 1 :].sum(dtype=dtype), (b + 1 - a, x.size - b - 1)


def _margin(margins, a, b):
    if margins is not None:
        a, b = float(a), float(b)
        m = max(abs(a), abs(b))
        if m > 0 and math.isfinite(m) and a != b:
            margins.append(abs(a - b) / m)


def detect(x, onset, d, window, D, Dw, G, S, B, Tn, rel, prom, keep, dtype=np.float64, margins=None):
    """dict(row, n0, Ed, M, kept (list of [n, e, Bsum, cnt, m, x[m]]), first, Edir, Erest, nonfinite, candidates (all M,
    in time order), terms (number of terms of Edir, Erest))."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    L, o = x.size, max(int(onset), 0)
    e = envelope(x, d, window, dtype)
    rmax = L if Tn >= UNBOUNDED else D + Tn + B
    R = max(0, min(L - o, rmax))
    row = e[o : o + R].copy()
    out = dict(row=row, n0=o, Ed=float("nan"), M=0, kept=[], first=-1, Edir=dtype(0.0), Erest=dtype(0.0),
               nonfinite=int(np.sum(~np.isfinite(row.astype(np.float64)))), candidates=[], terms=(0, 0))
    if R == 0:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        head = e[o : min(L, o + D)]
        n0 = o + int(np.argmax(np.where(np.isnan(head), -np.inf, head)))
        Ed = e[n0]
        edir, erest, terms = energies(x, n0, Dw, dtype)
        out.update(n0=n0, Ed=Ed, Edir=edir, Erest=erest, terms=terms)
        floor = Ed * dtype(rel)
        cands = []
        for n in range(n0 + G, min(L, n0 + Tn + 1)):
            v = e[n]
            before, after = e[n - S : n], e[n + 1 : min(n + S, L - 1) + 1]
            if margins is not None and np.isfinite(float(v)):
                for other in (before, after):                             # v against the greatest neighbour decides a rule
                    if other.size:
                        _margin(margins, v, other.max())
            if not np.all(v > before):
                continue
            if not np.all(v >= after):
                continue
            if not v >= floor:
                continue
            # the sequential sum, m ascending from 0.0: np.cumsum accumulates one term at a time, in order
            terms = np.concatenate([e[max(n - B, n0 + G) : max(n - S, 0)], e[n + S + 1 : min(n + B, L - 1) + 1]])
            cnt = int(terms.size)
            bsum = np.cumsum(terms, dtype=dtype)[-1] if cnt else dtype(0.0)
            ok = cnt == 0 or bsum == 0 or v * dtype(cnt) >= dtype(prom) * bsum
            if margins is not None:
                _margin(margins, v, floor)
                if cnt and bsum != 0:
                    _margin(margins, v * dtype(cnt), dtype(prom) * bsum)
            if ok:
                cands.append([n, v, bsum, cnt])
    order = sorted(range(len(cands)), key=lambda i: (-cands[i][1], cands[i][0]))
    if margins is not None and len(order) > keep:
        _margin(margins, cands[order[keep - 1]][1], cands[order[keep]][1])
    kept = sorted(order[:keep])
    rows = []
    for i in kept:
        n, v, bsum, cnt = cands[i]
        a, b = max(n - d, 0), min(n + d, L - 1)
        m = a + int(np.argmax(np.abs(x[a : b + 1])))
        rows.append([n, v, bsum, cnt, m, float(x[m])])
    out.update(M=len(cands), kept=rows, first=cands[0][0] if cands else -1, candidates=cands)
    return out


def decisions(res):
    """What a precision must agree on: n0, the candidate indices, the kept indices with their count and peak fields."""
    return (res["n0"], [c[0] for c in res["candidates"]], [(r[0], r[3], r[4], r[5]) for r in res["kept"]], res["first"],
            res["nonfinite"])


# ------------------------------------------------------------------------------------------------ seeded inputs
REFLECTIONS = ((3.1, 0.5), (7.4, -0.35), (12.0, 0.3), (19.7, 0.22), (41.3, -0.2))      # (ms after the direct pulse, gain)
DIRECT_AT = 200


def planted(fs=48000):
    """The sample indices of sparse_room's reflections."""
    return [DIRECT_AT + int(round(ms * fs / 1000.0)) for ms, _ in REFLECTIONS]


def sparse_room(n, seed, fs=48000):
    """200 samples of 1e-5 Gaussian pre-noise, a direct pulse of 1.0 at sample 200, five reflections, and a Gaussian tail
    0.02 * 10^(-3 t / 0.4) from 30 ms after the direct pulse on (t from there); float32."""
    rng = np.random.default_rng(seed)
    x = np.zeros(n, dtype=np.float64)
    x[:DIRECT_AT] = 1e-5 * rng.standard_normal(DIRECT_AT)
    x[DIRECT_AT] = 1.0
    for at, (_, gain) in zip(planted(fs), REFLECTIONS):
        if at < n:
            x[at] = gain
    t0 = DIRECT_AT + int(round(0.030 * fs))
    if n > t0:
        t = np.arange(n - t0) / float(fs)
        tail = 0.02 * 10.0 ** (-3.0 * t / 0.4) * rng.standard_normal(n - t0)
        keep = x[t0:] != 0.0
        x[t0:] = np.where(keep, x[t0:], tail)
    return x.astype(np.float32)


def twin_pulses(n=3000, first=100, second=1500, third=2200):
    """A direct pulse, then two identical isolated pulses in digital silence: their e is equal, a tie."""
    x = np.zeros(n, dtype=np.float32)
    x[first] = 1.0
    x[second] = x[third] = 0.5
    return x
