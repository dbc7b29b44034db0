"""
A long-double restatement of the ISO 3382-1 energy sums pinned in the docstring of audio_analysis_amd/analyse/energy.py
(ira_onset_index, ira_energy_windows in ira_energy.hip), written from the definitions and sharing no code with the module
or the kernels.  Helper module, like sti_ref.py / echo_ref.py: it holds no tests (tests/test_energy_ref_cpu.py holds it to a
per-sample loop, to closed forms and to hand-written onsets on a machine without a GPU).

A float32 squared is exact in float64 (24-bit significand -> 48 bits), so e = float64(x)^2 carries no rounding; the sums
are formed in long double (64-bit significand where the platform has one), which leaves the device's float64 sums ~2^-11
of their own rounding to be compared against.
"""
import math

import numpy as np

LD = np.longdouble


def onset(x, rel_energy):
    """The smallest n <= p with float64(x[n])^2 >= float64(x[p])^2 * rel_energy, p the first argmax |x|: float64 products and a
    float64 compare, exactly as the kernel states them."""
    x = np.asarray(x, dtype=np.float32)
    e = x.astype(np.float64) ** 2
    p = int(np.argmax(np.abs(x)))
    thr = e[p] * np.float64(rel_energy)
    return int(np.flatnonzero(e[: p + 1] >= thr)[0])


def edges(length, limits):
    """Partition j of a segment of `length` samples is [edges[j], edges[j + 1]): sample n belongs to partition
    #{k : N_k <= n} for the ascending limits N_k.  A limit past the end is the end, so the partitions behind it are empty;
    equal limits have an empty partition between them."""
    lim = [int(v) for v in limits]
    assert all(b >= a for a, b in zip(lim, lim[1:])) and (not lim or lim[0] >= 0), lim
    return [0] + [min(v, int(length)) for v in lim] + [int(length)]


def sums(y, onset, limits):
    """(P_0, .., P_K, S1) as long double over s = float64(y[onset:])^2: P_j = sum of s over partition j, S1 = sum n s[n] with
    n counted from the onset."""
    s = np.asarray(y, dtype=np.float32)[int(onset):].astype(np.float64) ** 2
    s = s.astype(LD)
    e = edges(s.size, limits)
    parts = [np.sum(s[a:b], dtype=LD) if b > a else LD(0) for a, b in zip(e[:-1], e[1:])]
    s1 = np.sum(np.arange(s.size, dtype=LD) * s, dtype=LD)
    return np.array(parts + [s1], dtype=LD)


def params(sums, fs, d_index=0):
    """(C_1 .. C_K in dB, D, Ts in seconds) from sums' P_0 .. P_K, S1: C_k = 10 log10(early / late) with early = P_0 + .. +
    P_{k-1}, +inf when the late sum is 0 and the early sum is not; D = (P_0 + .. + P_{d_index}) / total; Ts = S1 / (fs total)."""
    v = np.asarray(sums, dtype=LD)
    p, s1 = v[:-1], v[-1]
    total = np.sum(p, dtype=LD)
    c = []
    for i in range(1, p.size):
        early, late = np.sum(p[:i], dtype=LD), np.sum(p[i:], dtype=LD)
        if late == 0:
            c.append(math.inf if early > 0 else math.nan)
        else:
            c.append(float(LD(10) * np.log10(early / late)))
    return c, float(np.sum(p[: d_index + 1], dtype=LD) / total), float(s1 / (LD(fs) * total))
