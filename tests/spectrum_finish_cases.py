"""
Inputs of the ira_spectrum_finish tests (tests/test_gpu_spectrum_finish.py), built from tests/spectrum_ref.py alone so that
tests/test_spectrum_finish_cpu.py can prove on a CPU what the GPU tests assume about them.  Helper module: it holds no tests.
"""
import functools

import numpy as np

import spectrum_ref as R

LD, F32 = R.LD, R.F32

# packed half lengths l at the tile edges of both streams (Z[k] forwards, Z[l - k] backwards) and of the k == l wrap
PACKED_EDGE_L = [4095, 4096, 4097, 8193]


def length_for_bins(nb):
    """A transform length with L // 2 + 1 == nb: even for even nb, odd for odd nb > 1 (both kinds of length occur)."""
    return 2 * (nb - 1) + (1 if nb > 1 and nb % 2 else 0)


@functools.lru_cache(maxsize=None)
def unit_spectra():
    """[(L, spectrum)]: every phase family of R.unwrap_cases() (steps, winding, mixed, caller; bin counts 1 .. 12289, on both
    sides of every multiple of the 4096-bin tile) imposed on a unit-magnitude spectrum."""
    out = []
    for _, p in R.unwrap_cases():
        L = length_for_bins(p.size)
        assert L // 2 + 1 == p.size
        out.append((L, np.cos(p) + 1j * np.sin(p)))
    return out


@functools.lru_cache(maxsize=None)
def unpacked_batch():
    """The ragged unpacked batch: R.mag_phase_batch() with its planted operands, then the unit-magnitude spectra."""
    return list(R.mag_phase_batch()) + unit_spectra()


@functools.lru_cache(maxsize=None)
def packed_batch():
    """[(L, values, packed, signal)]: R.mag_phase_packed_batch() and packed elements of the half lengths PACKED_EDGE_L, built
    the same way (real decaying noise)."""
    out = list(R.mag_phase_packed_batch())
    rng = np.random.default_rng(4242)
    for l in PACKED_EDGE_L:
        L = 2 * l
        x = rng.standard_normal(L) * np.exp(-np.arange(L) / (0.2 * L + 3.0))
        z = np.zeros(l + 1, dtype=np.complex128)
        z[:l] = R.pack_real(x)
        z[l] = complex(np.nan, np.nan)                         # never read by a packed element
        out.append((L, z, 1, x))
    return out


# One packed element past the 512 x 1024 bins the kernel's table of tile twiddles covers: the table is rebuilt once, at tile
# 128, and the last tile is partly filled
LONG_PACKED_L = 2 * (512 * 1024 + 1025)


@functools.lru_cache(maxsize=None)
def long_packed():
    """(L, values, signal) of the long packed element."""
    L = LONG_PACKED_L
    rng = np.random.default_rng(7)
    x = rng.standard_normal(L) * np.exp(-np.arange(L) / (0.2 * L + 3.0))
    z = np.zeros(L // 2 + 1, dtype=np.complex128)
    z[: L // 2] = R.pack_real(x)
    z[L // 2] = complex(np.nan, np.nan)
    return L, z, x


def winding_margin(ref):
    """For a packed element's reference (R.mag_db_phase(..., packed=True)): per pair of neighbouring bins, how far the
    reference's angle difference stays from +-pi beyond what the two angles may be off by (the packed branch's bound over
    |X| and the angle's own bound).  Positive everywhere: the reference alone decides every winding of the unwrap."""
    mag = np.hypot(ref["re"], ref["im"]).astype(np.float64)
    off = R.packed_bin_bound(ref["absz"]) / np.maximum(mag, 1e-300) + R.phase_bound(ref["re"], ref["im"], ref["lib_phase"])
    dd = np.abs(np.diff(ref["phase"])).astype(np.float64)
    return np.abs(np.pi - dd) - (off[1:] + off[:-1])


def stats_spectrum(mag_db):
    """A spectrum whose dB values (floor -inf: no floor) are the float32 array mag_db: real parts 10^(dB/20), NaN where the
    array has one.  The float64 dB of such a bin sits within 1e-13 of a float32 value, far from every rounding tie."""
    m = np.asarray(mag_db, dtype=F32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        re = 10.0 ** (m / 20.0)
    return re.astype(np.complex128)
