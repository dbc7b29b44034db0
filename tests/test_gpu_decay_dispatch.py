"""Every entry point of ira_edc.hip (ira_peak_index, ira_edc_db, ira_edc_box_smooth, ira_curve_fits, ira_edc_fits) called
through the C-ABI against the long-double / oracle reference of tests/decay_ref.py.

Every input and output buffer of a launch is allocated here with 0xDEADBEEF-filled gaps of 1 to 7 elements between the
segments (offsets take every residue mod 4) and guard zones around the flat record arrays; every gap of every output
must come back untouched, and a read past a segment's end meets -6.3e18 instead of a neighbour's plausible sample.  One
ragged batch per launch: lengths around the 16-sample thread slice, the 4096-sample tile, the 16384-sample chunk and
the 32768-sample pre-search threshold, up to the documented maximum of 2047 tiles; decays from RT60 0.02 s to 200 s with
and without leading silence, silence, DC, single impulses, noise, rescaled IRs (the eps clamp on part and on all of the
curve), subnormal samples, exact-zero tails with eps = 0, NaN and infinite samples, -0.0, ties of |x|.

The bounds are those of decay_ref (A: curve against long double, B: records against the oracle on the curve the GPU
worked on, C: records against the oracle's float64 path on the samples); none of them comes from what the kernels
return.  test_zz_report prints the measured figures.  Measured on an MI355X: A: float64 curve within 0.23 of the
allowance (1.2e-13 dB), every float32 sample of every ira_edc_db and ira_edc_fits launch bit-identical to the long-double
reference, 99.909 % with tile partials (the rest within 1e-4 of the allowance); B: times 0 ulps, slope and
rt60 1.7e-12, intercept 3.0e-13, r2 2.3e-14; C: slope and rt60 1.8e-15, r2 6.7e-16, times and npts equal on all 64 records.

What these tests found (fixed with them): ira_peak_index let a later NaN with a larger payload beat the first NaN
("two_nans": index 20000 instead of 100); ira_edc_fits reported a valid fit with slope -8.2e-15 dB/s (RT60 7.3e15 s) on
a mask whose values are all equal ("lead32763/ir32768", range (0, -10)), where the reference and ira_curve_fits get
slope 0 and refuse it.
"""
import ctypes as C

import numpy as np
import pytest

import decay_ref as R

pytestmark = pytest.mark.gpu
SR = 48000
SENT32 = 0xDEADBEEF
SENT64 = 0xDEADBEEFDEADBEEF
GUARD = 16
IRA_E_NULL, IRA_E_SIZE, IRA_E_UNSUPPORTED = -1, -2, -3
SCRATCH = 4096                                # IRA_EDC_SCRATCH_DOUBLES
STATS = {}                                    # entry point -> measured figures, printed by test_zz_report


@pytest.fixture(scope="module")
def eng():
    R.need_longdouble()
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def _note(entry, **kv):
    """Fold figures into STATS[entry]: 'min_*' keys keep the minimum, every other key the maximum."""
    st = STATS.setdefault(entry, {})
    for k, v in kv.items():
        st[k] = min(st.get(k, v), v) if k.startswith("min_") else max(st.get(k, v), v)


# ----------------------------------------------------------------------------------------------------------- buffers
def _sentinel(n, dtype):
    dtype = np.dtype(dtype)
    if dtype.itemsize == 4:
        return np.full(n, SENT32, np.uint32).view(dtype)
    return np.full(n, SENT64, np.uint64).view(dtype)


def _is_sentinel(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) == SENT32 if a.dtype.itemsize == 4 else a.view(np.uint64) == SENT64


class Layout:
    """Segments of `lens` elements in one flat buffer, gaps of 1 .. 7 elements before, between and behind them."""

    def __init__(self, lens, phase=0):
        self.lens = np.asarray(lens, np.int64).reshape(-1)
        off, pos = [], 1 + phase % 7
        for k, n in enumerate(self.lens):
            off.append(pos)
            pos += int(n) + 1 + (k + phase + 1) % 7
        self.off = np.array(off, np.int64).reshape(-1)
        self.total = pos
        if self.lens.size >= 12:
            assert set(int(o) % 4 for o in self.off) == {0, 1, 2, 3}

    def filled(self, segs, dtype):
        buf = _sentinel(self.total, dtype)
        for o, s in zip(self.off, segs):
            buf[o:o + len(s)] = np.asarray(s, dtype)
        return buf

    def split(self, buf, what):
        """The segments of a buffer that came back; every gap must still hold the sentinel."""
        gaps = np.ones(self.total, bool)
        for o, n in zip(self.off, self.lens):
            gaps[o:o + n] = False
        bad = gaps & ~_is_sentinel(buf)
        assert not bad.any(), f"{what}: {int(bad.sum())} elements written outside the segments, first at {int(np.argmax(bad))}"
        return [buf[o:o + n].copy() for o, n in zip(self.off, self.lens)]


class Dev:
    """Device buffers of one launch (kept referenced until the results are back)."""

    def __init__(self, eng):
        import torch
        self.eng, self.torch, self.keep = eng, torch, []

    def put(self, arr):
        t = self.torch.from_numpy(np.ascontiguousarray(arr)).to(self.eng.device)
        self.keep.append(t)
        return t

    def gapped(self, layout, dtype, segs=None):
        buf = layout.filled(segs, dtype) if segs is not None else _sentinel(layout.total, dtype)
        return self.put(buf)

    def flat(self, n, dtype):
        """n elements between two guard zones: (tensor, pointer to the first of the n)."""
        t = self.put(_sentinel(n + 2 * GUARD, dtype))
        return t, t.data_ptr() + GUARD * np.dtype(dtype).itemsize

    def back_flat(self, t, n, dtype, what):
        a = t.cpu().numpy().view(dtype)
        assert _is_sentinel(a[:GUARD]).all() and _is_sentinel(a[GUARD + n:]).all(), f"{what}: guard zone written"
        return a[GUARD:GUARD + n].copy()


def _dbl(values):
    return (C.c_double * max(1, len(values)))(*[float(v) for v in values])


# ------------------------------------------------------------------------------------------------------ entry points
def peak_index(eng, segs, phase=0, max_len=None, want_abs=True):
    d = Dev(eng)
    lay = Layout([len(s) for s in segs], phase)
    x = d.gapped(lay, np.float32, segs)
    off, ln = d.put(lay.off), d.put(lay.lens)
    n = len(segs)
    pk, pk_ptr = d.flat(n, np.int64)
    pa, pa_ptr = d.flat(n, np.float32)
    ml = int(lay.lens.max()) if max_len is None else max_len
    rc = eng.lib.ira_peak_index(x.data_ptr(), off.data_ptr(), ln.data_ptr(), n, ml, pk_ptr, pa_ptr if want_abs else None,
                                eng.stream)
    eng.sync()
    assert rc == 0, rc
    assert _is_sentinel(x.cpu().numpy())[~_segment_mask(lay)].all()
    return d.back_flat(pk, n, np.int64, "peak_dev"), d.back_flat(pa, n, np.float32, "peak_abs_dev")


def _segment_mask(lay):
    m = np.zeros(lay.total, bool)
    for o, n in zip(lay.off, lay.lens):
        m[o:o + n] = True
    return m


def edc_db(eng, segs, eps, floor_db, want32=True, want64=False, phase=0):
    """ira_edc_db on a gapped batch: (float32 curves | None, float64 curves | None)."""
    d = Dev(eng)
    lay = Layout([len(s) for s in segs], phase)
    out_lay = Layout(lay.lens, phase + 3)                     # the curves sit at other offsets than the samples
    x = d.gapped(lay, np.float32, segs)
    off, ln, eoff = d.put(lay.off), d.put(lay.lens), d.put(out_lay.off)
    n = len(segs)
    o32 = d.gapped(out_lay, np.float32) if want32 else None
    o64 = d.gapped(out_lay, np.float64) if want64 else None
    sc, sc_ptr = d.flat(n * SCRATCH, np.float64)
    rc = eng.lib.ira_edc_db(x.data_ptr(), off.data_ptr(), ln.data_ptr(), n, int(lay.lens.max()), float(eps),
                            float(floor_db), o32.data_ptr() if want32 else None, o64.data_ptr() if want64 else None,
                            eoff.data_ptr(), sc_ptr, eng.stream)
    eng.sync()
    assert rc == 0, rc
    d.back_flat(sc, n * SCRATCH, np.float64, "scratch")
    return (out_lay.split(o32.cpu().numpy(), "edc_db_dev") if want32 else None,
            out_lay.split(o64.cpu().numpy(), "edc_db64_dev") if want64 else None)


def box_smooth(eng, curves64, window, floor_db, phase=0, max_len=None, expect=0):
    d = Dev(eng)
    lay = Layout([len(c) for c in curves64], phase)
    a = d.gapped(lay, np.float64, curves64)
    off, ln = d.put(lay.off), d.put(lay.lens)
    out = d.gapped(lay, np.float32)
    ml = int(lay.lens.max()) if max_len is None else max_len
    rc = eng.lib.ira_edc_box_smooth(a.data_ptr(), off.data_ptr(), ln.data_ptr(), len(curves64), ml, int(window),
                                    float(floor_db), out.data_ptr(), eng.stream)
    eng.sync()
    assert rc == expect, rc
    got = out.cpu().numpy()
    if expect != 0:
        assert _is_sentinel(got).all(), "a refused call wrote to its output"
        return None
    return lay.split(got, "box smooth out_dev")


def curve_fits(eng, curves, ranges, cross, min_points, t_mul=1.0, t_div=float(SR), t_axis=None, rel=None, phase=0,
               max_len=None):
    """ira_curve_fits on a gapped batch of float32 curves: (records (n, nranges, 8), crossings (n, ncross))."""
    d = Dev(eng)
    lay = Layout([len(c) for c in curves], phase)
    y = d.gapped(lay, np.float32, curves)
    off, ln = d.put(lay.off), d.put(lay.lens)
    n, nr, nc = len(curves), len(ranges), len(cross)
    fit, fit_ptr = d.flat(n * nr * 8, np.float64)
    cr, cr_ptr = d.flat(n * nc, np.float64)
    ta = d.put(np.asarray(t_axis, np.float32)) if t_axis is not None else None
    ml = int(lay.lens.max()) if max_len is None else max_len
    floor_db, min_peak = rel if rel is not None else (-120.0, 0.0)
    rc = eng.lib.ira_curve_fits(y.data_ptr(), off.data_ptr(), ln.data_ptr(), n, ml, float(t_mul), float(t_div),
                                ta.data_ptr() if ta is not None else None, _dbl([v for r in ranges for v in r]), nr,
                                int(min_points), _dbl(cross), nc, 1 if rel is not None else 0, float(floor_db),
                                float(min_peak), fit_ptr if nr else None, cr_ptr if nc else None, eng.stream)
    eng.sync()
    assert rc == 0, rc
    return (d.back_flat(fit, n * nr * 8, np.float64, "fit_out_dev").reshape(n, nr, 8),
            d.back_flat(cr, n * nc, np.float64, "cross_out_dev").reshape(n, nc))


def edc_fits(eng, segs, eps, floor_db, ranges, cross, min_points, want_edc=True, phase=0, parts=None, t_mul=1.0,
             t_div=float(SR)):
    """ira_edc_fits on a gapped batch: (records, crossings, float32 curves | None).  parts = (flat float64 array,
    part_off int64, part_wgs int32, part_tiles int32)."""
    d = Dev(eng)
    lay = Layout([len(s) for s in segs], phase)
    out_lay = Layout(lay.lens, phase + 5)
    x = d.gapped(lay, np.float32, segs)
    off, ln, eoff = d.put(lay.off), d.put(lay.lens), d.put(out_lay.off)
    n, nr, nc = len(segs), len(ranges), len(cross)
    fit, fit_ptr = d.flat(n * nr * 8, np.float64)
    cr, cr_ptr = d.flat(n * nc, np.float64)
    o32 = d.gapped(out_lay, np.float32) if want_edc else None
    sc, sc_ptr = d.flat(n * SCRATCH, np.float64)
    p = [d.put(a) for a in parts] if parts is not None else [None] * 4
    rc = eng.lib.ira_edc_fits(x.data_ptr(), off.data_ptr(), ln.data_ptr(), n, int(lay.lens.max()), float(eps),
                              float(floor_db), float(t_mul), float(t_div), _dbl([v for r in ranges for v in r]), nr,
                              int(min_points), _dbl(cross), nc, fit_ptr if nr else None, cr_ptr if nc else None,
                              o32.data_ptr() if want_edc else None, eoff.data_ptr() if want_edc else None, sc_ptr,
                              *[t.data_ptr() if t is not None else None for t in p], eng.stream)
    eng.sync()
    assert rc == 0, rc
    d.back_flat(sc, n * SCRATCH, np.float64, "scratch")
    return (d.back_flat(fit, n * nr * 8, np.float64, "fit_out_dev").reshape(n, nr, 8),
            d.back_flat(cr, n * nc, np.float64, "cross_out_dev").reshape(n, nc),
            out_lay.split(o32.cpu().numpy(), "edc_db_dev") if want_edc else None)


# ------------------------------------------------------------------------------------------------------------ inputs
_NAN_A = np.array([0x7fc00001], np.uint32).view(np.float32)[0]       # a quiet NaN with a small payload
_NAN_B = np.array([0xffffffff], np.uint32).view(np.float32)[0]       # a negative one with the largest payload


def _special(kind, n, seed):
    rng = np.random.default_rng(1000 + seed)
    if kind == "zero":
        return np.zeros(n, np.float32)
    if kind == "negzero":
        return np.full(n, -0.0, np.float32)
    if kind == "dc":
        return np.full(n, 0.25, np.float32)
    if kind == "last":
        x = np.zeros(n, np.float32); x[-1] = 1.0
        return x
    if kind == "first":
        x = np.zeros(n, np.float32); x[0] = -1.0
        return x
    if kind == "noise":
        return (0.3 * rng.standard_normal(n)).astype(np.float32)
    x = R.ir(500 + seed, n, 0.25 * n / SR + 0.01)                     # about -240 dB over the segment
    if kind == "tiny":                                                # every suffix sum below eps = 1e-20
        return (x.astype(np.float64) * 1e-18).astype(np.float32)
    if kind == "small":                                               # the tail of the curve below eps = 1e-20
        return (x.astype(np.float64) * 1e-7).astype(np.float32)
    if kind == "huge":
        return (x.astype(np.float64) * 1e18).astype(np.float32)
    if kind == "subnormal":
        return (x.astype(np.float64) * 3e-39).astype(np.float32)
    if kind == "zerotail":
        x[n - n // 3:] = 0.0
        return x
    if kind == "ir_negzero":
        x[::3] = -0.0
        return x
    pos = {"nan_first": min(1, n - 1), "nan_mid": n // 2, "nan_lasttile": max(n - 100, n // 2 + 1) if n > 8 else n - 2,
           "nan_last": n - 1, "pinf": n // 3, "ninf": n // 2}[kind]
    x[pos] = {"pinf": np.inf, "ninf": -np.inf}.get(kind, np.nan)
    return x


SPECIAL_KINDS = ("zero", "negzero", "dc", "last", "first", "noise", "tiny", "small", "huge", "ir_negzero", "nan_first",
                 "nan_mid", "nan_lasttile", "nan_last", "pinf", "ninf")
SPECIAL_LENGTHS = (4, 17, 257, 4097, 8192, 16385, 32769)
_MAIN = []


def main_batch():
    """(name, samples) of the batch ira_edc_db and ira_edc_fits share: every length of the issue as a decay whose RT60
    cycles from 0.02 s (all crossings in the first tile in time) to 200 s (no level but 0 dB is reached), the shorter
    ones again behind leading silence, and every special signal at lengths around the tile and chunk edges."""
    if _MAIN:
        return _MAIN
    rts = (0.02, 0.3, 2.0, 200.0, 0.08, 1.0)
    for k, n in enumerate(R.SEGMENT_LENGTHS):
        rt = rts[k % len(rts)]
        _MAIN.append((f"ir{n}/rt{rt}", R.ir(100 + k, n, rt)))
        if 16 <= n <= 3 * 16384 + 5:
            lead = (3, n // 2, 4096, n - 5, 4097)[k % 5]
            lead = min(lead, n - 4)
            _MAIN.append((f"lead{lead}/ir{n}", R.ir(200 + k, n, rts[(k + 2) % len(rts)] if n > 4097 else 0.02, lead=lead)))
    _MAIN.append(("ir480000/last-tile", R.ir(290, 480000, 9.0)))      # -35 dB about 5.2 s in; -65 dB never
    _MAIN.append(("ir250001/end", R.ir(291, 250001, 5.1)))            # -60 dB inside the last tiles
    for j, kind in enumerate(SPECIAL_KINDS):
        for i, n in enumerate(SPECIAL_LENGTHS):
            if (i + j) % 2 == 0 or n in (4097, 16385):
                _MAIN.append((f"{kind}{n}", _special(kind, n, 10 * j + i)))
    return _MAIN


_REF = {}


def _edc_ref(name, x, eps):
    key = (name, eps)
    if key not in _REF:
        _REF[key] = R.edc_reference(x, eps)
    return _REF[key]


def _check_curves(entry, batch, eps, floor_db, got32=None, got64=None):
    """Comparison A over one launch; returns the share of bit-identical float32 samples."""
    same = total = 0
    for i, (name, x) in enumerate(batch):
        try:
            st = R.compare_edc(x, eps, floor_db, got64=None if got64 is None else got64[i],
                               got32=None if got32 is None else got32[i], ref=_edc_ref(name, x, eps))
        except AssertionError as e:
            raise AssertionError(f"{entry} eps {eps} floor {floor_db}: segment {i} ({name}): {e}") from None
        same, total = same + st["same32"], total + st["n32"]
        _note(entry, A_f64_of_bound=st["worst64"], A_f32_of_bound=st["worst32"], A_f64_dB=st["dev64"], A_f32_dB=st["dev32"])
        finite = bool(np.all(np.isfinite(x)))
        if finite and (eps > 0.0 or np.any(x != 0)):
            if got32 is not None:
                assert got32[i][0] == 0.0, (entry, name, got32[i][0])
            if got64 is not None:
                assert got64[i][0] == 0.0, (entry, name, got64[i][0])
    if total:
        _note(entry, min_share_bit_identical=same / total)
        print(f"{entry} eps {eps} floor {floor_db}: {same} of {total} float32 samples bit-identical ({same / total:.6f})")
    return same / total if total else None


_RECS = {}


def _records(key, y, ranges, cross, min_points, **kw):
    """Cached decay_ref.curve_records, range by range (launches share curves and ranges)."""
    recs = []
    for r in ranges:
        k = ("r", key, r, min_points, tuple(sorted((a, str(b)) for a, b in kw.items() if a != "t")), id(kw.get("t")))
        if k not in _RECS:
            _RECS[k] = R.curve_records(y, [r], (), min_points, **kw)[0][0]
        recs.append(_RECS[k])
    return np.array(recs).reshape(len(ranges), 8), R.curve_records(y, [], cross, min_points, **kw)[1]


def _check_records_b(entry, names, curves, fit, cr, ranges, cross, min_points, **kw):
    st = {}
    for i, (name, y) in enumerate(zip(names, curves)):
        ref, cref = _records(name, y, ranges, cross, min_points, **kw)
        try:
            R.compare_records(fit[i], ref, st)
            st["cross_ulps"] = max(st.get("cross_ulps", 0.0), R.compare_times(cr[i], cref))
        except AssertionError as e:
            raise AssertionError(f"{entry}: curve {i} ({name}), ranges {ranges}, cross {cross}: {e}") from None
    _note(entry, **{f"B_{k}": v for k, v in st.items()})


# ------------------------------------------------------------------------------------------------------ ira_peak_index
def _tie_segments():
    """|x| ties whose first member must win: across the chunk edge (16383 | 16384), across the scalar head / float4 body
    split of the first and of a later chunk (the head is 0 .. 3 samples long, whatever the offset), and across the
    body / tail split at the end."""
    out = []
    n = 40003
    for a in (0, 1, 2, 3, 16382, 16383, 16384, 16385, 16386, 32767, n - 5, n - 4, n - 3, n - 2):
        x = np.zeros(n, np.float32)
        x[a], x[a + 1] = -0.5, 0.5
        x[(a + 7777) % n] = 0.25
        out.append((f"tie{a}", x))
    return out


def _peak_batch():
    b = list(main_batch())
    for rep in range(7):                                              # the tie set at every phase of the gap cycle
        b += [(f"{nm}/{rep}", x) for nm, x in _tie_segments()] + [(f"pad{rep}", np.zeros(4 + rep, np.float32))]
    two = R.ir(77, 40000, 0.3)
    two[100], two[20000] = _NAN_A, _NAN_B                             # the later NaN has the larger payload
    b.append(("two_nans", two))
    two = R.ir(78, 5000, 0.3)
    two[4000], two[4001] = _NAN_B, _NAN_A
    b.append(("two_nans_adjacent", two))
    inf = R.ir(79, 40000, 0.3)
    inf[30000], inf[35000] = -np.inf, np.inf
    b.append(("two_infs", inf))
    infnan = inf.copy(); infnan[39999] = np.nan
    b.append(("inf_then_nan", infnan))
    return b


def test_peak_index_batch(eng):
    b = _peak_batch()
    assert len(b) > 200
    for phase in (0, 2):
        idx, pa = peak_index(eng, [x for _, x in b], phase=phase)
        bad = []
        for i, (name, x) in enumerate(b):
            try:
                R.compare_peak(x, idx[i], pa[i])
            except AssertionError as e:
                bad.append((name, str(e)))
        assert not bad, bad
    _note("ira_peak_index", segments=len(b))


def test_peak_index_single_segments_and_empty_calls(eng):
    b = dict(_peak_batch())
    for name in ("ir480000/last-tile", "tie16383/0", "two_nans", "nan_last4097", "negzero4097", "ir4/rt0.02", "pinf16385"):
        for phase in (0, 1, 2, 3):
            idx, pa = peak_index(eng, [b[name]], phase=phase)
            R.compare_peak(b[name], idx[0], pa[0])
    idx, _ = peak_index(eng, [b["tie16383/0"]], want_abs=False)        # peak_abs_dev is optional
    assert idx[0] == 16383
    # nseg = 0: accepted, nothing written; max_len = 0: accepted, index 0
    d = Dev(eng)
    pk, pk_ptr = d.flat(4, np.int64)
    x = d.put(np.zeros(8, np.float32)); off = d.put(np.zeros(1, np.int64)); ln = d.put(np.zeros(1, np.int64))
    assert eng.lib.ira_peak_index(x.data_ptr(), off.data_ptr(), ln.data_ptr(), 0, 100, pk_ptr, None, eng.stream) == 0
    eng.sync()
    assert _is_sentinel(pk.cpu().numpy()).all()
    pa, pa_ptr = d.flat(1, np.float32)
    assert eng.lib.ira_peak_index(x.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, 0, pk_ptr, pa_ptr, eng.stream) == 0
    eng.sync()
    got = pk.cpu().numpy()
    assert got[GUARD] == 0 and _is_sentinel(got[GUARD + 1:]).all() and _is_sentinel(got[:GUARD]).all()
    assert eng.lib.ira_peak_index(None, off.data_ptr(), ln.data_ptr(), 1, 8, pk_ptr, None, eng.stream) == IRA_E_NULL
    assert eng.lib.ira_peak_index(x.data_ptr(), off.data_ptr(), ln.data_ptr(), -1, 8, pk_ptr, None, eng.stream) == IRA_E_SIZE
    assert eng.lib.ira_peak_index(x.data_ptr(), off.data_ptr(), ln.data_ptr(), 65536, 8, pk_ptr, None, eng.stream) == IRA_E_SIZE


# ---------------------------------------------------------------------------------------------------------- ira_edc_db
def test_edc_db_both_outputs(eng):
    b = main_batch()
    g32, g64 = edc_db(eng, [x for _, x in b], 1e-20, -120.0, True, True)
    _check_curves("ira_edc_db", b, 1e-20, -120.0, g32, g64)


def test_edc_db_float32_only_floor_60(eng):
    b = main_batch()
    g32, none = edc_db(eng, [x for _, x in b], 1e-20, -60.0, True, False, phase=1)
    assert none is None
    _check_curves("ira_edc_db", b, 1e-20, -60.0, g32)
    assert any(np.any(g == np.float32(-60.0)) and np.any(g > np.float32(-60.0)) for g in g32)


def _low_level_batch():
    b = [(nm, x) for nm, x in main_batch() if len(x) <= 32769 and not nm.startswith("lead")]
    for i, n in enumerate((17, 4097, 16385, 32769)):
        b.append((f"subnormal{n}", _special("subnormal", n, 300 + i)))
        b.append((f"zerotail{n}", _special("zerotail", n, 310 + i)))
    assert np.any(np.abs(b[-2][1]) < np.finfo(np.float32).tiny)
    return b


def test_edc_db_float64_only_eps_1e90(eng):
    b = _low_level_batch()
    none, g64 = edc_db(eng, [x for _, x in b], 1e-90, -300.0, False, True, phase=2)
    assert none is None
    _check_curves("ira_edc_db", b, 1e-90, -300.0, None, g64)


def test_edc_db_eps_zero(eng):
    """eps = 0: a tail of exact zeros is -inf in the float64 curve (the kernel leaves its table logarithm for log10) and
    the floor in the float32 curve; digital silence is 0 / 0 = NaN everywhere, as in the reference."""
    b = _low_level_batch()
    g32, g64 = edc_db(eng, [x for _, x in b], 0.0, -300.0, True, True, phase=3)
    _check_curves("ira_edc_db", b, 0.0, -300.0, g32, g64)
    names = [nm for nm, _ in b]
    z = g64[names.index("zerotail4097")]
    assert np.isneginf(z[-1]) and np.isfinite(z[0])
    assert np.all(np.isnan(g32[names.index("zero4097")]))


def test_edc_db_longest_segment_and_refusals(eng):
    x = R.end_to_end_inputs()[-1][1]
    assert x.size == R.MAX_SEGMENT == 2047 * 4096
    b = [("irmax", x)]
    g32, g64 = edc_db(eng, [x], 1e-20, -120.0, True, True, phase=1)
    _check_curves("ira_edc_db", b, 1e-20, -120.0, g32, g64)
    # one sample more: refused before anything is launched (the arguments are not looked at further)
    d = Dev(eng)
    small = d.put(np.zeros(64, np.float32)); off = d.put(np.zeros(1, np.int64)); ln = d.put(np.full(1, 8, np.int64))
    out, out_ptr = d.flat(8, np.float32)
    sc, sc_ptr = d.flat(SCRATCH, np.float64)
    args = lambda nseg, max_len, o32=out_ptr: (small.data_ptr(), off.data_ptr(), ln.data_ptr(), nseg, max_len, 1e-20,
                                               -120.0, o32, None, off.data_ptr(), sc_ptr, eng.stream)
    assert eng.lib.ira_edc_db(*args(1, R.MAX_SEGMENT + 1)) == IRA_E_SIZE
    assert eng.lib.ira_edc_db(*args(1, 0)) == IRA_E_SIZE
    assert eng.lib.ira_edc_db(*args(0, 8)) == 0
    assert eng.lib.ira_edc_db(*args(1, 8, None)) == IRA_E_NULL
    fit, fit_ptr = d.flat(8, np.float64)
    rc = eng.lib.ira_edc_fits(small.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, R.MAX_SEGMENT + 1, 1e-20, -120.0, 1.0,
                              float(SR), _dbl([-5.0, -25.0]), 1, 8, _dbl([]), 0, fit_ptr, None, None, None, sc_ptr, None,
                              None, None, None, eng.stream)
    assert rc == IRA_E_SIZE
    eng.sync()
    d.back_flat(out, 8, np.float32, "edc_db_dev")
    d.back_flat(sc, SCRATCH, np.float64, "scratch")
    d.back_flat(fit, 8, np.float64, "fit_out_dev")


# -------------------------------------------------------------------------------------------------- ira_edc_box_smooth
def _smooth_inputs(lens):
    out = []
    for k, n in enumerate(lens):
        rng = np.random.default_rng(600 + k)                          # about -170 dB at the end: below both floors
        x = (rng.standard_normal(n) * 10.0 ** (-8.5 * np.arange(n) / n)).astype(np.float32)
        out.append(R.edc_curve(x, 1e-90, -300.0)[0])
    return out


@pytest.mark.parametrize("window,lens", [(1, (4, 5, 17, 257, 4097)), (2, (4, 5, 17, 257, 4097, 16385)),
                                         (3, (4, 5, 17, 257, 4097)), (4, (4, 5, 17, 257)), (8, (8, 15, 257, 4097, 16385)),
                                         (255, (255, 256, 4097, 16385)), (4801, (4801, 8193, 32769))])
def test_box_smooth(eng, window, lens):
    """Windows 1, 2, 3, 8, 255, 4801 and window == the shortest segment of the batch (4, 8, 255, 4801), on float64 curves
    made on the host; the floor (-60 dB, then -120 dB) is reached inside every smoothed curve but the shortest."""
    curves = _smooth_inputs(lens)
    for floor_db, phase in ((-60.0, 0), (-120.0, 3)):
        got = box_smooth(eng, curves, window, floor_db, phase=phase)
        floored = 0
        for a, g in zip(curves, got):
            _note("ira_edc_box_smooth", of_bound=R.compare_smooth(a, window, floor_db, g))
            floored += int(np.any(g == np.float32(floor_db)) and np.any(g > np.float32(floor_db)))
        assert 2 * floored >= len(lens)


def test_box_smooth_refusal_contract(eng):
    """Finding 2: the function sees max_len only.  window > max_len is refused (IRA_E_UNSUPPORTED, nothing written); a
    window longer than SOME segment of a ragged batch is not: that segment's sums are clipped to it (in bounds), and it
    is the Python layer that refuses such a request, as numpy's "same" would return `window` values there."""
    curves = _smooth_inputs((300, 5, 64))
    assert box_smooth(eng, curves, 301, -120.0, expect=IRA_E_UNSUPPORTED) is None
    assert box_smooth(eng, curves, 8, -120.0, max_len=7, expect=IRA_E_UNSUPPORTED) is None
    assert box_smooth(eng, curves, 0, -120.0, expect=IRA_E_SIZE) is None
    got = box_smooth(eng, curves, 8, -120.0)                          # 5 < 8 <= 300: runs
    R.compare_smooth(curves[0], 8, -120.0, got[0])
    R.compare_smooth(curves[2], 8, -120.0, got[2])
    a, h = curves[1].astype(R.LD), (8 - 1) // 2
    for i in range(5):                                                # window i + h - 7 .. i + h, clipped to 0 .. 4
        clipped = np.float32(np.sum(a[max(0, i + h - 7):min(5, i + h + 1)] * R.LD(1.0 / 8.0)))
        assert abs(got[1][i] - clipped) <= np.spacing(abs(clipped)), (i, got[1], clipped)
    from audio_analysis_amd.analyse import decay
    x = R.ir(7, 400, 0.02)
    with pytest.raises(ValueError):
        decay.analyse_decay_for_channel(x, SR, "m", decay.DecayAnalysisSettings(edc_smoothing_window_samples=401))
    r = decay.analyse_decay_for_channel(x, SR, "m", decay.DecayAnalysisSettings(edc_smoothing_window_samples=400))
    assert r.edc_db.size == 400


# ------------------------------------------------------------------------------------------------------ ira_curve_fits
RANGE_POOL = ((-5.0, -25.0), (-5.0, -35.0), (0.0, -10.0), (-40.0, -60.0))
CROSS_POOL = (0.0, -10.0, -5.0, -33.3)
_CURVES = {}


def _line(n, db_per_sample):
    return (-(np.arange(n, dtype=np.float64) * db_per_sample)).astype(np.float32)


def host_curves(max_n):
    """(name, float32 curve), none longer than max_n and one of exactly max_n samples: reference EDCs of decays, exact
    lines (slope -db_per_sample * sr in closed form), staircases with long equal runs, a curve that rises again after its
    crossings, one that touches every target exactly, curves with a NaN next to a crossing, +Inf in front and -Inf at
    the end.  No NaN sits inside a fit mask: what the reference returns there is whatever LAPACK makes of a NaN (NaN
    coefficients that pass its `slope >= 0` refusal, or an exception), not a contract."""
    if max_n in _CURVES:
        return _CURVES[max_n]
    out = []
    for k, n in enumerate([max_n, max(4, max_n // 3), 257, 17, 5, 4]):
        n = min(n, max_n)
        out.append((f"edc{n}", R.edc_curve(R.ir(700 + k, n, max(0.01, 0.12 * n / SR)), 1e-20, -120.0)[1]))
    out.append((f"edc_slow{max_n}", R.edc_curve(R.ir(710, max_n, 30.0), 1e-20, -120.0)[1]))      # nothing below -1 dB
    n = min(max_n, 2000)
    out.append(("line", _line(n, 0.0625)))                           # exact in float32: -3000 dB/s at 48 kHz
    out.append(("line_long", _line(max_n, 70.0 / max_n)))
    out.append(("touch", _line(n, 0.25)))                            # holds 0, -5, -10, -25, -35, -40, -60 exactly
    i = np.arange(max_n)
    out.append(("stairs", (-0.5 * (i // max(1, max_n // 150))).astype(np.float32)))
    out.append(("stairs_short", (-7.5 * (np.arange(64) // 9)).astype(np.float32)))
    m = max(8, min(max_n, 3000))
    j = np.arange(m, dtype=np.float64)
    rise = np.where(j < m / 4, -160.0 * j / m, np.where(j < m / 2, -40.0 + 148.0 * (j - m / 4) / m, -3.0 - 160.0 * (j - m / 2) / m))
    out.append(("rise_again", rise.astype(np.float32)))
    y = (_line(n, 0.03) + np.float32(3.0)).astype(np.float32)
    y[int(np.argmax(y <= np.float32(0.0))) - 1] = np.nan             # the sample before the 0 dB crossing, in no mask
    out.append(("nan_neighbour", y))
    y = _line(n, 0.03).copy(); y[0] = np.nan
    out.append(("nan_first", y))
    y = _line(n, 0.03).copy(); y[0] = np.inf
    out.append(("pinf_first", y))
    y = _line(n, 0.02).copy(); y[-1] = -np.inf                       # ends at -40 dB: -inf is the -60 dB crossing
    out.append(("ninf_last", y))
    out.append(("flat", np.zeros(300, np.float32)))
    assert max(len(c) for _, c in out) == max_n
    _CURVES[max_n] = out
    return out


@pytest.mark.parametrize("nranges", [0, 1, 2, 3, 4])
def test_curve_fits_every_record_shape(eng, nranges):
    """Every (nranges, ncross) in {0..4} x {0..4} but (0, 0), on curves of up to 40000 samples: the crossing pre-search
    is on (its index slots alias the head of fit_out, or cross_out when there are no ranges; nranges = 1 with ncross = 4
    puts 6 slots into one 8-double record)."""
    cv = host_curves(40000)
    names, curves = [n for n, _ in cv], [c for _, c in cv]
    for ncross in range(5):
        if nranges == 0 and ncross == 0:
            continue
        ranges, cross = RANGE_POOL[:nranges], CROSS_POOL[:ncross]
        fit, cr = curve_fits(eng, curves, ranges, cross, 8, phase=nranges + ncross)
        _check_records_b("ira_curve_fits", names, curves, fit, cr, ranges, cross, 8)


@pytest.mark.parametrize("max_n", [2048, 2049, 32768, 32769])
def test_curve_fits_workgroup_sizes(eng, max_n):
    """max_len at the edges of the 64 / 256 / 1024-thread choice and of the pre-search threshold."""
    cv = host_curves(max_n)
    names, curves = [f"{max_n}/{n}" for n, _ in cv], [c for _, c in cv]
    fit, cr = curve_fits(eng, curves, FOUR, R.PRODUCT_CROSS, 8, phase=max_n % 7)
    _check_records_b("ira_curve_fits", names, curves, fit, cr, FOUR, R.PRODUCT_CROSS, 8)


FOUR = R.FOUR_RANGES


@pytest.mark.parametrize("t_mul,t_div", [(1.0, 48000.0), (512.0, 48000.0), (1.0, 44100.0)])
def test_curve_fits_analytic_axes(eng, t_mul, t_div):
    for max_n in (2049, 40000):
        cv = host_curves(max_n)
        names, curves = [f"{max_n}/{n}" for n, _ in cv], [c for _, c in cv]
        fit, cr = curve_fits(eng, curves, RANGE_POOL[:3], R.PRODUCT_CROSS, 8, t_mul=t_mul, t_div=t_div)
        _check_records_b("ira_curve_fits", names, curves, fit, cr, RANGE_POOL[:3], R.PRODUCT_CROSS, 8, t_mul=t_mul, t_div=t_div)
    if t_mul == 1.0 and t_div == 48000.0:                              # the slope of an exact line, in closed form
        k = [n for n, _ in host_curves(2049)].index("line")
        fit, _ = curve_fits(eng, [host_curves(2049)[k][1]], [(-5.0, -35.0)], (), 8)
        assert fit[0, 0, 0] == 1.0 and abs(fit[0, 0, 3] + 0.0625 * 48000.0) < 1e-6 * 3000.0 and fit[0, 0, 7] == 481
        assert abs(fit[0, 0, 6] - 0.02) < 1e-7 and abs(fit[0, 0, 5] - 1.0) < 1e-9


def test_curve_fits_explicit_axis(eng):
    """t_axis_dev: an increasing, non-uniform float32 axis shared by all curves."""
    for max_n in (2049, 40000):
        cv = host_curves(max_n)
        names, curves = [f"{max_n}/{n}" for n, _ in cv], [c for _, c in cv]
        i = np.arange(max_n + 3, dtype=np.float64)
        axis = (0.25 + (i / SR) * (1.0 + 0.3 * i / max_n) + 1e-4 * np.sin(i / 37.0) / SR).astype(np.float32)
        assert np.all(np.diff(axis) > 0)
        fit, cr = curve_fits(eng, curves, RANGE_POOL[:3], R.PRODUCT_CROSS, 8, t_axis=axis)
        _check_records_b("ira_curve_fits", names, curves, fit, cr, RANGE_POOL[:3], R.PRODUCT_CROSS, 8, t=axis)


@pytest.mark.parametrize("min_points", [2, 8, 10])
def test_curve_fits_min_points(eng, min_points):
    """Ranges that hold min_points - 1, min_points and min_points + 1 samples of a line of exactly 1 dB per sample."""
    y = _line(300, 1.0)
    ranges = [(-5.0, -5.0 - (min_points - 2)), (-5.0, -5.0 - (min_points - 1)), (-5.0, -5.0 - min_points)]
    curves = [y, y[:40].copy(), _line(300, 0.5)]
    names = [f"unit{min_points}", f"unit40/{min_points}", f"half{min_points}"]
    fit, cr = curve_fits(eng, curves, ranges, (), min_points)
    _check_records_b("ira_curve_fits", names, curves, fit, cr, ranges, (), min_points)
    if min_points > 2:
        assert list(fit[0, :, 7]) == [min_points - 1, min_points, min_points + 1]
        assert list(fit[0, :, 0]) == [0.0, 1.0, 1.0]
    else:
        assert fit[0, 0, 0] == 0.0 and list(fit[0, 1:, 7]) == [2, 3] and list(fit[0, 1:, 0]) == [1.0, 1.0]


def test_curve_fits_rel_to_peak(eng):
    """Modal-cloud mode: curves shifted by their own float32 maximum; peaks just under, on and just over
    min_peak_above_floor; non-finite curves flagged.  Short curves (64 threads) and 40000-sample ones (1024 threads; the
    pre-search stays off in this mode)."""
    floor_db, min_peak = -120.0, 30.0
    for max_n in (600, 40000):
        names, curves = [], []
        for nm, c in host_curves(max_n):
            for shift in (-90.0 - 1e-5, -90.0, -90.0 + 1e-5, -20.0):
                with np.errstate(all="ignore"):
                    curves.append((c + np.float32(shift)).astype(np.float32))
                names.append(f"{max_n}/{nm}{shift:+.6f}")
        for mp in (10, 8):
            fit, cr = curve_fits(eng, curves, RANGE_POOL[:2], R.PRODUCT_CROSS, mp, t_mul=512.0, rel=(floor_db, min_peak))
            _check_records_b("ira_curve_fits", names, curves, fit, cr, RANGE_POOL[:2], R.PRODUCT_CROSS, mp, t_mul=512.0,
                             rel=(floor_db, min_peak))
        usable = np.array([R.rel_to_peak(c, floor_db, min_peak)[1] for c in curves])
        assert usable.any() and (~usable).any()
        assert np.all(np.isnan(fit[~usable][:, :, 1:])) and np.all(fit[~usable][:, :, 0] == 0.0) and np.all(np.isnan(cr[~usable]))


def test_curve_fits_more_than_65535_curves(eng):
    """65536 + 3 short curves and one of 40000 samples in one launch (the curve count turns the pre-search off): records
    bit-identical to the same curves launched in two halves (the half with the long curve pre-searches), and a sample of
    them against the oracle."""
    rng = np.random.default_rng(5)
    n = 65536 + 3
    lens = rng.integers(4, 36, size=n)
    curves = [(-rng.random() * 9.0 * np.arange(m) + rng.standard_normal(m) * 0.2).astype(np.float32) for m in lens]
    long_at = 40000
    curves.insert(long_at, host_curves(40000)[0][1])
    ranges, cross = RANGE_POOL[:2], R.PRODUCT_CROSS
    fit, cr = curve_fits(eng, curves, ranges, cross, 2)
    h = 32770
    f1, c1 = curve_fits(eng, curves[:h], ranges, cross, 2)
    f2, c2 = curve_fits(eng, curves[h:], ranges, cross, 2)
    assert len(curves[h:]) <= 65535 and max(len(c) for c in curves[:h]) < 40000
    np.testing.assert_array_equal(fit.view(np.uint64), np.concatenate([f1, f2]).view(np.uint64))
    np.testing.assert_array_equal(cr.view(np.uint64), np.concatenate([c1, c2]).view(np.uint64))
    pick = sorted(set(rng.integers(0, n, size=300).tolist() + [0, long_at - 1, long_at, long_at + 1, n]))
    _check_records_b("ira_curve_fits", [f"many{i}" for i in pick], [curves[i] for i in pick], fit[pick], cr[pick], ranges,
                     cross, 2)
    assert 0 < np.sum(fit[:, :, 0] == 1.0) < fit.shape[0] * 2


# -------------------------------------------------------------------------------------------------------- ira_edc_fits
def _fits_on_emitted(entry, batch, eps, floor_db, ranges, cross, min_points, phase=0, parts=None, tag=""):
    """One launch with the curve and one without: records bit-identical; the emitted curve by comparison A; the records
    by comparison B against the oracle on the emitted curve."""
    segs = [x for _, x in batch]
    fit, cr, edc = edc_fits(eng=entry[0], segs=segs, eps=eps, floor_db=floor_db, ranges=ranges, cross=cross,
                            min_points=min_points, want_edc=True, phase=phase, parts=parts)
    fit2, cr2, none = edc_fits(eng=entry[0], segs=segs, eps=eps, floor_db=floor_db, ranges=ranges, cross=cross,
                               min_points=min_points, want_edc=False, phase=phase + 1, parts=parts)
    assert none is None
    np.testing.assert_array_equal(fit.view(np.uint64), fit2.view(np.uint64))
    np.testing.assert_array_equal(cr.view(np.uint64), cr2.view(np.uint64))
    _check_curves(entry[1], batch, eps, floor_db, edc)
    names = [f"{tag}{eps}/{floor_db}/{nm}" for nm, _ in batch]
    # keyed by name, eps and floor: the reference runs on the curve THIS launch emitted
    _check_records_b(entry[1], names, edc, fit, cr, ranges, cross, min_points)
    return fit, cr, edc


def test_edc_fits_product_ranges(eng):
    b = main_batch()
    fit, cr, edc = _fits_on_emitted((eng, "ira_edc_fits"), b, 1e-20, -120.0, R.PRODUCT_RANGES, R.PRODUCT_CROSS, 8)
    names = [nm for nm, _ in b]
    assert fit[names.index("ir480000/last-tile"), 2, 0] == 1.0
    assert np.isnan(fit[:, 2, 2]).any() and np.isnan(cr[:, 1]).any()          # levels that are never reached (eps clamp)


def test_edc_fits_disjoint_ranges_floor_as_target(eng):
    """Two disjoint ranges in one launch (the moments kernel walks the union of their tiles), a range that ends on the
    floor, one whose upper level is never reached by most segments, and the floor as a crossing target."""
    b = main_batch()
    ranges = ((0.0, -10.0), (-40.0, -60.0), (-5.0, -120.0), (-110.0, -120.0))
    _fits_on_emitted((eng, "ira_edc_fits"), b, 1e-20, -120.0, ranges, (0.0, -10.0, -120.0, -60.0), 8, phase=2)
    small = [(nm, x) for nm, x in b if len(x) <= 32769]
    _fits_on_emitted((eng, "ira_edc_fits"), small, 1e-20, -60.0, ((0.0, -10.0), (-40.0, -60.0)), (-60.0,), 8, phase=4)


def test_edc_fits_low_levels_and_record_shapes(eng):
    """eps = 1e-90 and eps = 0 (subnormal samples, exact-zero tails); nranges = 0 with crossings only and ranges without
    crossings."""
    b = _low_level_batch()
    _fits_on_emitted((eng, "ira_edc_fits"), b, 1e-90, -300.0, R.PRODUCT_RANGES, R.PRODUCT_CROSS, 8, phase=1)
    _fits_on_emitted((eng, "ira_edc_fits"), b, 0.0, -300.0, ((-5.0, -25.0), (-100.0, -250.0)), (), 8, phase=2)
    _fits_on_emitted((eng, "ira_edc_fits"), b, 1e-20, -120.0, (), CROSS_POOL, 8, phase=3)


def test_edc_fits_end_to_end(eng):
    """Comparison C (and A and B) on the end-to-end inputs with four ranges: nothing of the GPU in the reference.  The last
    two segments' -5 .. -65 dB range spans more than 320 tiles (chunks of more than four tiles in the moments kernel);
    the last one is the documented maximum of 2047 tiles."""
    b = R.end_to_end_inputs()
    fit, cr, edc = _fits_on_emitted((eng, "ira_edc_fits"), b, 1e-20, -120.0, FOUR, R.PRODUCT_CROSS, 8, tag="e2e")
    assert fit[-1, 3, 7] > 320 * 4096 and fit[-2, 3, 7] > 320 * 4096
    ref = [R.end_to_end_records(x, FOUR, R.PRODUCT_CROSS, 8) for _, x in b]
    st = R.compare_end_to_end(fit.reshape(-1, 8), np.concatenate([r for r, _ in ref]))
    for i, (_, c) in enumerate(ref):
        assert np.array_equal(np.isnan(cr[i]), np.isnan(c)) and np.all(np.abs(cr[i] - c)[~np.isnan(c)] < 1e-7)
    _note("ira_edc_fits", **{f"C_{k}": v for k, v in st.items()})
    # the 200 s decay of the existing fused test: 0 .. -10 dB over about 370 tiles
    slow = [("ir2880000/rt200", R.ir(79, 2_880_000, 200.0))]
    fit, _, _ = _fits_on_emitted((eng, "ira_edc_fits"), slow, 1e-20, -120.0, R.PRODUCT_RANGES, R.PRODUCT_CROSS, 8, phase=3)
    assert fit[0, 0, 0] == 1.0 and fit[0, 0, 7] > 320 * 4096


def test_edc_fits_flat_masks(eng):
    """Two impulses with silence between them: the curve stands at -3.01 dB from the second sample to the later impulse
    and falls to the floor behind it, so the mask of (-1, -10) holds equal values only.  The least-squares line is flat:
    slope exactly 0, refused, in the fused path as in ira_curve_fits (the shifted moments alone leave rounding noise of
    either sign there).  The same with a plateau of leading silence at 0 dB and the range (0, -10)."""
    batch = []
    for n, k in ((2000, 1000), (20000, 12345), (70000, 69990)):
        x = np.zeros(n, np.float32)
        x[0], x[k] = 1.0, -1.0
        batch.append((f"two_impulses{n}", x))
        y = np.zeros(n, np.float32)
        y[k:k + 3] = [1.0, 0.01, -0.001]                               # 0 dB up to sample k, -40 dB one sample later
        batch.append((f"plateau{n}", y))
    ranges = ((-1.0, -10.0), (0.0, -10.0), (-2.0, -3.5))
    fit, cr, edc = _fits_on_emitted((eng, "ira_edc_fits"), batch, 1e-20, -120.0, ranges, R.PRODUCT_CROSS, 2, tag="flat")
    fc, _ = curve_fits(eng, edc, ranges, (), 2)
    np.testing.assert_array_equal(fit[:, :, 0], fc[:, :, 0])
    v = np.float32(10.0 * np.log10(0.5))
    for i, k in ((0, 1000), (2, 12345), (4, 69990)):                  # the mask is 1 .. k
        for r in (0, 2):
            assert list(fit[i, r, [0, 3, 5, 6, 7]]) == [0.0, 0.0, 0.0, -np.inf, k] and fit[i, r, 4] == v, fit[i, r]
            assert list(fc[i, r, [0, 3, 5, 6, 7]]) == [0.0, 0.0, 0.0, -np.inf, k] and fc[i, r, 4] == v, fc[i, r]
    for i in (1, 3, 5):
        assert list(fit[i, 1, [0, 3, 4, 5, 6]]) == [0.0, 0.0, 0.0, 0.0, -np.inf], fit[i, 1]


def _tile_parts(batch, seed=0):
    """Partial tile energies laid out as include/ira.h documents for tile_part_dev: for every segment but each third one,
    the float64 energy of each 4096-sample tile (counted from the end) split at random over W in {1, 3, 8} workgroups at
    part[part_off + w * part_tiles + j].  part_tiles is the producer's tile count (more than the segment's, whose front was
    trimmed); the entries the kernel must not read (the tile that holds the first sample, and beyond) hold 1e30."""
    rng = np.random.default_rng(seed)
    blocks, p_off, p_wgs, p_tiles, pos = [], [], [], [], 3
    blocks.append(np.full(3, 1e30))
    for s, (_, x) in enumerate(batch):
        n = len(x)
        ntiles = (n + R.TILE - 1) // R.TILE
        w = (1, 3, 8)[s % 3]
        tiles = ntiles + s % 3
        if s % 3 == 2:
            p_off.append(-1); p_wgs.append(0); p_tiles.append(0)
            continue
        blk = np.full((w, tiles), 1e30)
        e = x.astype(np.float64) ** 2
        for j in range(ntiles - 1):
            ej = float(np.sum(e[n - (j + 1) * R.TILE:n - j * R.TILE]))
            share = rng.random(w) + 0.05
            share = ej * share / share.sum()
            share[-1] = ej - float(np.sum(share[:-1]))
            blk[:, j] = share
        blocks.append(blk.reshape(-1))
        p_off.append(pos); p_wgs.append(w); p_tiles.append(tiles)
        pos += blk.size
    return (np.concatenate(blocks), np.array(p_off, np.int64), np.array(p_wgs, np.int32), np.array(p_tiles, np.int32))


def test_edc_fits_tile_partials(eng):
    """tile_part_dev: tile energies from a producer's partial sums instead of a second read of the samples, mixed with
    part_off < 0 segments.  The curve must still meet comparison A (the partial sums add W roundings to a tile total,
    inside the allowance for the sum), the records B, and C on the plain decays."""
    b = [(nm, x) for nm, x in main_batch() if np.all(np.isfinite(x)) and len(x) >= 255] + R.end_to_end_inputs()[:8]
    parts = _tile_parts(b, seed=3)
    assert np.sum(parts[1] >= 0) > 20 and np.sum(parts[1] < 0) > 10
    fit, cr, edc = _fits_on_emitted((eng, "ira_edc_fits(tile_part)"), b, 1e-20, -120.0, R.PRODUCT_RANGES, R.PRODUCT_CROSS,
                                    8, phase=1, parts=parts, tag="parts")
    e2e = b[-8:]
    ref = np.concatenate([R.end_to_end_records(x, R.PRODUCT_RANGES, R.PRODUCT_CROSS, 8)[0] for _, x in e2e])
    st = R.compare_end_to_end(fit[-8:].reshape(-1, 8), ref)
    _note("ira_edc_fits(tile_part)", **{f"C_{k}": v for k, v in st.items()})


def test_edc_fits_single_segments(eng):
    """nseg = 1 at every offset residue."""
    b = dict(main_batch())
    for phase, name in enumerate(("ir4097/rt0.08", "ir16385/rt0.08", "lead4096/ir32767", "nan_mid4097", "ir5/rt0.3")):
        _fits_on_emitted((eng, "ira_edc_fits"), [(name, b[name])], 1e-20, -120.0, R.PRODUCT_RANGES, R.PRODUCT_CROSS, 8,
                         phase=phase)


def test_zz_report():
    """Prints the measured figures (run with -s): per entry point the worst deviation under A (as a share of the
    allowance and in dB), B and C, and the smallest share of float32 samples bit-identical to the long-double reference
    over the launches."""
    for entry in sorted(STATS):
        print(entry)
        for k in sorted(STATS[entry]):
            print(f"    {k:28s} {STATS[entry][k]:.6g}")
