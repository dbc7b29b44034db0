"""
ira_spectrum_finish (dB, unwrapped phase and statistics in one pass, ira_spectrum.hip: spectrum_finish_kernel) against the
three calls it replaces and against the restatement of tests/spectrum_ref.py.

  unpacked elements   every output has the BYTES of ira_spectrum_mag_phase -> ira_phase_unwrap -> ira_spectrum_stats on the
                      same input: dB, float32 degrees / radians, float64 radians, the statistics record, unwrap on and off,
                      alone and in a ragged batch
  packed elements     the three calls' own twiddle depends on their launch's grid stride, so byte equality with them is not
                      defined.  Instead: dB and the wrapped angles within the bars of test_gpu_spectrum.check_mag_phase (DC
                      and Nyquist exactly 0 or pi), the unwrapped float64 bit-equal to spectrum_ref.unwrap_tree of the kernel's
                      own wrapped angles, float32 outputs within half a float32 ulp of (float64 result * scale), statistics
                      byte-equal to ira_spectrum_stats on the kernel's own dB array and held to spectrum_ref.stats
  statistics          the tie, range and NaN rules of spectrum_ref.stats_cases through spectra with those dB values
  optional outputs    leaving any output out changes no byte of the others
The inputs are built in tests/spectrum_finish_cases.py; tests/test_spectrum_finish_cpu.py proves their planted conditions.

Measured on an MI355X: 184 649 unpacked bins x 4 floors x 4 modes byte-equal to the three calls; packed angles 4.1e-16 to
6.6e-16 of bounds 7.8e-15 to 1.1e-14 (the twiddle is one complex product, not a rotation), packed dB and the float32
phases at their float32 half-ulp (ratios 0.92 to 0.997), statistics' sums below 0.05 of their bound, the unwrap bit-equal
to unwrap_tree on every element, the 525 314-bin element past the twiddle table included.
"""
import numpy as np
import pytest

import spectrum_finish_cases as C
import spectrum_ref as R
from test_gpu_spectrum import _layout, check_mag_phase, report

pytestmark = pytest.mark.gpu

LD, F32, U = R.LD, R.F32, R.U
OUTS = ("mag", "p32", "p64", "wr", "stats")


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def _upload(eng, elems):
    lengths, bins, off = _layout([e[0] for e in elems])
    spec = np.concatenate([np.asarray(e[1], dtype=np.complex128)[:b] for e, b in zip(elems, bins)])
    return eng.to_dev(spec.view(np.float64)), lengths, bins, off


def _vals(lengths):
    return 48000.0 / np.maximum(np.asarray(lengths, dtype=np.float64), 1.0)


def finish(eng, d_spec, off, lengths, floor_db=-120.0, packed=None, outs=OUTS, unwrap=True, degrees=True, val=None,
           f_min=20.0, f_max=20000.0, probe=1000.0):
    """One ira_spectrum_finish call with exactly the outputs named in `outs` -> {name: host array}."""
    from audio_analysis_amd.engine import _ptr, check
    t = eng.torch
    n = int(off.size)
    total = int((lengths.astype(np.int64) // 2 + 1).sum())
    buf = dict(mag=eng.empty(total, t.float32), p32=eng.empty(total, t.float32), p64=eng.empty(total, t.float64),
               wr=eng.empty(total, t.float64), stats=eng.empty(n * 8, t.float64))
    p = {k: (_ptr(v) if k in outs else 0) for k, v in buf.items()}
    val = _vals(lengths) if val is None else np.ascontiguousarray(val, np.float64)
    d_o, d_l, d_pk, d_fv = eng.job_tables(off, lengths, None if packed is None else np.ascontiguousarray(packed, np.int32), val)
    check(eng.lib.ira_spectrum_finish(_ptr(d_spec), _ptr(d_o), _ptr(d_l), n, float(floor_db), _ptr(d_pk), p["mag"], _ptr(d_o),
                                      1 if unwrap else 0, 1 if degrees else 0, p["p32"], p["p64"], p["wr"], _ptr(d_fv),
                                      float(f_min), float(f_max), float(probe), p["stats"], eng.stream), "ira_spectrum_finish")
    eng.sync()
    size = dict(mag=total, p32=total, p64=total, wr=total, stats=n * 8)
    return {k: buf[k].cpu().numpy()[: size[k]].copy() for k in outs}


def chain(eng, d_spec, off, lengths, floor_db, unwrap, degrees, val, f_min=20.0, f_max=20000.0, probe=1000.0):
    """The three calls on the same input -> the same dict."""
    mag, ph = eng.spectrum_mag_phase(d_spec, off, lengths, floor_db, want_phase=True)
    out = dict(mag=mag.cpu().numpy(), wr=ph.cpu().numpy())
    out["p32"] = eng.phase_unwrap(ph, off, lengths, unwrap, degrees).cpu().numpy()
    out["p64"] = eng.phase_unwrap(ph, off, lengths, unwrap, False, as_float64=True).cpu().numpy()
    out["stats"] = eng.spectrum_stats(mag, off, lengths, val, f_min, f_max, probe).cpu().numpy().reshape(-1)
    return out


def same_bytes(got, want, what):
    for k in got:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype and g.size == w.size, (what, k, g.dtype, w.dtype, g.size, w.size)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.view(f"u{g.itemsize}") != w.view(f"u{w.itemsize}"))
            raise AssertionError((what, k, f"{bad.size} of {g.size} values differ, first at", bad[:8], g[bad[:8]], w[bad[:8]]))


# ================================================================================================= 1, 2: unpacked
@pytest.mark.parametrize("floor_db", R.MP_FLOORS)
def test_01_unpacked_ragged_batch_has_the_chain_s_bytes(floor_db):
    """One ragged launch of 50 elements, 1 to 12289 bins (every planted operand of R.mag_phase_batch; steps, windings and a
    caller's phases at the tile, thread and wave edges): every output byte for byte what the three calls give."""
    eng = _eng()
    elems = C.unpacked_batch()
    d_spec, lengths, bins, off = _upload(eng, elems)
    val = _vals(lengths)
    for unwrap in (True, False):
        for degrees in (True, False):
            want = chain(eng, d_spec, off, lengths, floor_db, unwrap, degrees, val)
            got = finish(eng, d_spec, off, lengths, floor_db, unwrap=unwrap, degrees=degrees, val=val)
            same_bytes(got, want, f"floor {floor_db} unwrap {unwrap} degrees {degrees}")
    print(f"SPEC-ERR finish unpacked floor {floor_db}: {int(bins.sum())} bins x 4 modes byte-equal to the three calls")


def test_02_unpacked_alone_equals_batch():
    eng = _eng()
    elems = list(R.mag_phase_batch()) + [e for e in C.unit_spectra() if e[0] // 2 + 1 in (1, 4097, 12289)]
    d_spec, lengths, bins, off = _upload(eng, elems)
    val = _vals(lengths)
    batch = finish(eng, d_spec, off, lengths, val=val)
    for i, (L, s) in enumerate(elems):
        d1, l1, b1, o1 = _upload(eng, [(L, s)])
        one = finish(eng, d1, o1, l1, val=val[i : i + 1])
        o, b = int(off[i]), int(bins[i])
        part = {k: (batch[k][8 * i : 8 * i + 8] if k == "stats" else batch[k][o : o + b]) for k in batch}
        same_bytes(one, part, f"element {i} L {L}")


# ========================================================================================================= 3: packed
def test_03_packed():
    eng = _eng()
    batch = C.packed_batch()
    d_spec, lengths, bins, off = _upload(eng, batch)
    packed = np.array([pk for _, _, pk, _ in batch], dtype=np.int32)
    val = _vals(lengths)
    got = {}
    for degrees in (True, False):
        got[degrees] = finish(eng, d_spec, off, lengths, packed=packed, degrees=degrees, val=val)
    raw = finish(eng, d_spec, off, lengths, packed=packed, unwrap=False, degrees=False, val=val)
    g = got[True]
    assert g["mag"].tobytes() == got[False]["mag"].tobytes() and g["wr"].tobytes() == raw["wr"].tobytes()
    assert raw["p64"].tobytes() == raw["wr"].tobytes()           # unwrap off: the wrapped angles come back
    # the statistics are those of ira_spectrum_stats on the kernel's own dB array, to the byte
    own = eng.spectrum_stats(eng.to_dev(g["mag"]), off, lengths, val, 20.0, 20000.0, 1000.0).cpu().numpy().reshape(-1)
    assert g["stats"].tobytes() == own.tobytes()
    scale = 180.0 / R.KPI
    for i, (L, z, pk, _) in enumerate(batch):
        o, b = int(off[i]), int(bins[i])
        db, wr, u = g["mag"][o : o + b], g["wr"][o : o + b], g["p64"][o : o + b]
        what = f"finish packed={pk} L {L}"
        ref = R.mag_db_phase(z, L, -120.0, packed=bool(pk))
        check_mag_phase(db, wr, ref, what, packed=bool(pk))
        if pk:
            assert np.all(C.winding_margin(ref) > 0), what
            assert set(R.bits64(wr[[0, -1]]).tolist()) <= set(R.bits64([0.0, R.KPI]).tolist()), (what, wr[[0, -1]])
        tree = R.unwrap_tree(wr)
        same = R.bits64(u) == R.bits64(tree)
        assert np.all(same), (what, "not unwrap_tree of the kernel's own angles at bins", np.flatnonzero(~same)[:8])
        for degrees, sc, unit in ((True, scale, "deg"), (False, 1.0, "rad")):
            v = u * sc
            bar = 2.0 ** -24 * np.abs(v) * (1 + 2.0 ** -20) + U * np.abs(v) + 2.0 ** -150
            report(f"finish f32 {unit}", what, np.abs(got[degrees]["p32"][o : o + b].astype(np.float64) - v), bar)
        rec = g["stats"][8 * i : 8 * i + 8]
        want, aux = R.stats(db, L, val[i], 20.0, 20000.0, 1000.0)
        for f in (0, 1, 2, 5, 6, 7):
            assert rec[f] == want[f] or (np.isnan(rec[f]) and np.isnan(want[f])), (what, "field", f, rec, want)
        if not pk:
            # the unpacked elements between the packed ones carry magnitudes of 2^+-60 (up to +-360 dB), where float32(dB) / 20
            # alone is off by more than sums_bound's unit error of exp10; their sums are held above, to the byte, to
            # ira_spectrum_stats, and unpacked elements to the three calls in test_01
            continue
        for f, s, a in ((3, aux["s3"], aux["abs3"]), (4, aux["s4"], aux["abs4"])):
            report(f"finish stats field {f}", what, abs(float(LD(rec[f]) - s)), R.sums_bound(a, aux["n_in"]))


# ====================================================================================================== 4: statistics
@pytest.mark.parametrize("kind", R.ST_KINDS)
def test_04_statistics_rules(kind):
    """The cases of test_gpu_spectrum.test_08 through the fused call: spectra whose dB values are the cases' arrays (no floor),
    1 to 40001 bins -- 16385 and 40001 are past one sweep of stats_kernel's 16-deep load loop."""
    eng = _eng()
    g = {c["name"]: c for c in R.stats_cases()}[kind]
    elems = [(L, C.stats_spectrum(m)) for L, _, m in g["elems"]]
    d_spec, lengths, bins, off = _upload(eng, elems)
    assert [int(b) for b in bins] == R.ST_BINS
    val = np.array([v for _, v, _ in g["elems"]])
    got = finish(eng, d_spec, off, lengths, floor_db=-np.inf, outs=("mag", "stats"), val=val, f_min=g["f_min"],
                 f_max=g["f_max"], probe=g["probe"])
    own = eng.spectrum_stats(eng.to_dev(got["mag"]), off, lengths, val, g["f_min"], g["f_max"], g["probe"]).cpu().numpy()
    assert got["stats"].tobytes() == own.reshape(-1).tobytes(), kind
    for i, (L, v, m) in enumerate(g["elems"]):
        o, b = int(off[i]), int(bins[i])
        db = got["mag"][o : o + b]
        what = f"finish {kind} bins {b}"
        assert np.array_equal(np.isnan(db), np.isnan(m)) and np.all((db == m) | np.isnan(m)), (what, "the dB values are not the case's")
        rec = got["stats"][8 * i : 8 * i + 8]
        ref, aux = R.stats(db, L, v, g["f_min"], g["f_max"], g["probe"])
        for f in (0, 1, 2, 5, 6, 7):
            assert rec[f] == ref[f] or (np.isnan(rec[f]) and np.isnan(ref[f])), (what, "field", f, rec, ref)
        for f, s, a in ((3, aux["s3"], aux["abs3"]), (4, aux["s4"], aux["abs4"])):
            if np.isnan(ref[f]):
                assert np.isnan(rec[f]), (what, f, rec)
            else:
                report(f"finish stats field {f}", what, abs(float(LD(rec[f]) - s)), R.sums_bound(a, aux["n_in"]))


# ================================================================================================ 5: optional outputs
def test_05_leaving_an_output_out_changes_no_other():
    eng = _eng()
    batch = C.packed_batch()
    d_spec, lengths, bins, off = _upload(eng, batch)
    packed = np.array([pk for _, _, pk, _ in batch], dtype=np.int32)
    full = finish(eng, d_spec, off, lengths, packed=packed)
    for leave in OUTS:
        outs = tuple(k for k in OUTS if k != leave and not (leave == "mag" and k == "stats"))     # stats needs mag
        part = finish(eng, d_spec, off, lengths, packed=packed, outs=outs)
        same_bytes(part, {k: full[k] for k in outs}, f"without {leave}")
    for outs in (("mag",), ("mag", "stats"), ("p64",), ("p32",), ("wr",)):
        same_bytes(finish(eng, d_spec, off, lengths, packed=packed, outs=outs), {k: full[k] for k in outs}, f"only {outs}")
    # and the engine's method is that call
    done = eng.spectrum_finish(d_spec, off, lengths, -120.0, packed=packed, want_phase=True, want_wrapped=True,
                               stats=(_vals(lengths), 20.0, 20000.0, 1000.0))
    assert done["mag"].cpu().numpy()[: full["mag"].size].tobytes() == full["mag"].tobytes()
    assert done["phase"].cpu().numpy()[: full["p32"].size].tobytes() == full["p32"].tobytes()
    assert done["wrapped"].cpu().numpy()[: full["wr"].size].tobytes() == full["wr"].tobytes()
    assert done["stats"].cpu().numpy().reshape(-1).tobytes() == full["stats"].tobytes()
    rad = eng.spectrum_finish(d_spec, off, lengths, packed=packed, want_mag=False, want_phase=True, degrees=False,
                              as_float64=True)
    assert rad["mag"] is None and rad["stats"] is None
    assert rad["phase"].cpu().numpy()[: full["p64"].size].tobytes() == full["p64"].tobytes()


# ========================================================================= 6: past the table of tile twiddles (packed)
def test_06_packed_element_longer_than_the_twiddle_table():
    """525 314 bins: the kernel's LDS table of W^(1024 q) covers 512 x 1024 of them and is rebuilt, between two barriers of its
    own, at tile 128; the same rules as test_03, on both sides of the rebuild."""
    eng = _eng()
    L, z, _ = C.long_packed()
    d_spec, lengths, bins, off = _upload(eng, [(L, z)])
    packed = np.ones(1, dtype=np.int32)
    val = _vals(lengths)
    g = finish(eng, d_spec, off, lengths, packed=packed, val=val)
    what = f"finish packed long L {L}"
    ref = R.mag_db_phase(z, L, -120.0, packed=True)
    assert np.all(C.winding_margin(ref) > 0), what
    check_mag_phase(g["mag"], g["wr"], ref, what, packed=True)
    assert set(R.bits64(g["wr"][[0, -1]]).tolist()) <= set(R.bits64([0.0, R.KPI]).tolist()), (what, g["wr"][[0, -1]])
    same = R.bits64(g["p64"]) == R.bits64(R.unwrap_tree(g["wr"]))
    assert np.all(same), (what, "not unwrap_tree of the kernel's own angles at bins", np.flatnonzero(~same)[:8])
    v = g["p64"] * (180.0 / R.KPI)
    bar = 2.0 ** -24 * np.abs(v) * (1 + 2.0 ** -20) + U * np.abs(v) + 2.0 ** -150
    report("finish f32 deg", what, np.abs(g["p32"].astype(np.float64) - v), bar)
    own = eng.spectrum_stats(eng.to_dev(g["mag"]), off, lengths, val, 20.0, 20000.0, 1000.0).cpu().numpy().reshape(-1)
    assert g["stats"].tobytes() == own.tobytes()
    want, aux = R.stats(g["mag"], L, val[0], 20.0, 20000.0, 1000.0)
    for f in (0, 1, 2, 5, 6, 7):
        assert g["stats"][f] == want[f], (what, "field", f, g["stats"], want)
    for f, s, a in ((3, aux["s3"], aux["abs3"]), (4, aux["s4"], aux["abs4"])):
        report(f"finish stats field {f}", what, abs(float(LD(g["stats"][f]) - s)), R.sums_bound(a, aux["n_in"]))
