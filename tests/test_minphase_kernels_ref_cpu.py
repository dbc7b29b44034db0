"""tests/minphase_kernels_ref.py on a machine without a GPU: an honest float64 NumPy emulation of each kernel of
ira_minphase.hip passes every checker on every case of the tables tests/test_gpu_minphase_kernels.py launches, every
subtly wrong kernel modelled here is rejected by the case named beside it, and the long-double restatements agree with
the float64 chain of tests/minphase_ref.py to the rounding that chain's own arithmetic allows."""
import math

import numpy as np
import pytest

import minphase_kernels_ref as K
import minphase_ref as R


@pytest.fixture(scope="module", autouse=True)
def _longdouble():
    K.need_longdouble()


# ------------------------------------------------------------------------------------------------------ the emulations
def emu_logmag(els, floor_db, wrong=None):
    """[(G complex128, P, count)] per element, float64 NumPy, as the two kernels of ira_minphase_logmag compute them."""
    out = []
    fl = K.floor_lin(floor_db)
    for i, e in enumerate(els):
        nb = e["n"] // 2 + 1
        if wrong == "previous_n" and i:
            nb = min(nb, els[i - 1]["n"] // 2 + 1)
        p = K.power(e["X"])
        with np.errstate(all="ignore"):
            seen = p[: nb - 1] if wrong == "half_bins" else p[:nb]
            P = float(np.fmax.reduce(seen)) if wrong == "fmax" else (math.nan if np.isnan(seen).any() else float(np.max(seen)))
            g = np.full(p.size, np.nan) + 0j                       # a bin no lane reached holds whatever was there
            count = 0
            if K.valid(P):
                pf = P * fl
                below = p[:nb] <= pf if wrong == "floor_le" else p[:nb] < pf
                count = int(np.count_nonzero(below))
                v = np.maximum(p[:nb], pf)
                g[:nb] = 0.5 * (np.log(v.astype(np.float32)).astype(np.float64) if wrong == "log_f32" else np.log(v))
            else:
                g[:nb] = 0.0
        out.append((g, P, count))
    return out


def emu_excess(e, wrong=None):
    n, p = e["n"], e["p"]
    X, T = e["X"], e["T"]
    k = np.arange(n // 2 + 1, dtype=np.int64)
    if not e["valid"]:
        return np.zeros(k.size)
    two_pi = float(np.float32(K.TWO_PI)) if wrong == "two_pi_f32" else K.TWO_PI
    with np.errstate(all="ignore"):
        if wrong == "kp_f64":
            turn = k.astype(np.float64) * float(p) / float(n)
        elif wrong == "kp_i32":
            kp = (k * p).astype(np.int32).astype(np.int64)
            turn = np.fmod(kp, n).astype(np.float64) / float(n)
        else:
            turn = ((k * p) % n).astype(np.float64) / float(n)
        im = X.imag
        ang = np.arctan2(X.real, im) if wrong == "atan2_swapped" else np.arctan2(im, X.real)
        d = (ang + two_pi * turn) - 2.0 * T.imag
        if wrong == "fmod":
            return np.fmod(d + two_pi / 2.0, two_pi) - two_pi / 2.0 + np.where(d + two_pi / 2.0 < 0, two_pi, 0.0)
        return d - two_pi * np.rint(d / two_pi)


def emu_gather(els, bins, wrong=None):
    """(nb, npts, FIELDS) from the flat arrays, as the kernel indexes them."""
    off = np.cumsum([0] + [e["n"] // 2 + 1 for e in els])
    X, T, u = (np.concatenate([e[q] for e in els]) for q in ("X", "T", "u"))
    out = np.empty((len(els), bins.shape[1], K.FIELDS))
    for i, e in enumerate(els):
        k = bins[i].astype(np.int64)
        if wrong != "unclamped":
            k = np.clip(k, 1, e["n"] // 2 - 1)
        if not e["valid"]:
            out[i] = np.nan
            continue
        at = lambda a, dk: np.take(a, off[i] + k + dk, mode="wrap")        # an index outside the element reads a neighbour
        lo, mid, hi = (0, 1, 2) if wrong == "neighbours" else (-1, 0, 1)
        rec = [at(X.real, 0), at(X.imag, 0), at(T.imag, lo), at(T.imag, mid), at(T.imag, hi), at(u, lo), at(u, mid), at(u, hi)]
        if wrong == "swapped":
            rec[4], rec[5] = rec[5], rec[4]
        out[i] = np.stack(rec, axis=1)
    return out


def emu_spectrum(e, wrong=None):
    if not e["valid"]:
        return np.zeros(e["G"].size, np.complex128)
    t2 = (1.0 if wrong == "angle_t" else 2.0) * e["T"].imag
    mag = np.exp(e["G"].real)
    m = mag * np.cos(t2) + 1j * (mag * np.sin(t2))
    m.imag[0] = 0.0
    if wrong != "nyquist_imag":
        m.imag[-1] = 0.0
    return m


# --------------------------------------------------------------------------------------------------------- the judging
def rejections(kernel, wrong=None):
    """The names of the cases that reject this emulation, judged by the checkers the GPU tests use."""
    els, hits = K.elements(), []

    def judge(name, fn):
        try:
            fn()
        except AssertionError:
            hits.append(name)

    if kernel == "logmag":
        for db in K.FLOORS_DB:
            for e, (g, P, c) in zip(els, emu_logmag(els, db, wrong)):
                judge(f"{e['name']}@{db:g}", lambda: K.check_logmag(g, P, c, e["X"], db))
    elif kernel == "excess":
        for e in els + (K.big_element(),):
            judge(e["name"], lambda: K.check_excess(emu_excess(e, wrong), e["X"], e["T"], e["p"], e["n"], e["valid"]))
    elif kernel == "gather":
        for npts in K.NPTS:
            for abi in ((False, True) if npts >= 6 else (False,)):
                bins = K.gather_bins(npts, abi)
                got = emu_gather(els, bins, wrong)
                for i, e in enumerate(els):
                    judge(f"{e['name']}/{npts}{'/abi' if abi else ''}",
                          lambda: K.check_gather(got[i], e["X"], e["T"], e["u"], bins[i], e["n"], e["valid"]))
    else:
        for e in els:
            judge(e["name"], lambda: K.check_spectrum(emu_spectrum(e, wrong), e["G"], e["T"], e["valid"]))
    return hits


@pytest.mark.parametrize("kernel", ["logmag", "excess", "gather", "spectrum"])
def test_the_honest_emulation_passes_every_case(kernel):
    assert rejections(kernel) == []


WRONG = (("logmag", "fmax", "nan_bin@-120", "the maximum by fmax drops a NaN"),
         ("logmag", "half_bins", "max_at_nyquist@-60", "the maximum over N/2 bins misses the last"),
         ("logmag", "floor_le", "equal_maxima@0", "<= at the floor counts a bin equal to P"),
         ("logmag", "floor_le", "planted@-60", "<= at the floor counts the bin planted on P_floor"),
         ("logmag", "log_f32", "max_at_0@-120", "the float32 logarithm"),
         ("logmag", "previous_n", "max_at_nyquist@-120", "an element's bins counted with the previous element's N"),
         ("excess", "kp_f64", "nine_groups", "k p in float64 without the integer reduction"),
         ("excess", "kp_f64", "big", "k p in float64 without the integer reduction"),
         ("excess", "fmod", "max_at_0", "fmod in place of rint resolves the tie the other way"),
         ("excess", "two_pi_f32", "equal_maxima", "the float32 2 pi"),
         ("excess", "atan2_swapped", "max_at_nyquist", "atan2(re, im)"),
         ("gather", "neighbours", "max_at_0/1", "neighbours k, k + 1, k + 2"),
         ("gather", "unclamped", "planted/479/abi", "an unclamped bin"),
         ("gather", "swapped", "equal_maxima/255", "two record fields swapped"),
         ("spectrum", "nyquist_imag", "max_at_nyquist", "Im M left non-zero at N/2"),
         ("spectrum", "angle_t", "planted", "sin and cos of t instead of 2 t"))


@pytest.mark.parametrize("kernel,wrong,case,why", WRONG, ids=[f"{w[1]}-{w[2]}" for w in WRONG])
def test_a_subtly_wrong_kernel_is_rejected_by_its_case(kernel, wrong, case, why):
    assert case in rejections(kernel, wrong), why


def test_kp_in_int32_is_the_same_function_and_is_not_rejected():
    """k p formed in int32 (two's complement wrap-around) is no wrong kernel for a power-of-two N: 2^32 is a multiple of
    N, so the wrapped product has the residue of the exact one, and C's remainder of a negative product differs from it
    by one whole turn, which the wrap removes.  No case rejects it, and the emulation differs from the honest one by
    rounding alone even at p = 2^31 - 1 and k p = 2^51; what a table CAN reject is the product that loses bits
    (kp_f64 above)."""
    assert rejections("excess", "kp_i32") == []
    e = K.big_element()
    a, b = emu_excess(e), emu_excess(e, "kp_i32")
    assert not np.array_equal(a, b) and np.max(np.abs(K.wrap64(a - b))) < 64 * K.U * 110.0


def test_fmod_differs_only_at_the_ties():
    """The fmod wrap is the same function except at d = odd multiple of pi, where it returns -pi for +pi: the exact-d bins
    of max_at_0 are what reject it, not a tolerance."""
    e = K.elements()[0]
    a, b = emu_excess(e), emu_excess(e, "fmod")
    assert a[1] == K.PI and b[1] == -K.PI and a[2] == -K.PI and b[2] == -K.PI
    assert np.max(np.abs(K.wrap64(a[10:] - b[10:]))) < 1e-13


# ------------------------------------------------------------------------------------------------- the tables themselves
def test_the_tables_hold_what_they_say():
    els = K.elements()
    assert [(e["name"], e["n"], e["p"]) for e in els] == [(n, s, p) for n, s, p, _ in K.ELEMENTS]
    by = {e["name"]: e for e in els}
    am = lambda name: int(np.argmax(K.power(by[name]["X"])))
    assert am("max_at_0") == 0 and am("max_at_nyquist") == 32 and am("max_in_last_group") == 1500 and am("nine_groups") == 8965
    assert 1500 % 512 >= 256 and 8965 % (9 * 256) >= 8 * 256                 # the workgroup (of 2, of 9) that owns the bin
    p = K.power(by["equal_maxima"]["X"])
    assert p[7] == p[100] == p.max() and np.count_nonzero(p == p.max()) == 2
    assert [by[n]["valid"] for n in ("zeros", "nan_bin", "inf_bin", "overflow")] == [False] * 4
    assert by["zeros"]["P"] == 0.0 and math.isnan(by["nan_bin"]["P"]) and by["inf_bin"]["P"] == math.inf
    assert by["overflow"]["P"] == math.inf and np.isfinite(by["overflow"]["X"].view(np.float64)).all()
    pl = K.power(by["planted"]["X"])
    assert by["planted"]["P"] == K.P_PLANTED and pl[2048] == np.nextafter(4.0, 0.0)
    for db in K.FLOORS_DB:
        pf = K.P_PLANTED * K.floor_lin(db)
        assert pf >= 2.2250738585072014e-308 * 2.0 ** 52                     # a normal number with room below it
        for s in K.PLANT_STEPS:
            if not (db == 0.0 and s > 0):
                assert np.count_nonzero(pl == K.steps(pf, s)) >= 1, (db, s)
        _, _, count = K.logmag(by["planted"]["X"], db)
        if db:
            assert count >= 5
        else:                                                              # at 0 dB every bin is below but the two at P
            assert count == pl.size - 2 and np.count_nonzero(pl == K.P_PLANTED) == 2
    _, _, count = K.logmag(by["equal_maxima"]["X"], 0.0)
    assert count == 257 - 2
    # the signed zeros, at k = 0 and N/2 among others
    sig = lambda z: (z.real, bool(np.signbit(z.real)), bool(np.signbit(z.imag)), z.imag)
    assert sig(by["max_at_nyquist"]["X"][0]) == (-1.0, True, False, 0.0) and sig(by["max_at_nyquist"]["X"][32])[:3] == (-8.0, True, True)
    assert sig(by["equal_maxima"]["X"][0])[:3] == (-1.0, True, True) and sig(by["equal_maxima"]["X"][256])[:3] == (-1.0, True, False)
    assert sig(by["max_in_last_group"]["X"][0])[1:3] == (False, False) and sig(by["max_in_last_group"]["X"][2048])[1:3] == (True, True)
    assert sig(by["max_at_nyquist"]["X"][3])[1:3] == (False, False) and sig(by["max_at_nyquist"]["X"][5])[1:3] == (True, True)
    # d = pi, -pi, 3 pi exactly, and the centres
    e = by["max_at_0"]
    ex = K.exact_bins(e["X"], e["p"], e["n"])
    assert ex[1:9].all() and list(-2.0 * e["T"].imag[1:4]) == [K.PI, -K.PI, 3.0 * K.PI]
    assert list(K.wrap64(-2.0 * e["T"].imag[1:3])) == [K.PI, -K.PI]
    assert {e["p"] for e in els} >= {0, 1, 511, 4096, (1 << 31) - 1}
    assert K.exact_bins(by["max_in_last_group"]["X"], 4096, 4096)[20:30].all()
    big = K.big_element()
    assert big["n"] == 1 << 21 and (big["n"] // 2) * big["p"] >= 1 << 50
    assert float(np.max(np.abs(np.concatenate([e["T"].imag for e in els])))) > 49.0
    for npts in K.NPTS:
        b = K.gather_bins(npts)
        assert b.shape == (len(els), npts)
        assert all((b[i, 0] == 1 or npts == 1) and (b[i, -1] == e["n"] // 2 - 1 or npts == 1) for i, e in enumerate(els))
        assert npts > 1 or (b[0, 0] == 1 and b[1, 0] == 31)
        assert all(np.all((b[i] >= 1) & (b[i] <= e["n"] // 2 - 1)) for i, e in enumerate(els))
    assert list(K.gather_bins(479, True)[0, 1:5]) == [0, -5, 16, 1 << 30]
    assert all(e["n"] <= 4096 for e in K.sparse_elements()) and len(K.sparse_elements()) == 9


# ----------------------------------------------------------------------------------- the restatements against the chain
@pytest.mark.parametrize("length,p,seed,floor_db", [(100, 3, 1, -120.0), (257, 40, 2, -60.0), (1000, 0, 3, -120.0)])
def test_restatements_agree_with_the_float64_chain(length, p, seed, floor_db):
    """G, the wrapped excess phase and M (through minimum_phase_ir) of minphase_ref.chain against the long-double
    restatements evaluated on the chain's own X, T and G.  NumPy's ln, arctan2, exp, sin and cos are within an ulp, so
    the chain lies within the bounds the device is held to; the response within the inverse transform's rounding,
    64 u log2(N) max |h|, plus (2/N) sum |dM|."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(length) * np.exp(-np.arange(length) / (length / 5.0))).astype(np.float32)
    x[p] = -4.0 if seed == 2 else 4.0
    d, n = R.sizes(length, p, 48000)
    ref = R.chain(x, p, d, n, floor_db)
    g, P, count = K.logmag(ref["X"], floor_db)
    assert P == ref["P"] and count == int(ref["floored"].sum())
    K.check_logmag(ref["G"] + 0j, ref["P"], count, ref["X"], floor_db, "chain G")
    ratio, near, _ = K.check_excess(ref["wrapped"], ref["X"], ref["T"], p, n, True, "chain wrapped")
    assert ratio <= 1.0
    re, im, mag = K.spectrum(ref["G"] + 0j, ref["T"])
    M = re.astype(np.float64) + 1j * im.astype(np.float64)
    h = np.fft.irfft(M, n=n)[:d]
    want = R.minimum_phase_ir(ref)
    tol = 64.0 * K.U * math.log2(n) * float(np.max(np.abs(want))) + (2.0 / n) * 2.0 * K.SPEC_C * K.U * float(np.sum(mag))
    assert np.max(np.abs(h - want)) <= tol
