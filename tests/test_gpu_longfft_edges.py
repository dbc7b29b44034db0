"""GPU: the long-FFT kernels (ira_fftsmooth.hip, ira_fftlong.hip, the planning in engine_plan.py) against the long-double
restatement tests/longfft_ref.py at small lengths and argument edges, with the bounds derived there: every direct length
64..8192 and the plan extremes, every small Bluestein length and every convolution-size boundary, padding / window / offset
edges, batch invariance, exact zeros, and the band inverses at their edges (one-bin bands, bin 0, Nyquist, the narrow /
dense switch, the smallest half-length inverse, output guards, tile energies).

Assertions per element: ||X_dev - X||_2 <= the probabilistic bound (primary) and <= the rigorous one, every bin's error <=
the rigorous 2-norm bound, Im X[0] == 0.0 and (even L) Im X[L/2] == 0.0.  The worst error / bound ratio of every path and
family is printed when the module finishes (LONGFFT-RATIO lines; recorded in DESIGN.md)."""
import contextlib

import numpy as np
import pytest

import longfft_ref as R
import spectrum_ref as S

pytestmark = pytest.mark.gpu
LD = np.longdouble
RATIOS = {}
SWITCH_DEFAULTS = dict(half_real_ffts=True, fuse_half_split=True, pair_across_channels=False, three_pow2_sizes=True)


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


@contextlib.contextmanager
def switches(eng, **kw):
    old = {k: getattr(eng, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(eng, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(eng, k, v)


@pytest.fixture(scope="module", autouse=True)
def _print_ratios():
    yield
    for key in sorted(RATIOS):
        r = RATIOS[key]
        print(f"LONGFFT-RATIO {key[0]:28s} {key[1]:12s} worst error/bound: probabilistic {r[0]:.4f} rigorous {r[1]:.5f} "
              f"per-bin {r[2]:.5f}  ({r[3]})")


def _norm(a):
    return float(np.sqrt(np.sum(np.asarray(a, dtype=np.float64) ** 2)))


def _c(re, im):
    return np.asarray(re, dtype=np.float64) + 1j * np.asarray(im, dtype=np.float64)


class Elements:
    """Rows of float32 samples laid out in ONE buffer at arbitrary sample offsets (each row is followed by `gap` samples of
    its own continuation, so that a kernel reading past data_len would see non-zero data), and the per-element arguments."""

    def __init__(self):
        self.rows, self.L, self.d, self.w, self.names, self.tags = [], [], [], [], [], []

    def add(self, names, x, L, d=None, w=None, tag=None):
        for nm, row in zip(names, x):
            self.rows.append(np.asarray(row, dtype=np.float32))
            self.L.append(L); self.d.append(L if d is None else d); self.w.append(L if w is None else w)
            self.names.append(nm); self.tags.append(tag)

    def layout(self, pad=1):
        sizes = np.array([r.size + pad for r in self.rows], dtype=np.int64)
        off = np.cumsum(sizes) - sizes
        flat = np.full(int(sizes.sum()) + 8, 0.5, dtype=np.float32)
        for r, o in zip(self.rows, off):
            flat[o : o + r.size] = r
        return flat, off


def planned_paths(eng, off, lens, data_len=None, win_len=None, packed_ok=False):
    """What the engine's planner does with this call under the engine's switches AS THEY STAND (the very call _rfft_any makes:
    plan_rfft with eng._switches() and eng.smooth_split): per element (family, kind, size), and the number of launches."""
    from audio_analysis_amd.engine_plan import SMOOTH, plan_rfft
    _, launches, _ = plan_rfft(np.asarray(off, np.int64), np.asarray(lens, np.int32), data_len, win_len, packed_ok,
                               eng._switches(), eng.smooth_split)
    paths = [None] * len(lens)
    for ln in launches:
        for j, e in enumerate(ln.jobs):
            if ln.family == SMOOTH:
                kind = ("half_fused" if ln.tables["x2"] is None else "half_split") if ln.half else "full"
            else:
                il = ln.tables["il"]
                kind = "half" if (il is not None and il[j]) else ("pair" if ln.partner[j] >= 0 else "single")
            paths[int(e)] = (ln.family, kind, ln.size)
            if ln.partner[j] >= 0:
                paths[int(ln.partner[j])] = (ln.family, kind, ln.size)
    return paths, len(launches)


def run_forward(eng, el, hann, padded=False, packed=False, flat_off=None):
    flat, off = el.layout() if flat_off is None else flat_off
    x = eng.to_dev(flat)
    lens = np.array(el.L, np.int32)
    el.planned, _ = planned_paths(eng, off, lens, np.array(el.d, np.int32) if padded else None,
                                  np.array(el.w, np.int32) if padded else None, packed)
    if packed:
        spec, so, pk = eng.rfft_any_packed(x, off, lens, hann)
    else:
        kw = dict(data_len=np.array(el.d, np.int32), win_len=np.array(el.w, np.int32)) if padded else {}
        spec, so = eng.rfft_any(x, off, lens, hann, **kw)
        pk = None
    h = spec.cpu().numpy().reshape(-1, 2)
    out = [h[o : o + L // 2 + 1, 0] + 1j * h[o : o + L // 2 + 1, 1] for o, L in zip(so, el.L)]
    return (out, pk) if packed else out


_REF_CACHE = {}


def reference(key, rows, L, d, w, hann, cache=True):
    """(re, im, vnorm, xnorm) per row, computed once per key and left unchanged."""
    k = (key, L, d, w, hann, hash(b"".join(np.ascontiguousarray(r).tobytes() for r in rows)))
    if not cache:
        _REF_CACHE.pop(k, None)
    if k not in _REF_CACHE:
        x = np.stack([np.pad(r, (0, max(0, L - r.size)))[: max(L, 1)] if r.size < L else r for r in rows])
        re, im = R.rfft_ref(x, L, data_len=d, win_len=w, hann=hann)
        v, xs = R.windowed_input(x, L, d, w, hann)
        _REF_CACHE[k] = (re, im, [_norm(r) for r in v], [_norm(r) for r in xs])
    return _REF_CACHE[k] if cache else _REF_CACHE.pop(k)


def check_element(got, re, im, vnorm, xnorm, L, hann, d, w, label, name, pair_norms=None, padded=False, planned=None,
                  **sw):
    """One element against its reference and bounds; records the ratios under (label and path, family).  planned: what
    the engine's planner did with the element (planned_paths) -- the bound is that of the path the element TOOK."""
    flags = dict(SWITCH_DEFAULTS); flags.update(sw)
    path = R.predict_path(L, padded=padded, paired=pair_norms is not None, **flags)
    if planned is not None:
        assert planned == path, (label, name, L, "the planner took", planned, "the restatement predicts", path)
    vn, xn = pair_norms if (pair_norms is not None and path[1] == "pair") else (vnorm, xnorm)
    if path[0] == "smooth":
        prob, rig = R.direct_bound(L, path[1], vn, xn, hann, d, w)
    else:
        prob, rig = R.bluestein_bound(L, path[1], path[2], vn, xn, hann, d, w)
    ref = _c(re, im)
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got.real)) and np.all(np.isfinite(got.imag)), (label, name, L)
    assert got[0].imag == 0.0 and (L % 2 or got[-1].imag == 0.0), (label, name, L, got[0], got[-1])
    err = np.abs(got - ref)
    e2 = float(np.sqrt(np.sum(err ** 2)))
    what = (label, name, L, hann, d, w, path)
    if xn == 0.0:
        assert np.all(got == 0.0), what                        # all-zero input: exactly 0 in every bin
        return path
    assert e2 <= prob, (what, "2-norm", e2, prob, e2 / prob)
    assert e2 <= rig and float(err.max()) <= rig, (what, "rigorous", e2, float(err.max()), rig)
    key = (f"{label} {path[0]} {path[1]}", name.split()[0])
    r = RATIOS.setdefault(key, [0.0, 0.0, 0.0, ""])
    if e2 / prob > r[0]:
        r[3] = f"L={L} hann={hann}"
    r[0], r[1], r[2] = max(r[0], e2 / prob), max(r[1], e2 / rig), max(r[2], float(err.max()) / rig)
    return path


def thread_run(L):
    """Index of a thread's second window-rotation step in the Bluestein column pass: (256 / C) * N2 of the element's M."""
    path = R.predict_path(L)
    if path[0] != "bluestein":
        return None
    _, n1, n2, C = R.bluestein_geometry(path[2])
    run = (256 // C) * n2
    return run if run < L else None


# ================================================================================================ forward: direct lengths
def _direct_inputs(L, **kw):
    """The families of a direct length: impulses also at the first / last index of the second column of the transform that
    runs (n2, n2 - 1 of a full-length job; samples 2 n2 - 1, 2 n2 of a half-length job, whose element m is x[2m] + i x[2m+1])."""
    n2 = R.smooth_split_py(L)[1]
    half = R.predict_path(L)[1] != "full"
    return R.make_inputs(L, n2=n2, run=2 * R.smooth_split_py(L // 2)[1] if half else None, **kw)


DIRECT = R.direct_lengths()
DIRECT_CHUNKS = [DIRECT[i::4] for i in range(4)]


@pytest.mark.parametrize("hann", [False, True])
@pytest.mark.parametrize("chunk", range(4))
def test_every_direct_length_64_to_8192(chunk, hann):
    """Every n = 2^a 3^b 5^c in [64, 8192], all five families in one batch per length: the default switches, and every even
    length again with fuse_half_split = False and with half_real_ffts = False -- each against the reference."""
    eng = _eng()
    kinds = set()
    lengths = DIRECT_CHUNKS[chunk]
    el = Elements()
    for L in lengths:
        split = eng.smooth_split(L)
        assert split == R.smooth_split_py(L), (L, split, R.smooth_split_py(L))
        el.add(*_direct_inputs(L), L)
    layout = el.layout()
    variants = [dict(), dict(fuse_half_split=False), dict(half_real_ffts=False)]
    for sw in variants:
        with switches(eng, **sw):
            got = run_forward(eng, el, hann, flat_off=layout)
        i = 0
        for L in lengths:
            names, x = _direct_inputs(L)
            re, im, vn, xn = reference("direct", list(x), L, L, L, hann)
            for j, nm in enumerate(names):
                if not sw or L % 2 == 0:
                    check_element(got[i], re[j], im[j], vn[j], xn[j], L, hann, L, L, "direct", nm, planned=el.planned[i], **sw)
                    kinds.add(el.planned[i][1])                   # what the planner did under these switches
                i += 1
    assert kinds == {"half_fused", "half_split", "full"}, kinds       # the switches reached all three variants


@pytest.mark.parametrize("L", R.PLAN_EXTREMES)
def test_direct_plan_extremes(L):
    """3^12, 5^8, 2^20, 1024 * 1000, 729 * 720: the longest radix chains and the largest sub-transforms; impulses and noise,
    with and without the window (one reference transform per length: the impulses are closed forms)."""
    eng = _eng()
    split = eng.smooth_split(L)
    assert split == R.smooth_split_py(L)
    names, x = _direct_inputs(L, families=("impulse", "noise"))
    el = Elements()
    el.add(names, x, L)
    layout = el.layout()
    for hann in (False, True):
        got = run_forward(eng, el, hann, flat_off=layout)
        re, im, vn, xn = reference("extreme", list(x), L, L, L, hann, cache=False)
        for j, nm in enumerate(names):
            check_element(got[j], re[j], im[j], vn[j], xn[j], L, hann, L, L, "extreme", nm, planned=el.planned[j])


# ================================================================================================ forward: Bluestein
BLUE = R.bluestein_lengths()
BLUE_SMALL = [L for L in BLUE if L <= 320]
BLUE_EDGE = [L for L in BLUE if L > 320]


def _bluestein_sweep(lengths, hann, three, families, label):
    eng = _eng()
    el = Elements()
    inputs = {}
    for L in lengths:
        inputs[L] = R.make_inputs(L, run=thread_run(L), families=families)
        el.add(*inputs[L], L)
    with switches(eng, three_pow2_sizes=three):
        got = run_forward(eng, el, hann)
    kinds, i = set(), 0
    for L in lengths:
        names, x = inputs[L]
        re, im, vn, xn = reference(label, list(x), L, L, L, hann)
        for j, nm in enumerate(names):
            path = check_element(got[i], re[j], im[j], vn[j], xn[j], L, hann, L, L, label, nm, planned=el.planned[i],
                                 three_pow2_sizes=three)
            kinds.add(path[1])
            i += 1
    return kinds


@pytest.mark.parametrize("three", [True, False])
@pytest.mark.parametrize("hann", [False, True])
def test_every_small_bluestein_length(hann, three):
    """Every L in [1, 320] without a direct transform: odd single jobs, even half jobs from L = 8, even L in {2, 4, 6} below
    that rule; M = 2^k and 3 * 2^k."""
    assert {2, 4, 6, 7, 14, 97, 194}.issubset(BLUE_SMALL)
    kinds = _bluestein_sweep(BLUE_SMALL, hann, three, R.FAMILY_NAMES, "small")
    assert kinds == {"single", "half"}
    for L in (2, 4, 6):
        assert R.predict_path(L)[1] == "single"


@pytest.mark.parametrize("three", [True, False])
@pytest.mark.parametrize("hann", [False, True])
def test_bluestein_lengths_at_every_size_boundary(hann, three):
    """Every non-direct L within +-2 of a boundary of conv_size (L + L // 2 and 2 l - 1) up to M = 3 * 2^13."""
    _bluestein_sweep(BLUE_EDGE, hann, three, ("impulse", "noise"), "boundary")


@pytest.mark.parametrize("hann", [False, True])
def test_bluestein_pairs_across_channels(hann):
    """pair_across_channels = True with two and with three equal-length channels (one pair and one left over)."""
    eng = _eng()
    for L in (7, 97, 194, 683, 2 * 683 + 1):
        for count in (2, 3):
            names, x = R.make_inputs(L, families=("noise", "alternating", "constant"))
            x = x[:count] * np.array([1.0, 1e-3, 0.3], np.float32)[:count, None]      # very different levels on purpose
            el = Elements()
            el.add(names[:count], x, L)
            with switches(eng, pair_across_channels=True):
                got = run_forward(eng, el, hann)
            re, im, vn, xn = reference(("pairs", count), list(x), L, L, L, hann)
            pair_norms = (float(np.hypot(vn[0], vn[1])), float(np.hypot(xn[0], xn[1])))
            for j in range(count):
                check_element(got[j], re[j], im[j], vn[j], xn[j], L, hann, L, L, "pairs", names[j], planned=el.planned[j],
                              pair_norms=pair_norms if j < 2 else None, pair_across_channels=True)


def test_bluestein_packed_spectra_through_mag_phase():
    """rfft_any_packed leaves even Bluestein lengths packed; untangled in long double they are the reference's bins within
    the half job's bound, and ira_spectrum_mag_phase's dB and angle of them hold that kernel's own bounds."""
    from test_gpu_spectrum import check_mag_phase
    eng = _eng()
    lengths = [14, 194, 254, 2 * 683, 97]
    el = Elements()
    inputs = {}
    for L in lengths:
        inputs[L] = R.make_inputs(L, families=("noise",))       # (well-conditioned bins: the dB / angle bounds assume them)
        el.add(*inputs[L], L)
    flat, off = el.layout()
    x = eng.to_dev(flat)
    lens = np.array(el.L, np.int32)
    spec, so, pk = eng.rfft_any_packed(x, off, lens, True)
    assert pk is not None and list(pk) == [0 if L % 2 else 1 for L in el.L]
    mag, ph = eng.spectrum_mag_phase(spec, so, lens, -120.0, want_phase=True, packed=pk)
    h = spec.cpu().numpy().reshape(-1, 2)
    mag, ph = mag.cpu().numpy(), ph.cpu().numpy()
    i = 0
    for L in lengths:
        names, xr = inputs[L]
        re, im, vn, xn = reference("packed", list(xr), L, L, L, True)
        for j, nm in enumerate(names):
            o, nb = int(so[i]), L // 2 + 1
            z = h[o : o + nb, 0] + 1j * h[o : o + nb, 1]
            if pk[i]:
                ur, ui, _, _ = S.packed_bins_ld(z[: L // 2], L)
                got = _c(ur, ui)
            else:
                got = z
            check_element(got, re[j], im[j], vn[j], xn[j], L, True, L, L, "packed", nm)
            r = S.mag_db_phase(z[: L // 2] if pk[i] else z, L, -120.0, packed=bool(pk[i]))
            check_mag_phase(mag[o : o + nb], ph[o : o + nb], r, f"edges packed={pk[i]} L {L} {nm}", packed=bool(pk[i]))
            i += 1


# ================================================================================================ padding and windows
PAD_LENGTHS = [360, 450, 225, 194, 97]        # direct: half fused, half split, odd full; Bluestein: even, odd


@pytest.mark.parametrize("L", PAD_LENGTHS)
@pytest.mark.parametrize("hann", [False, True])
def test_padding_truncation_and_window_lengths(L, hann):
    """numpy.fft.rfft(x[:d] * hanning(w)[:d], n=L) for d in {0, 1, 2, L-1, L, L+1, 2L} and w in {1, 2, 3, d-1, d, d+1, 2d}
    (w >= 1).  d > L truncates; w < d continues the window's cosine (the documented choice); hanning(1) = 1 and
    hanning(2) = [0, 0] give no NaN; an all-zero input gives exactly 0 in every bin."""
    eng = _eng()
    names, x = R.make_inputs(2 * L, families=("noise", "constant"))     # 2 L samples: what lies past d is NOT zero
    names = names + ["zeros"]
    x = np.concatenate([x, np.zeros((1, 2 * L), np.float32)])
    combos = []
    for d in (0, 1, 2, L - 1, L, L + 1, 2 * L):
        for w in sorted({1, 2, 3, d - 1, d, d + 1, 2 * d}):
            if w >= 1 and (hann or w == max(d, 1)):
                combos.append((d, w))
    el = Elements()
    for d, w in combos:
        el.add(names, x, L, d, w)
    got = run_forward(eng, el, hann, padded=True)
    i = 0
    for d, w in combos:
        re, im, vn, xn = reference(("pad", L), list(x), L, d, w, hann)
        for j, nm in enumerate(names):
            check_element(got[i], re[j], im[j], vn[j], xn[j], L, hann, d, w, "padded", nm, padded=True, planned=el.planned[i])
            i += 1


# ================================================================================================ offsets and batches
@pytest.mark.parametrize("hann", [False, True])
def test_sample_offsets_and_overlapping_elements(hann):
    """Sample offsets = 0, 1, 2, 3 mod 4 and elements that overlap in x: the same samples, the same reference."""
    eng = _eng()
    rng = np.random.default_rng(77)
    base = (rng.standard_normal(9000) * np.exp(-np.arange(9000) / 3000.0)).astype(np.float32)
    x = eng.to_dev(base)
    lengths = [360, 450, 225, 194, 97, 4099, 4800]
    offs, lens = [], []
    for L in lengths:
        for o in (0, 1, 2, 3, 5, 130):                            # every residue mod 4, all overlapping one another
            offs.append(o); lens.append(L)
    spec, so = eng.rfft_any(x, np.array(offs, np.int64), np.array(lens, np.int32), hann)
    h = spec.cpu().numpy().reshape(-1, 2)
    for o, L, s in zip(offs, lens, so):
        re, im, vn, xn = reference(("offset", o), [base[o : o + L]], L, L, L, hann)
        got = h[s : s + L // 2 + 1, 0] + 1j * h[s : s + L // 2 + 1, 1]
        check_element(got, re[0], im[0], vn[0], xn[0], L, hann, L, L, "offsets", "noise")


def test_an_element_alone_and_in_a_ragged_batch_gives_the_same_bytes():
    """One element alone, inside a ragged batch of 40 mixed lengths, and inside the same batch cut into several launches by
    a small workspace budget: the same bytes (default switches: no element shares a transform with another channel)."""
    eng = _eng()
    rng = np.random.default_rng(78)
    lengths = [4800, 4099, 360, 194, 97, 8192, 450, 225, 2 * 683, 683] * 4
    rows = [(rng.standard_normal(L) * np.exp(-np.arange(L) / 2000.0)).astype(np.float32) for L in lengths]
    b = eng.upload(rows)
    lens = np.array(lengths, np.int32)
    for hann in (False, True):
        spec, so = eng.rfft_any(b.x, b.off, lens, hann)
        h = spec.cpu().numpy().reshape(-1, 2)
        _, whole = planned_paths(eng, b.off, lens)
        with switches(eng, workspace_budget_bytes=1):              # no two jobs fit one launch
            _, cut = planned_paths(eng, b.off, lens)
            spec2, so2 = eng.rfft_any(b.x, b.off, lens, hann)
        assert whole == 10 and cut == 40, (whole, cut)             # one launch per length -> one per element
        assert np.array_equal(so, so2) and spec2.cpu().numpy().tobytes() == h.tobytes()
        for e in range(10):                                       # every distinct length once
            s1, o1 = eng.rfft_any(b.x, b.off[e : e + 1], lens[e : e + 1], hann)
            nb = lengths[e] // 2 + 1
            assert s1.cpu().numpy()[: 2 * nb].tobytes() == h[so[e] : so[e] + nb].tobytes(), (lengths[e], hann)


# ================================================================================================ band inverses
def _mask_values(eng, rec, fv, nbins):
    from audio_analysis_amd import _lib
    out = eng.empty(nbins, eng.torch.float32)
    assert eng.lib.ira_band_mask_values(_lib.dbl_array(list(rec)), float(fv), nbins, int(out.data_ptr()), eng.stream) == 0
    return out.cpu().numpy()


def _rec(kind, hp=(0.0, 0.0), lp=(0.0, 0.0)):
    return np.array([kind, hp[0], hp[1], lp[0], lp[1], 0, 0, 0], dtype=np.float64)


def _one_bin(k):
    return _rec(3.0, (k - 0.75, k - 0.25), (k + 0.25, k + 0.75))


def edge_bands(n):
    """(name, record) on the axis f(k) = k (bin step 1): bin 0 alone, one-bin bands, the Nyquist high-pass, everything."""
    nb = n // 2 + 1
    out = [("lowpass bin 0 alone", _rec(1.0, lp=(0.25, 0.75))),
           ("one bin k=1", _one_bin(1)), ("one bin centre", _one_bin(nb // 2)),
           ("highpass to the last bin", _rec(2.0, hp=(nb - 5.5, nb - 2.5))),
           ("allpass", _rec(1.0, lp=(float(n), float(n + 1)))),
           ("bandpass wide", _rec(3.0, (1.5, 3.5), (0.3 * nb, 0.45 * nb)))]
    if n % 2 == 0:
        out.append(("one bin Nyquist", _one_bin(n // 2)))
    # coinciding edges (x0 == x1: the ramp is the step f >= x1, and every bin takes the full formula -- what the band
    # tables give for the top band of a 44.1 kHz recording, tests/test_gpu_rates.py): the low-pass side of a band-pass at
    # the last bin and at an interior one, a high-pass, and a low-pass with both edges at bin 0 (nothing passes)
    out += [("coincide lowpass edges at the last bin", _rec(3.0, (1.5, 3.5), (float(nb - 1), float(nb - 1)))),
            ("coincide lowpass edges inside", _rec(3.0, (1.5, 3.5), (float(nb // 3), float(nb // 3)))),
            ("coincide highpass edges", _rec(2.0, hp=(float(nb // 3), float(nb // 3)))),
            ("coincide lowpass edges at bin 0", _rec(1.0, lp=(0.0, 0.0)))]
    return out


def run_bands(eng, spec_dev, spec_off, n, recs, fvs, gap=7, sentinel=-777.25, tiles=False):
    """band_irfft of len(recs) entries into a sentinel-filled y with a gap after each signal; returns (signals, result)."""
    t = eng.torch
    nbands = len(recs)
    y = eng.empty(nbands * (n + gap) + gap, t.float32)
    y.fill_(sentinel)
    yoff = gap + np.arange(nbands, dtype=np.int64) * (n + gap)
    res = eng.band_irfft(spec_dev, np.asarray(spec_off, np.int64), np.full(nbands, n, np.int32), np.stack(recs),
                         np.asarray(fvs, np.float64), y, yoff, want_tiles=tiles)
    h = y.cpu().numpy()
    keep = np.ones(h.size, dtype=bool)
    for o in yoff:
        keep[o : o + n] = False
    assert np.all(h[keep] == np.float32(sentinel)), "a band inverse wrote outside its signal"
    return [h[o : o + n].copy() for o in yoff], res


_BAND_REF = {}


def masked_norm(X, mask, n):
    return _norm(np.abs(np.asarray(X)[: n // 2 + 1]) * mask.astype(np.float64))


def partner_norms(j1, j2, norms):
    """Per entry: the masked-spectrum norm of the entry it shares a transform with (0: none), and whether it has one."""
    out, paired = np.zeros(len(norms)), np.zeros(len(norms), dtype=bool)
    for a, b in zip(j1, j2):
        if b >= 0:
            out[a], out[b] = norms[b], norms[a]
            paired[a] = paired[b] = True
    return out, paired


def check_band(got, X, mask, n, paired, label, name, partner_norm=0.0, **sw):
    """One band signal against irfft_masked_ref and band_bound.  partner_norm: ||X2 mask2||_2 of the band that shares the
    complex transform (y1 + i y2): the float64 term is that of the transform, i.e. of both."""
    fam, kind, size = R.predict_inverse_path(n, paired, **sw)
    key = (n, hash(np.asarray(X).tobytes()), hash(mask.tobytes()))
    if key not in _BAND_REF:
        _BAND_REF[key] = R.irfft_masked_ref(X, mask, n)
    y = _BAND_REF[key]
    xm = float(np.hypot(masked_norm(X, mask, n), partner_norm))
    bound, t = R.band_bound(y, xm, n, fam, kind, size)
    assert np.all(np.isfinite(got)), (label, name, n)
    err = np.abs(got.astype(LD) - y).astype(np.float64)
    k = int(np.argmax(err / bound))
    assert err[k] <= bound[k], (label, name, n, (fam, kind, size), k, err[k], bound[k], float(t))
    # the float64 part alone: how much of the float64 term the device uses where the float32 rounding does not hide it
    r = RATIOS.setdefault((f"inverse {label} {fam} {kind}", name.split()[0].rstrip("0123456789")), [0.0, 0.0, 0.0, ""])
    ratio = float(err[k] / bound[k])
    if ratio > r[0]:
        r[3] = f"n={n} {name}"
    r[0] = r[1] = r[2] = max(r[0], ratio)


BAND_LENGTHS = [64, 128, 130, 4800, 28800, 97, 194, 23257]
TILE_N2 = min(n for n in range(4097, 4400) if R.is_direct(n))


@pytest.mark.parametrize("n", BAND_LENGTHS)
def test_band_inverse_edges(n):
    """Direct 64, 128 (the first half-length inverse), 130 (its half is not smooth), 4800, 28800; Bluestein 97, 194, 23257:
    the device's own spectrum of a noise signal and hand-made one-bin spectra (exact cosines) through bin-0, one-bin,
    Nyquist, all-pass and wide bands, as pairs (full-length inverse) and alone (half-length where the length allows),
    sparse_bands on and off, guards around every output."""
    eng = _eng()
    nb = n // 2 + 1
    names, x = R.make_inputs(n, families=("noise",))
    b = eng.upload([x[0]])
    spec, so = eng.rfft_any(b.x, b.off, np.array([n], np.int32), False)
    Xdev = spec.cpu().numpy().reshape(-1, 2)
    Xdev = Xdev[:nb, 0] + 1j * Xdev[:nb, 1]
    bands = edge_bands(n)
    masks = [_mask_values(eng, rec, 1.0, nb) for _, rec in bands]
    assert np.count_nonzero(masks[0]) == 1 and masks[0][0] == 1.0
    assert np.count_nonzero(masks[1]) == 1 and masks[1][1] == 1.0
    assert masks[3][-1] == 1.0 and 0.0 < masks[3][-3] < 1.0 and np.all(masks[4] == 1.0)
    by_name = {name: m for (name, _), m in zip(bands, masks)}
    k = nb // 3
    m = by_name["coincide lowpass edges at the last bin"]
    assert m[-1] == 0.0 and np.all(m[4:-1] == 1.0) and np.all(m[:2] == 0.0)              # the step f >= x1 cuts the edge bin
    m = by_name["coincide lowpass edges inside"]
    assert np.all(m[k:] == 0.0) and np.all(m[4:k] == 1.0)
    m = by_name["coincide highpass edges"]
    assert np.all(m[:k] == 0.0) and np.all(m[k:] == 1.0)
    assert np.all(by_name["coincide lowpass edges at bin 0"] == 0.0)
    # hand-made spectra: one non-zero bin each, at 0, 1, a band's first / centre / last bin and the last bin
    hand = []
    for k in sorted({0, 1, 2, nb // 2, int(0.45 * nb), nb - 1}):
        z = np.zeros(nb, np.complex128)
        z[k] = (3.0 - 2.0j) if 0 < k < nb - 1 or (k == nb - 1 and n % 2) else 3.0
        hand.append((f"bin{k}", z))
    spectra = [("noise", Xdev)] + hand
    allspec = np.concatenate([z for _, z in spectra])
    d_spec = eng.to_dev(allspec.view(np.float64))
    offs = np.arange(len(spectra), dtype=np.int64) * nb
    for sparse in (True, False):
        with switches(eng, sparse_bands=sparse):
            # pairs: every spectrum with all its bands in one call (an odd band count leaves the narrowest alone)
            recs = [rec for _ in spectra for _, rec in bands]
            so_all = np.repeat(offs, len(bands))
            got, _ = run_bands(eng, d_spec, so_all, n, recs, np.ones(len(recs)))
            from audio_analysis_amd.engine_plan import band_pairs
            j1, j2 = band_pairs(so_all, np.full(len(recs), n, np.int32), np.stack(recs), np.ones(len(recs)), eng._switches())
            norms = [masked_norm(z, m, n) for _, z in spectra for m in masks]
            pn, paired = partner_norms(j1, j2, norms)
            i = 0
            for sname, z in spectra:
                for (bname, _), m in zip(bands, masks):
                    check_band(got[i], z, m, n, bool(paired[i]), f"sparse={int(sparse)}", f"{sname} {bname}", pn[i])
                    i += 1
            # alone: one band per call (the half-length inverse where n allows it)
            for (bname, rec), m in zip(bands, masks):
                got1, _ = run_bands(eng, d_spec, offs[:1], n, [rec], [1.0])
                check_band(got1[0], Xdev, m, n, False, f"sparse={int(sparse)}", f"noise-alone {bname}")


def test_band_inverse_ignores_imaginary_parts_of_bin_0_and_nyquist():
    """numpy.fft.irfft ignores Im X[0] and (even n) Im X[n/2]; so do the inverses: hand-made spectra that have both, through
    the full-length pair inverse, the half-length single inverse, the narrow path and Bluestein."""
    eng = _eng()
    for n in (64, 128, 4800, 130, 194, 97):
        nb = n // 2 + 1
        z = np.zeros(nb, np.complex128)
        z[0], z[3], z[-1] = 2.0 + 0.5j, 1.0 - 1.0j, 1.5 - 0.75j
        d_spec = eng.to_dev(z.view(np.float64))
        bands = [("allpass", _rec(1.0, lp=(float(n), float(n + 1)))), ("lowpass bin 0 alone", _rec(1.0, lp=(0.25, 0.75))),
                 ("highpass to the last bin", _rec(2.0, hp=(nb - 5.5, nb - 2.5)))]
        masks = [_mask_values(eng, rec, 1.0, nb) for _, rec in bands]
        for sparse in (True, False):
            with switches(eng, sparse_bands=sparse):
                got, _ = run_bands(eng, d_spec, np.zeros(2, np.int64), n, [bands[0][1], bands[2][1]], np.ones(2))
                check_band(got[0], z, masks[0], n, True, "imag", "handmade allpass", masked_norm(z, masks[2], n))
                check_band(got[1], z, masks[2], n, True, "imag", "handmade highpass", masked_norm(z, masks[0], n))
                for (bname, rec), m in zip(bands, masks):
                    got1, _ = run_bands(eng, d_spec, np.zeros(1, np.int64), n, [rec], [1.0])
                    check_band(got1[0], z, m, n, False, "imag", f"handmade-alone {bname}")


def test_third_octave_bands_paired_and_single():
    """The RT60 bank's own third-octave masks (band_mask_record, bin step 48000 / n) on 4800 and 28800 samples and on the
    Bluestein length 23257: pairs through the full-length inverse, the band left over through the half-length one."""
    from audio_analysis_amd.analyse import rt60bands as rb
    from audio_analysis_amd.analyse.frequency_response import rfft_bin_step
    eng = _eng()
    st = rb.Rt60BandsAnalysisSettings(band_mode="third")
    third = rb._build_band_definitions(st, 48000)
    for n, sel in ((4800, third[8::3]), (28800, third[3::4]), (23257, third[5::6])):
        sel = sel[: len(sel) - (1 - len(sel) % 2)]                # an odd count: one band is left over
        nb = n // 2 + 1
        names, x = R.make_inputs(n, families=("noise",))
        b = eng.upload([x[0]])
        spec, so = eng.rfft_any(b.x, b.off, np.array([n], np.int32), False)
        X = spec.cpu().numpy().reshape(-1, 2)
        X = X[:nb, 0] + 1j * X[:nb, 1]
        fv = rfft_bin_step(n, 48000)
        recs = [rb.band_mask_record(bd, st.transition_width_octaves, 24000.0) for bd in sel]
        got, _ = run_bands(eng, spec, np.full(len(recs), so[0], np.int64), n, recs, np.full(len(recs), fv))
        from audio_analysis_amd.engine_plan import band_pairs
        j1, j2 = band_pairs(np.zeros(len(recs), np.int64), np.full(len(recs), n, np.int32), np.stack(recs),
                            np.full(len(recs), fv), eng._switches())
        assert (j2 < 0).sum() == 1
        mks = [_mask_values(eng, rec, fv, nb) for rec in recs]
        pn, paired = partner_norms(j1, j2, [masked_norm(X, m, n) for m in mks])
        if n != 23257:
            assert len(eng.last_band_info_half) == 2 and sorted(eng.last_band_info_half) == [False, True]
        for i, (bd, rec) in enumerate(zip(sel, recs)):
            check_band(got[i], X, mks[i], n, bool(paired[i]), "third", f"noise {bd.name}", pn[i])


def test_hulls_on_either_side_of_the_narrow_band_switch():
    """n = 4800, sparse_q = 9.  Alone (half-length inverse over 2400 = n1 x n2) a band whose hull spans 9 n2 bins is a narrow
    job and one of 9 n2 + 1 bins a dense one; as a pair (full length 4800) the switch is at 9 n2 / 9 n2 + 1 bins of the
    pair's common hull, n2 that of 4800.  last_band_info shows exactly that, and both sides hold the bound."""
    eng = _eng()
    n, nb = 4800, 2401
    n2h, n2f = eng.smooth_split(2400)[1], eng.smooth_split(4800)[1]
    assert (n2h, n2f) == (R.smooth_split_py(2400)[1], R.smooth_split_py(4800)[1])
    names, x = R.make_inputs(n, families=("noise",))
    b = eng.upload([x[0]])
    spec, so = eng.rfft_any(b.x, b.off, np.array([n], np.int32), False)
    X = spec.cpu().numpy().reshape(-1, 2)
    X = X[:nb, 0] + 1j * X[:nb, 1]
    hull = lambda lo, w: _rec(3.0, (lo - 0.5, lo + 10.5), (lo + w - 12.5, lo + w - 0.5))     # support exactly [lo, lo + w)
    for lo, w, narrow in ((300, 9 * n2h, 1), (300, 9 * n2h + 1, 0), (1, 9 * n2h, 1)):
        rec = hull(lo, w)
        m = _mask_values(eng, rec, 1.0, nb)
        assert m[lo - 1] == 0.0 and m[lo + w] == 0.0 and m[lo + 1] > 0.0 and m[lo + w - 2] > 0.0
        got, _ = run_bands(eng, spec, so[:1], n, [rec], [1.0])
        info = np.concatenate([i.cpu().numpy().reshape(-1, 4) for i in eng.last_band_info])
        assert eng.last_band_info_half == [True] and info[0].tolist() == [narrow, lo, w, (w + n2h - 1) // n2h], (lo, w, info)
        check_band(got[0], X, m, n, False, "switch", f"noise hull {w} alone")
    for w, narrow in ((9 * n2f, 1), (9 * n2f + 1, 0)):
        recs = [hull(200, 300), hull(200 + w - 300, 300)]          # common hull [200, 200 + w)
        got, _ = run_bands(eng, spec, np.full(2, so[0], np.int64), n, recs, np.ones(2))
        info = np.concatenate([i.cpu().numpy().reshape(-1, 4) for i in eng.last_band_info])
        assert eng.last_band_info_half == [False] and info[0].tolist() == [narrow, 200, w, (w + n2f - 1) // n2f], (w, info)
        mks = [_mask_values(eng, rec, 1.0, nb) for rec in recs]
        for i, g in enumerate(got):
            check_band(g, X, mks[i], n, True, "switch", f"noise hull {w} pair", masked_norm(X, mks[1 - i], n))


@pytest.mark.parametrize("n", [4800, TILE_N2])
def test_tile_energies_at_small_lengths(n):
    """band_tile_energies = True: the partials of the second pass, added up, are the energies of the 4096-sample tiles of
    the float32 signals to 1e-12 relative -- at 4800 and at the first direct length past 4096 (a partial last tile of a few
    samples; 4096 + 64 = 64 * 5 * 13 has no direct transform and leaves no partials), pairs and a single band."""
    from audio_analysis_amd.analyse import rt60bands as rb
    from audio_analysis_amd.analyse.frequency_response import rfft_bin_step
    eng = _eng()
    assert eng.smooth_split(n) is not None
    st = rb.Rt60BandsAnalysisSettings(band_mode="three")
    bands = rb._build_band_definitions(st, 48000)
    names, x = R.make_inputs(n, families=("noise",))
    b = eng.upload([x[0]])
    spec, so = eng.rfft_any(b.x, b.off, np.array([n], np.int32), False)
    fv = rfft_bin_step(n, 48000)
    recs = [rb.band_mask_record(bd, st.transition_width_octaves, 24000.0) for bd in bands]
    with switches(eng, band_tile_energies=True):
        got, tiles = run_bands(eng, spec, np.full(len(recs), so[0], np.int64), n, recs, np.full(len(recs), fv), tiles=True)
    assert tiles is not None
    part, poff, pwgs, ptiles = tiles
    ntile = (n + 4095) // 4096
    assert np.all(poff >= 0) and np.all(pwgs > 0) and np.all(ptiles[: len(recs)] >= ntile)
    ph = part.cpu().numpy()
    for e in range(len(recs)):
        nt = int(ptiles[e])
        have = ph[poff[e] : poff[e] + nt * pwgs[e]].reshape(pwgs[e], nt).sum(axis=0)
        yh = got[e].astype(np.float64)
        want = np.array([np.sum(yh[max(0, n - (j + 1) * 4096) : n - j * 4096] ** 2) for j in range(ntile)])
        assert np.allclose(have[:ntile], want, rtol=1e-12, atol=1e-300), (n, e, have, want)
