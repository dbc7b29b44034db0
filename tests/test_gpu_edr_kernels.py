"""
The two energy-decay-relief kernels alone, called through the C-ABI on guarded buffers the test owns.

ira_edr_power against numpy.fft.rfft of the float64 windowed frames under the derived bound of edr_ref.power_bound (the
largest observed / bound is printed per case): n_fft 256, 2048, 4096 and 8192 (the smallest, and one per instantiation), hops
n_fft, n_fft / 4, 37 and 1, T = 1, 2, 3, 15, 16, 17, 31, 32, 33 frames (odd counts, both sides of a chunk edge), rows that are
empty, one bin, hold DC, hold the Nyquist bin, cover every bin, and sit on either side of the serial / wavefront threshold,
nrows 1 and 256 (at 8192 points 256 rows stage half a chunk per store).  Every case puts NaN straight after each segment's
last frame, checks the padding columns and the guard words.  Silent frames are exact zeros; a segment's bytes do not depend on
the batch.

ira_edr_integrate on host-made P (values over 1e-200 .. 1e200, exact small integers, zeros, a NaN and an infinity at chosen
frames; NaN in the padding columns, which are never read): S, N and the record equal the NumPy restatement bit for bit (any
NaN equals any NaN: the payload of an invalid operation differs between the two machines), the float32 curve is within the
table logarithm's allowance on the device's own S.  T = 1, 2, 63, 64, 65, 127, 128, 129, 1000; q = 0, 1, 7, T.
"""
import functools

import numpy as np
import pytest

import edr_ref as R
import guard_buffers as GB

pytestmark = pytest.mark.gpu

FRAME_COUNTS = (1, 2, 3, 15, 16, 17, 31, 32, 33)
INTEGRATE_T = (1, 2, 63, 64, 65, 127, 128, 129, 1000)
EPS, FLOOR = 1e-30, -120.0


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def same(a, b):
    """The same bits; a NaN equals any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------------------------------------------------ ira_edr_power
def run_power(segs, n_fft, hop, win_name, first, count, phase=0, poison=True):
    """One ira_edr_power call on guarded buffers -> [P (nrows, Tpad) per segment].  poison: NaN in every sample past a
    segment's last frame and in the element behind the segment."""
    from audio_analysis_amd._lib import check, ptr
    eng = _eng()
    first, count = np.asarray(first, np.int32), np.asarray(count, np.int32)
    nrows = int(first.size)
    lens = [len(s) for s in segs]
    frames = [R.frame_count(n, n_fft, hop) for n in lens]
    fx = GB.Flat(lens, np.float32, phase)
    xbuf = fx.filled(segs)
    if poison:
        for o, n, t in zip(fx.off, lens, frames):
            xbuf[o + ((t - 1) * hop + n_fft if t else 0) : o + n + 1] = np.nan
    fp = GB.Flat([nrows * R.tpad(t) for t in frames], np.float64, phase + 3)
    d_x, d_p = GB.to_device(eng, xbuf), GB.to_device(eng, fp.filled())
    tabs = [GB.to_device(eng, np.asarray(a)) for a in (np.asarray(fx.off, np.int64), np.asarray(lens, np.int64),
                                                        np.asarray(fp.off, np.int64), first, count)]
    win = eng.window(n_fft, win_name == "hann", 64)
    tw = eng.twiddle(n_fft, 64)
    check(eng.lib.ira_edr_power(ptr(d_x), ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), len(segs), max(frames), n_fft, hop, ptr(win),
                                ptr(tw), ptr(tabs[3]), ptr(tabs[4]), nrows, ptr(d_p), eng.stream), "ira_edr_power")
    eng.sync()
    parts = fp.split(d_p.cpu().numpy(), "P")
    return [p.reshape(nrows, R.tpad(t)) for p, t in zip(parts, frames)]


def noise(seed, n):
    """Broadband noise whose level wanders over two decades in blocks of 500 samples: loud frames beside quiet ones."""
    rng = np.random.default_rng(seed)
    level = 10.0 ** rng.uniform(-2.0, 0.0, -(-n // 500))
    return (rng.standard_normal(n) * np.repeat(level, 500)[:n]).astype(np.float32)


def standard_rows(n_fft):
    """empty, one bin, DC, Nyquist, every bin, 16 and 17 bins (the two row-sum paths), an empty row at the end of the bins."""
    half = n_fft // 2
    return (np.array([5, 9, 0, half - 2, 0, 20, 40, half + 1], np.int32), np.array([0, 1, 3, 3, half + 1, 16, 17, 0], np.int32))


def check_power(segs, n_fft, hop, win_name, first, count, what):
    got = run_power(segs, n_fft, hop, win_name, first, count)
    win = R.window(n_fft, win_name)
    worst = 0.0
    for s, g in zip(segs, got):
        fr = R.windowed_frames(s, n_fft, hop, win)
        T = fr.shape[0]
        P, X = R.band_powers(fr, first, count)
        bound = R.power_bound(fr, X, first, count, n_fft)
        assert g.shape[1] == R.tpad(T) and np.all(g[:, T:] == 0.0), (what, "padding columns")
        d = np.abs(g[:, :T].T - P)
        assert np.all(np.isfinite(g)), (what, "NaN past the last frame was read")
        assert np.all(d[bound == 0.0] == 0.0), (what, "a row without bins or energy is exactly 0")
        if np.any(bound > 0.0):
            ratio = d[bound > 0.0] / bound[bound > 0.0]
            worst = max(worst, float(ratio.max()))
    print(f"{what}: observed / bound {worst:.3f}")
    assert worst <= 1.0, (what, worst)
    return worst


@pytest.mark.parametrize("n_fft", [256, 2048, 4096, 8192])
@pytest.mark.parametrize("hop_kind", ["n_fft", "quarter", "37", "1"])
def test_band_powers_within_the_bound(n_fft, hop_kind):
    hop = {"n_fft": n_fft, "quarter": n_fft // 4, "37": 37, "1": 1}[hop_kind]
    # a few samples past the last frame (fewer than a hop), so that T rounds down
    segs = [noise(1000 * n_fft + 10 * hop + t, n_fft + (t - 1) * hop + min(hop - 1, 5)) for t in FRAME_COUNTS]
    first, count = standard_rows(n_fft)
    check_power(segs, n_fft, hop, "hann" if hop_kind != "1" else "rect", first, count, f"n_fft {n_fft} hop {hop}")


@pytest.mark.parametrize("n_fft", [256, 8192])
@pytest.mark.parametrize("nrows", [1, 254, 256])
def test_band_powers_with_one_row_and_with_256(n_fft, nrows):
    half = n_fft // 2
    j = np.arange(nrows)
    first = ((j * 37) % (half + 1)).astype(np.int32)
    count = np.minimum((j * 5) % 41, half + 1 - first).astype(np.int32)
    if nrows == 1:
        first, count = np.array([0], np.int32), np.array([half + 1], np.int32)
    segs = [noise(n_fft + nrows + t, n_fft + (t - 1) * 37 + 3) for t in (3, 17, 32)]
    check_power(segs, n_fft, 37, "hann", first, count, f"n_fft {n_fft} nrows {nrows}")


def test_silent_frames_are_exact_zeros():
    n_fft, hop = 256, 256
    first, count = standard_rows(n_fft)
    loud = noise(5, 256)
    x = np.concatenate([loud, np.zeros(256, np.float32), loud * 1e6, np.zeros(512, np.float32)]).astype(np.float32)
    edge = np.zeros(n_fft + 2 * hop, np.float32)
    edge[0] = 1.0                                                           # times hanning(256)[0] == 0: frame 0 is silent too
    edge[hop + 7] = 1.0
    got = run_power([x, np.zeros(1000, np.float32), edge], n_fft, hop, "hann", first, count, poison=False)
    live = count > 0
    assert np.all(got[0][:, [1, 3, 4]] == 0.0) and np.all(got[0][live][:, [0, 2]] > 0.0)
    assert np.all(got[1] == 0.0) and got[1].shape[1] == 16
    assert np.all(got[2][:, [0, 2]] == 0.0) and np.all(got[2][live][:, 1] > 0.0)


def test_a_segments_powers_do_not_depend_on_the_batch():
    n_fft, hop = 2048, 512
    first, count = standard_rows(n_fft)
    a, b, c = noise(1, n_fft + 20 * hop + 9), noise(2, n_fft + 40 * hop), noise(3, n_fft)
    alone = run_power([a], n_fft, hop, "hann", first, count)[0]
    for phase, (order, k) in enumerate((([a, b, c], 0), ([b, c, a], 2), ([b, a, c], 1), ([c, a, c, b], 1))):
        assert same(run_power(order, n_fft, hop, "hann", first, count, phase=phase + 1)[k], alone), order


# -------------------------------------------------------------------------------------------------------- ira_edr_integrate
def run_integrate(ps, qs, eps=EPS, floor_db=FLOOR, phase=0, with_s=True):
    """One ira_edr_integrate call on host-made powers ps = [(nrows, T) float64] -> [(S (nrows, Tpad) | None, records (nrows, 4),
    curve float32 (nrows, T))] per segment.  The padding columns of P hold NaN: they are never read."""
    from audio_analysis_amd._lib import check, ptr
    eng = _eng()
    nrows = ps[0].shape[0]
    frames = [p.shape[1] for p in ps]
    pads = [R.tpad(t) for t in frames]
    padded = []
    for p, t, tp in zip(ps, frames, pads):
        full = np.full((nrows, tp), np.nan)
        full[:, :t] = p
        padded.append(full.reshape(-1))
    fp = GB.Flat([nrows * tp for tp in pads], np.float64, phase)
    fc = GB.Flat([nrows * t for t in frames], np.float32, phase + 4)
    fr = GB.Flat([len(ps) * nrows * 4], np.float64, phase)
    d_p, d_c, d_r = (GB.to_device(eng, f.filled(v)) for f, v in ((fp, padded), (fc, None), (fr, None)))
    tabs = [GB.to_device(eng, a) for a in (np.asarray(fp.off, np.int64), np.asarray(frames, np.int32), np.asarray(qs, np.int32),
                                            np.asarray(fc.off, np.int64))]
    d_s = GB.to_device(eng, fp.filled()) if with_s else None                # S has the layout, and the offsets, of P
    check(eng.lib.ira_edr_integrate(ptr(d_p), ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), ptr(tabs[3]), len(ps), nrows, eps, floor_db,
                                    ptr(d_c), int(d_r.data_ptr()) + 8 * fr.off[0], ptr(d_s), eng.stream), "ira_edr_integrate")
    eng.sync()
    assert same(fp.split(d_p.cpu().numpy(), "P")[0], padded[0])             # the input is untouched
    curves = fc.split(d_c.cpu().numpy(), "curves")
    rec = fr.split(d_r.cpu().numpy(), "records")[0].reshape(len(ps), nrows, 4)
    sums = fp.split(d_s.cpu().numpy(), "S") if with_s else [None] * len(ps)
    return [(None if s is None else s.reshape(nrows, tp), rec[i], c.reshape(nrows, t))
            for i, (s, c, t, tp) in enumerate(zip(sums, curves, frames, pads))]


@functools.lru_cache(maxsize=None)
def host_powers(T):
    """(6, T): values over 1e-200 .. 1e200, exact small integers, zeros, a NaN at a chosen frame, an infinity at a chosen
    frame, a plain decay."""
    rng = np.random.default_rng(T)
    p = np.zeros((6, T))
    p[0] = 10.0 ** rng.uniform(-200.0, 200.0, T)
    p[1] = rng.integers(0, 1000, T).astype(np.float64)
    p[3] = rng.random(T)
    p[3, (2 * T) // 3] = np.nan
    p[4] = rng.random(T) * 1e3
    p[4, T // 2] = np.inf
    p[5] = 10.0 ** (-9.0 * np.arange(T) / max(T - 1, 1)) * (1.0 + 0.1 * rng.random(T)) + 1e-7
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def host_reference(T, q):
    p = host_powers(T)
    return [R.integrate_row(p[j], q) for j in range(p.shape[0])]


@pytest.mark.parametrize("q_kind", ["0", "1", "7", "T"])
def test_integrate_equals_the_restatement_bit_for_bit(q_kind):
    qs = [{"0": 0, "1": 1, "7": min(7, t), "T": t}[q_kind] for t in INTEGRATE_T]
    out = run_integrate([host_powers(t) for t in INTEGRATE_T], qs)
    worst = 0.0
    for t, q, (s, rec, curve) in zip(INTEGRATE_T, qs, out):
        assert np.all(s[:, t:] == 0.0), ("padding columns of S", t)
        for j, (rs, rn, rrec) in enumerate(host_reference(t, q)):
            assert same(s[j, :t], rs), ("S", t, q, j)
            assert same(rec[j], rrec) and same(rec[j, 1], rn), ("record", t, q, j, rec[j], rrec)
            worst = max(worst, R.compare_curve(curve[j], s[j, :t], EPS, FLOOR))
    print(f"q = {q_kind}: curve, observed / allowance {worst:.3f}")
    # the rows of zeros are silent: exactly the floor
    assert all(np.all(c[2] == np.float32(FLOOR)) for _, _, c in out)


def test_integrate_without_the_sums_and_whatever_the_batch():
    a, b, c = host_powers(129), host_powers(1000), host_powers(2)
    alone = run_integrate([a], [7])[0]
    for phase, (order, qs, k) in enumerate((([a, b, c], [7, 0, 2], 0), ([b, c, a], [100, 1, 7], 2), ([c, a, b], [0, 7, 1000], 1))):
        got = run_integrate(order, qs, phase=phase + 1, with_s=phase != 1)[k]
        assert same(got[1], alone[1]) and np.array_equal(got[2].view(np.uint32), alone[2].view(np.uint32)), order
        assert got[0] is None or same(got[0], alone[0])


# ----------------------------------------------------------------------------------------------------------- non-finite input
def test_a_nan_sample_marks_exactly_the_frames_that_cover_it():
    eng = _eng()
    n_fft, hop, at = 256, 96, 1500
    x = noise(9, n_fft + 40 * hop)
    x[at] = np.nan
    first, count = standard_rows(n_fft)
    d_x = GB.to_device(eng, x)
    p, frames, p_off = eng.edr_power(d_x, np.zeros(1, np.int64), np.array([x.size]), n_fft, hop, True, first, count)
    T = int(frames[0])
    _, _, rec, s = eng.edr_integrate(p, frames, first.size, np.zeros(1, np.int64), EPS, FLOOR, with_sums=True)
    P = p.cpu().numpy().reshape(first.size, R.tpad(T))[:, :T]
    S = s.cpu().numpy().reshape(first.size, R.tpad(T))[:, :T]
    covers = np.array([m * hop <= at < m * hop + n_fft for m in range(T)])
    assert T == 41 and covers.sum() == 3 and covers[-1] == False        # noqa: E712
    live = count > 0
    assert np.all(np.isnan(P[live]) == covers[None, :]) and np.all(P[~live] == 0.0)
    last = int(np.flatnonzero(covers)[-1])
    assert np.all(np.isnan(S[live][:, : last + 1])) and np.all(np.isfinite(S[live][:, last + 1 :]))
    r = rec.cpu().numpy().reshape(first.size, 4)
    assert np.all(np.isnan(r[live, 0])) and np.all(r[live, 3] == np.flatnonzero(covers)[0]) and np.all(r[~live, 0] == 0.0)
