"""The quiet-frame rule of stft5_kernel (float64 / n_fft 8192: ira_stft_mag_db_tf and ira_stft_logbin), in NumPy, and the
inputs of tests/test_gpu_stft5_quiet.py.

The kernel skips the transform of a frame whose windowed samples xw[n] obey 4 N sum(xw^2) <= floor^2 (N = 8192, floor =
10^(floor_db / 20)) and writes the floor instead.  That is right because every bin obeys |X[k]|^2 <= N sum(xw^2) (triangle
inequality, then Cauchy-Schwarz); the factor 4 is a 6 dB margin over the float64 rounding of the transform.  Here:

  * on every input of the GPU file, each frame the rule calls quiet has max |rfft(xw)|^2 < floor^2 / 2 in float64;
  * the inputs are what the GPU file's cases say: frames on both sides of the rule, the change from loud to quiet (and back)
    inside a chunk of K frames, frames a part in a thousand under and over the threshold, NaN frames that the rule does not
    call quiet between frames that it does, odd segment offsets, selections that repeat and reverse quiet frames;
  * a planted counter-example fails the check: a constant frame under a rectangular window, where the bound is attained at
    bin 0, with an energy 8 times the threshold and forced to "quiet".

The frame energy is summed directly per frame (never as a difference of running sums, which cancels).
"""
import numpy as np
import pytest

import test_gpu_stft5_chunks as C
import test_gpu_stft_dispatch as D

N_FFT = C.N_FFT
K = C.K
HOP_GAP = N_FFT + 37                 # hop >= n_fft: a frame shares no sample with its neighbours
CONFIGS = ((True, -120.0), (False, -93.7), (True, -93.7), (False, -120.0))


def floor_pow(floor_db):
    """floor^2 as the launcher forms it."""
    return (10.0 ** (float(floor_db) / 20.0)) ** 2


def _window(use_hann):
    return np.hanning(N_FFT) if use_hann else np.ones(N_FFT)


class QuietBatch(D.Batch):
    """D.Batch's layout (every offset off a multiple of four, gaps between the segments) over given signals:
    segs = [(name, float32 signal, frame selection or None)]."""

    def __init__(self, hop, segs):
        self.n_fft, self.hop = N_FFT, hop
        self.kinds, self.sel, xs, offs, pos = [], [], [], [], 3
        for s, (name, x, sel) in enumerate(segs):
            assert x.dtype == np.float32 and x.size >= N_FFT
            xs.append(x)
            offs.append(pos)
            pos += x.size + 1 + 2 * (s % 3)
            pos += 1 if pos % 4 == 0 else 0
            self.kinds.append(name)
            self.sel.append(None if sel is None else np.asarray(sel, np.int64))
        self.x = np.zeros(pos + 5, np.float32)
        for o, x in zip(offs, xs):
            self.x[o : o + x.size] = x
        self.segs = xs
        self.off = np.array(offs, np.int64)
        self.valid = np.array([1 + (x.size - N_FFT) // hop for x in xs], np.int32)
        assert np.all(self.off % 4 != 0)
        self.cols = np.array([v if s is None else s.size for v, s in zip(self.valid, self.sel)], np.int32)


# ------------------------------------------------------------------------------------------------------------ signals
def _decay(t, hop, seed, reverse=False, decades=28.0):
    """t frames of noise that falls by `decades` over the segment and is exactly zero over its last two fifths; reversed:
    silence, then the burst."""
    n = (t - 1) * hop + N_FFT + 101
    x = 0.3 * np.random.default_rng(seed).standard_normal(n) * 10.0 ** (-decades * np.arange(n) / n)
    x[(3 * n) // 5 :] = 0.0
    return (x[::-1] if reverse else x).astype(np.float32)


def _levels(pattern, rels, use_hann, floor_db, hop=HOP_GAP, nan_at=()):
    """One frame of `pattern` per entry of rels, hop >= n_fft apart, scaled so that 4 N sum(xw^2) = rel * floor^2;
    nan_at = (frame, sample of the frame) pairs that are overwritten with NaN."""
    assert hop >= N_FFT
    e = np.sum((pattern * _window(use_hann)) ** 2)
    x = np.zeros((len(rels) - 1) * hop + N_FFT + 55)
    for j, rel in enumerate(rels):
        x[j * hop : j * hop + N_FFT] = pattern * np.sqrt(rel * floor_pow(floor_db) / (4.0 * N_FFT) / e)
    for j, i in nan_at:
        x[j * hop + i] = np.nan
    return x.astype(np.float32)


UNDER, OVER = 1.0 - 1e-3, 1.0 + 1e-3
THRESHOLD_RELS = [UNDER, OVER, OVER, UNDER, UNDER, UNDER, OVER, UNDER, OVER, OVER, OVER, UNDER, OVER, UNDER, UNDER, OVER,
                  UNDER, OVER, UNDER][: 2 * K + 3]
DC_RELS = [UNDER, 8.0, UNDER, UNDER, 8.0, 8.0, UNDER, 8.0, UNDER][: K + 1]
NAN_RELS = [1e-2] * (K + 5)


def cases():
    """name -> (window, floor dB, batch): the launches of tests/test_gpu_stft5_quiet.py.  Every segment has at most
    2 K + 3 frames."""
    out = {}
    for use_hann, floor_db, hop, dec in ((True, -120.0, 1537, 28.0), (False, -93.7, 1025, 24.0)):
        t = 2 * K + 3
        out[f"decay hann={use_hann} floor={floor_db}"] = use_hann, floor_db, QuietBatch(hop, [
            ("decay", _decay(t, hop, 1, decades=dec), None), ("burst", _decay(t, hop, 2, reverse=True, decades=dec), None),
            ("zero", np.zeros(K * hop + N_FFT + 7, np.float32), None), ("decay", _decay(K + 1, hop, 3, decades=dec), None)])
    noise = np.random.default_rng(7).standard_normal(N_FFT)
    for use_hann, floor_db in CONFIGS:
        out[f"threshold hann={use_hann} floor={floor_db}"] = use_hann, floor_db, QuietBatch(HOP_GAP, [
            ("noise", _levels(noise, THRESHOLD_RELS, use_hann, floor_db), None),
            ("dc", _levels(np.ones(N_FFT), DC_RELS, use_hann, floor_db), None)])
    for use_hann, floor_db in CONFIGS[:2]:
        out[f"nan hann={use_hann} floor={floor_db}"] = use_hann, floor_db, QuietBatch(HOP_GAP, [
            ("nan2", _levels(noise, NAN_RELS, use_hann, floor_db, nan_at=[(2, N_FFT // 2 + 1)]), None),
            # the first sample of a frame: a Hann end point, 0 * NaN is NaN too
            ("nan_edge", _levels(noise, [0.0] * (2 * K + 3), use_hann, floor_db, nan_at=[(K + 1, 0)]), None)])
    t = 2 * K + 3
    out["selected"] = True, -120.0, QuietBatch(1537, [
        ("decay", _decay(t, 1537, 1), np.concatenate([np.arange(t - 1, 4, -1), [t - 1, t - 1, t - 2, t - 2, 0]])),
        ("burst", _decay(t, 1537, 2, reverse=True), np.repeat(np.arange(5, K + 7), 2)[: 2 * K + 3]),
        ("zero", np.zeros(K * 1537 + N_FFT, np.float32), np.array([3, 3, 0, K, 1]))])
    return out


NAN_FRAMES = {"nan2": [2], "nan_edge": [K + 1]}


# -------------------------------------------------------------------------------------------------------------- the rule
def windowed_frames(b, s, use_hann):
    """The (frames, n_fft) float64 windowed frames of segment s, in output order."""
    x = b.segs[s].astype(np.float64)
    fr = np.lib.stride_tricks.sliding_window_view(x, N_FFT)[:: b.hop][: b.valid[s]]
    if b.sel[s] is not None:
        fr = fr[b.sel[s]]
    return fr * _window(use_hann)


def scaled_energy(xw):
    """4 N sum(xw^2) per frame."""
    return np.sum(xw * xw, axis=1) * (4.0 * N_FFT)


def quiet_rule(xw, floor_db):
    return scaled_energy(xw) <= floor_pow(floor_db)                # false for a frame holding a NaN, like the kernel's


def check_quiet_frames(xw, quiet, floor_db):
    """Every frame marked quiet is floored on every bin, with 3 dB to spare."""
    if quiet.any():
        p = np.abs(np.fft.rfft(xw[quiet], axis=1)) ** 2
        assert np.all(p.max(axis=1) < 0.5 * floor_pow(floor_db)), float(p.max() / floor_pow(floor_db))


@pytest.fixture(scope="module")
def marked():
    """name -> [(segment name, windowed frames, quiet mask, floor dB)]"""
    out = {}
    for name, (use_hann, floor_db, b) in cases().items():
        out[name] = [(b.kinds[s], xw, quiet_rule(xw, floor_db), floor_db)
                     for s in range(len(b.segs)) for xw in [windowed_frames(b, s, use_hann)]]
    return out


def test_every_certified_frame_is_under_the_floor(marked):
    quiet = loud = 0
    for name, segs in marked.items():
        for _, xw, q, floor_db in segs:
            check_quiet_frames(xw, q, floor_db)
            quiet += int(q.sum())
            loud += int((~q).sum())
    assert quiet > 50 and loud > 50, (quiet, loud)                 # frames on both sides of the rule


def test_the_inputs_are_what_the_cases_say(marked):
    all_cases = cases()
    for name, (use_hann, floor_db, b) in all_cases.items():
        assert b.cols.max() <= 2 * K + 3 and np.any(b.off % 2 == 1) and np.all(b.off % 4 != 0), name
    for name, segs in marked.items():
        for kind, xw, q, floor_db in segs:
            rel = scaled_energy(xw) / floor_pow(floor_db)
            if name.startswith("decay") and kind == "decay":
                first = int(np.argmax(q))
                assert q.any() and not q[:first].any() and q[first:].all(), name       # loud, then quiet for good
                assert first % K != 0 or q.size <= K + 1, (name, first)               # the change falls inside a chunk
                assert np.any(rel[q] > 0) and (np.any(rel == 0) or q.size <= K + 1)    # certified noise and exact zeros
            if name.startswith("decay") and kind == "burst":
                first = int(np.argmin(q))
                assert q[:first].all() and not q[first:].any() and 0 < first and first % K != 0, (name, first)
            if kind == "zero":
                assert q.all() and np.all(rel == 0)
            if kind == "noise":
                want = np.array(THRESHOLD_RELS)
                assert np.all(np.abs(rel / want - 1.0) < 1e-5) and np.array_equal(q, want < 1.0), name
                assert np.any(q[:K] != q[0])                                           # both kinds inside one chunk
            if kind == "dc":
                want = np.array(DC_RELS)
                assert np.all(np.abs(rel / want - 1.0) < 1e-5) and np.array_equal(q, want < 1.0), name
            if kind in NAN_FRAMES:
                bad = np.zeros(q.size, bool)
                bad[NAN_FRAMES[kind]] = True
                assert np.array_equal(np.isnan(xw).any(axis=1), bad) and np.array_equal(q, ~bad), name
    # bin 0 of a loud constant frame under the rectangular window lies ABOVE the floor: calling it quiet would show
    _, xw, q, floor_db = marked["threshold hann=False floor=-93.7"][1]
    assert np.all(np.abs(np.fft.rfft(xw[~q], axis=1)[:, 0]) ** 2 > 1.9 * floor_pow(floor_db))
    sel = marked["selected"]
    assert all(q.any() for _, _, q, _ in sel)                                          # quiet frames are selected ...
    b = all_cases["selected"][2]
    assert np.all(np.diff(b.sel[0][: 2 * K - 2]) == -1) and np.any(np.diff(b.sel[1]) == 0)   # ... reversed and repeated


def test_a_planted_counter_example_fails():
    """A constant frame under the rectangular window attains the bound at bin 0: |X[0]|^2 = N sum(x^2).  At 8 times the
    threshold that is twice the floor, so a rule that called this frame quiet must fail the check."""
    floor_db = -120.0
    x = _levels(np.ones(N_FFT), [8.0], False, floor_db)[:N_FFT].astype(np.float64)[None, :]
    assert abs(scaled_energy(x)[0] / floor_pow(floor_db) - 8.0) < 1e-4
    assert not quiet_rule(x, floor_db)[0]
    check_quiet_frames(x, quiet_rule(x, floor_db), floor_db)       # nothing marked: passes
    with pytest.raises(AssertionError):
        check_quiet_frames(x, np.array([True]), floor_db)
