"""The quiet-chunk rule of stft5_kernel (float64 / n_fft 8192: ira_stft_mag_db_tf and ira_stft_logbin), in NumPy, and the
inputs of tests/test_gpu_stft_quiet_chunks.py.

stft5_kernel walks K consecutive frames of a segment per workgroup.  Without a frame selection it first sums x^2 over the
chunk's sample span [col0 hop, (col1 - 1) hop + N) and, where 4 N wmax2 S <= floor^2 (wmax2 = max w^2 of the window table it
was given), writes the floor for all of the chunk's frames without loading one of them.  That is right because
sum((x w)^2) over a frame <= wmax2 * sum(x^2) over the span: every frame of such a chunk obeys the per-frame rule of
tests/test_stft5_quiet_cpu.py (4 N sum(xw^2) <= floor^2), which that file holds to |X[k]|^2 < floor^2 / 2.  The test is made
only where the span is at most 2 N samples.  Here:

  * on every input of the GPU file, each chunk the rule certifies consists only of frames the frame rule certifies, and each
    of those frames has max |rfft(xw)|^2 < floor^2 / 2 in float64;
  * the inputs are what the GPU file's cases say (chunks on both sides of the rule, frames that pass where their chunk
    fails, a NaN inside a quiet span, the short last chunk, energy in the gaps between frames only);
  * a planted counter-example fails the check: a window table with maximum 2.5, judged with wmax2 = 1.

Span energies are summed directly (never as differences of running sums, which cancel).
"""
import numpy as np
import pytest

import test_stft5_quiet_cpu as Q

N_FFT, K, HOP = Q.N_FFT, Q.K, 512
SPAN_MAX = 2 * N_FFT                       # the kernel's SPAN5_MAX
L24 = N_FFT + 23 * HOP                     # 24 frames: three chunks of 8
L27 = N_FFT + 26 * HOP                     # 27 frames: a short last chunk of 3
L8 = N_FFT + 7 * HOP                       # one chunk
UNDER, OVER = Q.UNDER, Q.OVER
NAN_AT = 12388                             # inside frames 9 .. 23 of a 24-frame segment, behind the first chunk's span
WSCALE = 2.5


def window(use_hann, scale=1.0):
    return scale * (np.hanning(N_FFT) if use_hann else np.ones(N_FFT))


# ---------------------------------------------------------------------------------------------------------------- the rules
def span_energy(x, col0, nfr, hop):
    """sum x^2 over the samples frames col0 .. col0 + nfr - 1 read, in float64."""
    a = col0 * hop
    return float(np.sum(x[a : a + (nfr - 1) * hop + N_FFT].astype(np.float64) ** 2))


def chunk_rule(x, hop, frames, floor_db, wmax2, kfr=K):
    """Per frame: does the chunk rule certify the frame's chunk?  (False for a span that holds a NaN, like the kernel's.)"""
    out = np.zeros(frames, bool)
    for col0 in range(0, frames, kfr):
        nfr = min(kfr, frames - col0)
        if (nfr - 1) * hop + N_FFT <= SPAN_MAX:
            out[col0 : col0 + nfr] = 4.0 * N_FFT * wmax2 * span_energy(x, col0, nfr, hop) <= Q.floor_pow(floor_db)
    return out


def frames_of(x, hop, w, n_fft=N_FFT):
    """The (frames, n_fft) float64 windowed frames of one segment."""
    fr = np.lib.stride_tricks.sliding_window_view(x.astype(np.float64), n_fft)[::hop]
    return fr[: 1 + (x.size - n_fft) // hop] * w


def _scaled(x, lo, hi, rel, floor_db, wmax2=1.0):
    """x (float64) scaled so that 4 N wmax2 sum(x[lo:hi]^2) = rel floor^2."""
    return x * np.sqrt(rel * Q.floor_pow(floor_db) / (4.0 * N_FFT * wmax2 * np.sum(x[lo:hi] ** 2)))


def _noise(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


# --------------------------------------------------------------------------------------------------------- stft5 inputs
def _segments(use_hann, floor_db):
    """[(name, float32 signal)] at hop 512.  `faint` noise has a twentieth of the chunk threshold over the WHOLE segment."""
    w = window(use_hann)
    wmax2 = float(np.max(w * w))
    faint = lambda n, seed: _scaled(_noise(n, seed), 0, n, 0.05, floor_db)
    segs = [("zero", np.zeros(L24))]
    x = faint(L24, 11)
    x[: K * HOP] = 0.3 * _noise(K * HOP, 12)                      # in the first chunk's frames only
    segs.append(("loud_first", x))
    x = np.zeros(L24)
    if use_hann:                                                   # sample 1: frame 0 alone holds it, at w[1] = 1.5e-7
        x[1] = np.sqrt(0.5 * Q.floor_pow(floor_db) / (4.0 * N_FFT * w[1] ** 2))
    else:                                                          # first and last sample of the span: frames 0 and 7
        x[0] = x[(K - 1) * HOP + N_FFT - 1] = np.sqrt(0.6 * Q.floor_pow(floor_db) / (4.0 * N_FFT))
    segs.append(("frames_pass", x))
    for name, rel in (("under", UNDER), ("over", OVER)):           # samples both of the first two chunks' spans hold
        x = np.zeros(L24)
        x[K * HOP : N_FFT] = _noise(N_FFT - K * HOP, 13)
        segs.append((name, _scaled(x, 0, L24, rel, floor_db, wmax2)))
    x = faint(L24, 14)
    x[NAN_AT] = np.nan
    segs.append(("nan_span", x))
    x = faint(L27, 15)
    x[-2000:] = 0.3 * _noise(2000, 16)                             # the short last chunk is loud
    segs.append(("loud_tail", x))
    segs.append(("zero27", np.zeros(L27)))
    segs.append(("faint27", faint(L27, 17)))                       # the LAST segment: its last span ends the buffer
    return [(n, x.astype(np.float32)) for n, x in segs]


def _gap_segment(t, seed):
    """t frames at hop HOP_GAP, all zeros; the 37 samples between two frames hold loud noise."""
    x = np.zeros((t - 1) * Q.HOP_GAP + N_FFT)
    for j in range(t - 1):
        x[j * Q.HOP_GAP + N_FFT : (j + 1) * Q.HOP_GAP] = 0.3 * _noise(Q.HOP_GAP - N_FFT, seed + j)
    return x.astype(np.float32)


def _selected_segments():
    x = _scaled(_noise(L24, 21), 0, L24, 0.05, -120.0)
    x[-N_FFT // 2 :] = 0.3 * _noise(N_FFT // 2, 22)               # frames 16 .. 23 are loud, the first two spans faint
    loud_sel = np.concatenate([[23, 22, 21, 20, 16, 0, 1, 2], np.arange(3, 11), [17]])
    return [("loud_end", x.astype(np.float32), loud_sel),
            ("zero", np.zeros(L24, np.float32), np.repeat(np.arange(2, 14), 2)[: 2 * K + 3])]


def cases():
    """name -> (window, floor dB, batch): the stft5 launches of tests/test_gpu_stft_quiet_chunks.py with the standard
    window tables.  The batches without a frame selection run in both output modes."""
    out = {}
    for use_hann, floor_db in Q.CONFIGS:
        out[f"chunks hann={use_hann} floor={floor_db}"] = use_hann, floor_db, Q.QuietBatch(
            HOP, [(n, x, None) for n, x in _segments(use_hann, floor_db)])
    for use_hann, floor_db in Q.CONFIGS[:2]:
        out[f"gaps hann={use_hann} floor={floor_db}"] = use_hann, floor_db, Q.QuietBatch(
            Q.HOP_GAP, [("gaps", _gap_segment(K + 3, 30), None), ("gaps", _gap_segment(2, 50), None)])
    out["selected"] = True, -120.0, Q.QuietBatch(HOP, _selected_segments())
    return out


def scaled_window_case():
    """(floor dB, batch): constant segments of one chunk under the RECTANGULAR window scaled to 2.5, where the bound is
    attained at bin 0.  'wmax_1' is under the chunk threshold only if wmax2 were taken as 1 (its bin 0 then lies 0.36 dB
    ABOVE the floor); 'under' and 'over' sit a part in a thousand off the true threshold, wmax2 = 6.25."""
    floor_db = -120.0
    one = np.ones(L8)
    segs = [("wmax_1", _scaled(one, 0, L8, UNDER, floor_db, 1.0)),
            ("under", _scaled(one, 0, L8, UNDER, floor_db, WSCALE ** 2)),
            ("over", _scaled(one, 0, L8, OVER, floor_db, WSCALE ** 2)),
            ("zero", np.zeros(L8))]
    return floor_db, Q.QuietBatch(HOP, [(n, x.astype(np.float32), None) for n, x in segs])


def reference_with_window(b, w, floor_db):
    """The oracle's rule (|rfft| -> max(., floor) -> 20 log10 -> float32) with a given window table: (F, T) per segment."""
    fl = 10.0 ** (float(floor_db) / 20.0)
    return [(20.0 * np.log10(np.maximum(np.abs(np.fft.rfft(frames_of(x, b.hop, w, b.n_fft), axis=1)), fl))).astype(np.float32).T
            for x in b.segs]


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.fixture(scope="module")
def marked():
    """name -> [(segment name, windowed frames, chunk-certified mask, floor dB)] of the unselected stft5 cases"""
    out = {}
    for name, (use_hann, floor_db, b) in cases().items():
        if b.sel[0] is None:
            w = window(use_hann)
            out[name] = [(b.kinds[s], frames_of(x, b.hop, w), chunk_rule(x, b.hop, b.valid[s], floor_db, float(np.max(w * w))),
                          floor_db) for s, x in enumerate(b.segs)]
    return out


def test_a_certified_chunk_holds_certified_frames_only(marked):
    quiet = loud = 0
    for name, segs in marked.items():
        for _, xw, cert, floor_db in segs:
            assert np.all(Q.quiet_rule(xw, floor_db)[cert]), name
            Q.check_quiet_frames(xw, cert, floor_db)
            quiet += int(cert.sum())
            loud += int((~cert).sum())
    assert quiet > 200 and loud > 200, (quiet, loud)


def test_the_inputs_are_what_the_cases_say(marked):
    assert K == 8
    chunks = lambda m: [bool(m[i]) for i in range(0, m.size, K)]
    for name, segs in marked.items():
        by = {}
        for kind, xw, cert, floor_db in segs:
            by.setdefault(kind, (xw, cert, Q.quiet_rule(xw, floor_db), Q.scaled_energy(xw) / Q.floor_pow(floor_db)))
        if name.startswith("gaps"):
            xw, cert, fq, rel = by["gaps"]
            assert not cert.any() and fq.all() and np.all(rel == 0)                  # no chunk test at this hop; silent frames
            continue
        for kind, (xw, cert, fq, rel) in by.items():
            assert np.all(cert == np.repeat(chunks(cert), K)[: cert.size]), (name, kind)   # whole chunks
        assert by["zero"][1].all() and by["zero27"][1].all() and by["faint27"][1].all()
        assert by["zero27"][1].size == 3 * K + 3 and np.any(by["faint27"][3] > 0)
        assert segs[-1][0] == "faint27"
        assert chunks(by["loud_first"][1]) == [False, True, True] and not by["loud_first"][2][:K].any()
        xw, cert, fq, rel = by["frames_pass"]
        assert chunks(cert) == [False, True, True] and fq.all() and rel[:K].max() > 0.4   # the frame rule passes, the chunk's fails
        assert chunks(by["under"][1]) == [True, True, True] and chunks(by["over"][1]) == [False, False, True]
        xw, cert, fq, rel = by["nan_span"]
        bad = np.isnan(xw).any(axis=1)
        assert np.array_equal(np.nonzero(bad)[0], np.arange(9, 24)) and chunks(cert) == [True, False, False]
        assert np.array_equal(fq, ~bad)                                                # frame 8: quiet by the frame rule alone
        xw, cert, fq, rel = by["loud_tail"]
        assert chunks(cert) == [True, True, False, False] and fq[2 * K : 3 * K - 1].all() and not fq[3 * K :].any()
    # the threshold pair is a part in a thousand off the threshold, in float32 samples
    use_hann, floor_db, b = cases()["chunks hann=True floor=-120.0"]
    w = window(True)
    for kind, want in (("under", UNDER), ("over", OVER)):
        x = b.segs[b.kinds.index(kind)]
        rel = 4.0 * N_FFT * np.max(w * w) * span_energy(x, 0, K, HOP) / Q.floor_pow(floor_db)
        assert abs(rel / want - 1.0) < 1e-5
    # the selection puts loud frames into an output chunk whose own columns' span is faint
    _, floor_db, b = cases()["selected"]
    x, sel = b.segs[0], b.sel[0]
    assert chunk_rule(x, HOP, b.valid[0], floor_db, 1.0)[: 2 * K].all()
    fq = Q.quiet_rule(frames_of(x, HOP, window(True)), floor_db)
    assert not fq[sel[:5]].any() and fq[sel[5:16]].all()
    assert np.any(b.off % 2 == 1) and all(np.any(c[2].off % 2 == 1) for c in cases().values())


def test_a_scaled_window_judged_as_one_fails():
    """The planted counter-example: under a window table of maximum 2.5 a chunk that 4 N S <= floor^2 alone would certify
    has a bin above the floor; the rule with the table's own maximum does not certify it."""
    floor_db, b = scaled_window_case()
    w = window(False, WSCALE)
    x = b.segs[b.kinds.index("wmax_1")]
    xw = frames_of(x, HOP, w)
    assert chunk_rule(x, HOP, K, floor_db, 1.0).all() and not chunk_rule(x, HOP, K, floor_db, WSCALE ** 2).any()
    assert np.all(np.abs(np.fft.rfft(xw, axis=1)[:, 0]) ** 2 > 1.05 * Q.floor_pow(floor_db))
    with pytest.raises(AssertionError):
        Q.check_quiet_frames(xw, chunk_rule(x, HOP, K, floor_db, 1.0), floor_db)
    for kind, want in (("under", True), ("over", False), ("zero", True)):
        x = b.segs[b.kinds.index(kind)]
        cert = chunk_rule(x, HOP, K, floor_db, WSCALE ** 2)
        assert cert.all() == want and cert.any() == want
        Q.check_quiet_frames(frames_of(x, HOP, w), cert, floor_db)
