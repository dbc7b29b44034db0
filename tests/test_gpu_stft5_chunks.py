"""stft5_kernel (float64 / n_fft 8192: ira_stft_mag_db_tf and ira_stft_logbin) walks K consecutive frames of a segment per
workgroup.  These cases sit on the edges of that loop, through the C-ABI, against the float64 NumPy oracle by the rules of
test_gpu_stft_dispatch (precision 64: every bin within one float32 ulp of the reference or 1e-12 of the frame's peak in
linear terms, >= 99 % bit-identical, equal NaN masks; log-bin curves: the same, plus one ulp of the rows a bin averages):

  * frame counts 1, K-1, K, K+1, 2K+3, a multiple of K next to one that is not, and (through an empty frame selection, the
    only way the ABI describes one) 0, in one ragged batch; segment offsets are odd (sample pairs are 4-byte aligned only);
  * a NaN sample in a frame in the middle of a chunk: that frame alone is NaN, the frames after it in the chunk are finite;
  * frame selections out of order, repeated and empty;
  * the results do not depend on K: the tuning build (IRA_STFT5_K) at two other K gives the very bytes of the product
    library (each in a process of its own, which is how that build is loaded).

The fused log-bin curves are also held against ira_stft_mag_db_tf + ira_logbin_aggregate by the bound the existing
comparison of the two uses (test_gpu_waterfall_modal: < 2e-5 dB, > 99.9 % equal): the two paths convert dB to linear
magnitude by different formulas and never were bit-identical.
"""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
if __name__ == "__main__":
    sys.path[:0] = [str(REPO), str(REPO / "tests")]

import test_gpu_stft_dispatch as D  # noqa: E402
from oracle import ira_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
N_FFT = 8192
K = int(re.search(r"constexpr int KF5 = (\d+);", (REPO / "audio_analysis_amd/csrc/ira_stft4.hip").read_text()).group(1))
COUNTS = (1, K - 1, K, K + 1, 2 * K + 3, 3 * K, 2 * K - 1)
KINDS = ("ir", "noise", "tone_mid", "ir_large", "ir", "noise", "ir_small")


def _ragged():
    """(window, floor, batch): every frame count of COUNTS, hop odd and below n_fft (frames overlap)."""
    return True, -120.0, D.Batch(N_FFT, N_FFT // 4 + 1, [(k, t, None) for k, t in zip(KINDS, COUNTS)])


def _nan_batch():
    """hop >= n_fft, so the NaN of 'nan_mid' lies in frame 2 alone: the third frame of a chunk of K."""
    return False, -93.7, D.Batch(N_FFT, N_FFT + 37, [("nan_mid", K + 5, None), ("ir", K, None), ("nan_mid", 2 * K + 3, None)])


def _selected():
    rng = np.random.default_rng(5)
    segs = [("ir", 3 * K, np.concatenate([rng.permutation(3 * K)[: 2 * K + 3], [3 * K - 1, 3 * K - 1, 0]])),
            ("noise", K, np.zeros(0, np.int64)),                                  # no frame at all
            ("tone_mid", K + 1, np.arange(K, -1, -1)),
            ("nan_mid", K + 2, np.array([4, 2, K + 1, 2, 0, 3, 1])),
            ("ir", 2 * K, np.arange(0, 2 * K, 2)[:K])]                            # exactly one chunk
    return True, -120.0, D.Batch(N_FFT, 3 * N_FFT // 8 + 3, segs)


def _logbin_set():
    """The modal cloud's bins: 20 Hz .. 20 kHz, 24 per octave."""
    freq = np.fft.rfftfreq(N_FFT, 1.0 / D.SR).astype(np.float32)
    rows = np.nonzero((freq >= 20.0) & (freq <= 20000.0))[0]
    edges = O.log_bin_edges(20.0, 20000.0, 24, 24)
    _, first, count = O.log_bin_membership(freq[rows], edges)
    return int(rows[0]), first.astype(np.int32), count.astype(np.int32), edges, rows.size, freq


def _logbin(eng, b, use_hann, floor_db):
    """ira_stft_logbin on a gapped output: every segment's (nbins, T) curves."""
    import torch
    from audio_analysis_amd._lib import check
    k_base, first, count = _logbin_set()[:3]
    ln = D.Launch(eng, b, first.size)
    head, ooff = ln.args()
    d_first, d_count = torch.from_numpy(first).to(eng.device), torch.from_numpy(count).to(eng.device)
    check(eng.lib.ira_stft_logbin(*head, N_FFT, b.hop, eng.window(N_FFT, use_hann, 64).data_ptr(),
                                  eng.twiddle(N_FFT, 64).data_ptr(), 64, floor_db, k_base, d_first.data_ptr(),
                                  d_count.data_ptr(), first.size, ln.out.data_ptr(), ooff, eng.stream), "ira_stft_logbin")
    return [m.reshape(first.size, t) for m, t in zip(ln.result(), b.cols)]


def _check_logbin(curves, refm):
    """The rule of test_gpu_stft_dispatch.test_stft_logbin over (curves, reference dB matrix) pairs."""
    k_base, first, count, edges, nrows, freq = _logbin_set()
    n = same = 0
    for got, mag in zip(curves, refm):
        _, ref = O.aggregate_log_bins(freq[k_base : k_base + nrows], mag[k_base : k_base + nrows], edges)
        row_ulp = np.zeros(ref.shape)
        for j in np.nonzero(count)[0]:
            r0 = k_base + first[j]
            row_ulp[j] = np.spacing(np.abs(mag[r0 : r0 + count[j]])).max(axis=0)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN masks differ"
        full = count > 0
        keep = ~np.isnan(ref[full]).any(axis=0)
        g, r, u = got[full][:, keep], ref[full][:, keep], row_ulp[full][:, keep]
        err = np.abs(g.astype(np.float64) - r.astype(np.float64))
        ulp = np.spacing(np.abs(r)).astype(np.float64)
        bad = (err > ulp + u) & ~(D._lin_err(g, r) < 1e-12)
        assert not bad.any(), float(np.max(err / ulp))
        n += r.size
        same += int(np.sum(g.view(np.uint32) == r.view(np.uint32)))
    assert n > 0 and same >= 0.99 * n, (same, n)


def _only_frames_nan(mats, frames_of):
    """Per segment: exactly the columns frames_of(segment) are NaN (all of the column), every other value is finite."""
    for s, m in enumerate(mats):
        want = np.zeros(m.shape[1], bool)
        want[list(frames_of(s))] = True
        assert np.array_equal(np.isnan(m).all(axis=0), want) and np.array_equal(np.isnan(m).any(axis=0), want), s


@pytest.fixture(scope="module")
def eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def test_ragged_chunks(eng):
    use_hann, floor_db, b = _ragged()
    assert np.array_equal(b.cols, COUNTS) and np.any(b.off % 2 == 1)
    ref = b.reference(use_hann, floor_db)
    D.check64(list(zip(D._stft(eng, b, 64, use_hann, floor_db, frame_major=True), ref)))
    _check_logbin(_logbin(eng, b, use_hann, floor_db), ref)


def test_nan_frame_inside_a_chunk(eng):
    use_hann, floor_db, b = _nan_batch()
    ref = b.reference(use_hann, floor_db)
    nan_at = lambda s: [2] if b.kinds[s] == "nan_mid" else []
    _only_frames_nan(ref, nan_at)                                 # the inputs are what this test says they are
    got = D._stft(eng, b, 64, use_hann, floor_db, frame_major=True)
    _only_frames_nan(got, nan_at)
    D.check64(list(zip(got, ref)))
    cur = _logbin(eng, b, use_hann, floor_db)
    full = _logbin_set()[2] > 0
    _only_frames_nan([c[full] for c in cur], nan_at)
    _check_logbin(cur, ref)


def test_frame_selections(eng):
    use_hann, floor_db, b = _selected()
    assert 0 in b.cols and K in b.cols
    got = D._stft(eng, b, 64, use_hann, floor_db, frame_major=True)
    D.check64(list(zip(got, b.reference(use_hann, floor_db))))


def test_fused_logbin_against_the_two_kernel_path(eng):
    use_hann, floor_db, b = _ragged()
    import torch
    k_base, first, count = _logbin_set()[:3]
    x = torch.from_numpy(b.x).to(eng.device)
    mag, off, cols = eng.stft_mag_db(x, b.off, b.valid, N_FFT, b.hop, use_hann, floor_db, 64, frame_major=True)
    two, two_off = eng.logbin_aggregate(mag, off, cols, k_base, first, count, frame_major_rows=N_FFT // 2 + 1)
    eng.sync()
    two = two.cpu().numpy()
    for o, t, f in zip(two_off, cols, _logbin(eng, b, use_hann, floor_db)):
        s = two[o : o + first.size * t].reshape(first.size, t)
        assert np.array_equal(np.isnan(f), np.isnan(s))
        ok = ~np.isnan(s)
        assert np.max(np.abs(f[ok] - s[ok])) < 2e-5 and np.mean(f[ok] == s[ok]) > 0.999


def _all_outputs(eng):
    """Every output of the batches above as one uint32 array."""
    parts = []
    for use_hann, floor_db, b in (_ragged(), _nan_batch(), _selected()):
        parts += D._stft(eng, b, 64, use_hann, floor_db, frame_major=True)
        if all(s is None for s in b.sel):
            parts += _logbin(eng, b, use_hann, floor_db)
    return np.concatenate([np.ascontiguousarray(p).ravel().view(np.uint32) for p in parts])


def _tuning_library():
    from audio_analysis_amd import build as B
    lib = B.CSRC / "libira_tuning.so"
    deps = [B.CSRC / n for n in B.SOURCES] + list(B.CSRC.glob("*.h")) + [REPO / "include" / "ira.h"]
    if not lib.exists() or any(d.stat().st_mtime > lib.stat().st_mtime for d in deps):
        B.build_tuning(verbose=False)
    return lib


def test_results_do_not_depend_on_k(eng, tmp_path):
    ref = _all_outputs(eng)
    lib = _tuning_library()
    for k in (5, 2 * K):
        out = tmp_path / f"k{k}.npy"
        env = dict(os.environ, IRA_TUNING="1", IRA_LIBRARY=str(lib), IRA_STFT5_K=str(k))
        subprocess.run([sys.executable, str(Path(__file__).resolve()), str(out)], env=env, check=True, timeout=600)
        assert np.array_equal(np.load(out), ref), f"K = {k} and K = {K} give different bytes"


if __name__ == "__main__":
    from audio_analysis_amd.engine import get_engine
    np.save(sys.argv[1], _all_outputs(get_engine()))
