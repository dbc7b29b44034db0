"""stft5_kernel (float64 / n_fft 8192: ira_stft_mag_db_tf and ira_stft_logbin) certifies a whole chunk of K consecutive
frames from one pass over the chunk's sample span and then stores the floor without loading a frame; in log-bin mode a
quiet frame of an uncertified chunk takes its log-bin values from a per-workgroup table.  The rule and the inputs are in
tests/test_stft_quiet_chunks_cpu.py; the cases, through the C-ABI, at odd segment offsets:

  hop 512, 24 frames (three chunks) and 27 frames (a short last chunk of 3), both output modes, Hann and rectangular
  windows, floors -120 and -93.7 dB:
  * all zeros; a loud first chunk before two certified ones; a loud short last chunk;
  * a chunk whose frames each pass the frame rule while the chunk rule fails;
  * chunks a part in a thousand under and over the chunk threshold;
  * one NaN sample inside an otherwise certified span: only the frames that hold it are NaN, every other value is the floor;
  * a faint segment that is the last of the batch: its last span ends 5 floats before the buffer does;
  * hop >= n_fft with loud noise in the gaps between the frames only;
  * dB mode with a frame selection that puts loud frames where the columns' own span is faint: the chunk test stays out;
  * a rectangular window table scaled to 2.5: a chunk that would be certified with max w^2 taken as 1 has bin 0 above the
    floor.

Every case is held to the float64 NumPy oracle by the rules of test_gpu_stft_dispatch (check64) and of
test_gpu_stft5_chunks (_check_logbin), and every output of every case must equal, byte for byte, what the tuning build
gives with every shortcut switched off (IRA_STFT5_ABLATE=256; in a process of its own, which is how that build is loaded).
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
if __name__ == "__main__":
    sys.path[:0] = [str(REPO), str(REPO / "tests")]

import test_gpu_stft5_chunks as C  # noqa: E402
import test_gpu_stft_dispatch as D  # noqa: E402
import test_stft_quiet_chunks_cpu as QC  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = QC.cases()
N_FFT = QC.N_FFT


@pytest.fixture(scope="module")
def eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def _logbin(eng, b, window, floor_db):
    """ira_stft_logbin with a given window table on a gapped output: every segment's (nbins, T) curves."""
    import torch
    from audio_analysis_amd._lib import check
    k_base, first, count = C._logbin_set()[:3]
    ln = D.Launch(eng, b, first.size)
    head, ooff = ln.args()
    d_first, d_count = torch.from_numpy(first).to(eng.device), torch.from_numpy(count).to(eng.device)
    check(eng.lib.ira_stft_logbin(*head, N_FFT, b.hop, window.data_ptr(), eng.twiddle(N_FFT, 64).data_ptr(), 64, floor_db,
                                  k_base, d_first.data_ptr(), d_count.data_ptr(), first.size, ln.out.data_ptr(), ooff,
                                  eng.stream), "ira_stft_logbin")
    return [m.reshape(first.size, t) for m, t in zip(ln.result(), b.cols)]


def _outputs(eng, name):
    """(dB matrices, log-bin curves or None) of one stft5 case."""
    use_hann, floor_db, b = CASES[name]
    mats = D._stft(eng, b, 64, use_hann, floor_db, frame_major=True)
    curves = C._logbin(eng, b, use_hann, floor_db) if all(s is None for s in b.sel) else None
    return mats, curves


def _scaled_window_outputs(eng):
    floor_db, b = QC.scaled_window_case()
    w = eng.window(N_FFT, False, 64) * QC.WSCALE
    return D._stft(eng, b, 64, False, floor_db, frame_major=True, window=w), _logbin(eng, b, w, floor_db)


@pytest.mark.parametrize("name", list(CASES))
def test_stft5_against_the_oracle(eng, name):
    use_hann, floor_db, b = CASES[name]
    assert np.any(b.off % 2 == 1)
    ref = b.reference(use_hann, floor_db)
    mats, curves = _outputs(eng, name)
    D.check64(list(zip(mats, ref)))
    if curves is not None:
        C._check_logbin(curves, ref)
    fl = np.float32(floor_db)
    for kind, m in zip(b.kinds, mats):
        if kind in ("zero", "zero27", "faint27", "under", "frames_pass", "gaps"):
            assert np.all(m == fl), kind
    if "nan_span" in b.kinds:
        nan_at = lambda s: range(9, 24) if b.kinds[s] == "nan_span" else []
        C._only_frames_nan(ref, nan_at)                          # the inputs are what this test says they are
        C._only_frames_nan(mats, nan_at)
        full = C._logbin_set()[2] > 0
        C._only_frames_nan([c[full] for c in curves], nan_at)
        m = mats[b.kinds.index("nan_span")]
        assert np.all(m[~np.isnan(m)] == fl)
    if name == "selected":
        m = mats[0]
        assert np.all(m[:, :5].max(axis=0) > floor_db + 40.0) and np.all(m[:, 5:16] == fl)


def test_stft5_with_a_scaled_window_table(eng):
    floor_db, b = QC.scaled_window_case()
    ref = QC.reference_with_window(b, QC.window(False, QC.WSCALE), floor_db)
    mats, curves = _scaled_window_outputs(eng)
    D.check64(list(zip(mats, ref)))
    C._check_logbin(curves, ref)
    by = dict(zip(b.kinds, mats))
    assert np.all(by["wmax_1"][0] > floor_db + 0.3) and np.all(by["wmax_1"][1:] == np.float32(floor_db))
    assert all(np.all(by[k] == np.float32(floor_db)) for k in ("under", "over", "zero"))


def _all_outputs(eng):
    """Every output of every case as one uint32 array."""
    parts = []
    for name in CASES:
        mats, curves = _outputs(eng, name)
        parts += mats + (curves or [])
    mats, curves = _scaled_window_outputs(eng)
    parts += mats + curves
    return np.concatenate([np.ascontiguousarray(p).ravel().view(np.uint32) for p in parts])


def test_the_shortcuts_change_no_byte(eng, tmp_path):
    got = _all_outputs(eng)
    out = tmp_path / "full_path.npy"
    env = dict(os.environ, IRA_TUNING="1", IRA_LIBRARY=str(C._tuning_library()), IRA_STFT5_ABLATE="256")
    subprocess.run([sys.executable, str(Path(__file__).resolve()), str(out)], env=env, check=True, timeout=600)
    full = np.load(out)
    assert got.size == full.size and np.array_equal(got, full), \
        f"{int(np.sum(got != full))} of {got.size} values differ from the full path's"


if __name__ == "__main__":
    from audio_analysis_amd.engine import get_engine
    np.save(sys.argv[1], _all_outputs(get_engine()))
