"""stft5_kernel (float64 / n_fft 8192: ira_stft_mag_db_tf and ira_stft_logbin) skips the transform of a frame whose windowed
samples obey 4 N sum(xw^2) <= floor^2 and writes the floor instead (the rule and its inputs: tests/test_stft5_quiet_cpu.py).
The cases below put frames on both sides of that rule, through the C-ABI, in both output modes:

  * decaying noise that ends in exact zeros, and silence followed by a burst: the change falls inside a chunk of K frames;
    an all-zero segment;
  * frames of one fixed noise pattern, hop >= n_fft, scaled a part in a thousand under and over the threshold, and constant
    frames (whose bin 0 attains the bound under the rectangular window) just under it and 8 times over it;
  * a quiet-level frame holding one NaN sample (also on a Hann end point): that frame alone is NaN, every other value of
    the segment IS the floor;
  * floors -120 and -93.7 dB, Hann and rectangular windows; odd segment offsets (every batch);
  * frame selections that repeat and reverse quiet frames -- frame-major dB output only: ira_stft_logbin takes no selection.

Every case is held to the float64 NumPy oracle by the rules of test_gpu_stft_dispatch (check64) and of
test_gpu_stft5_chunks (_check_logbin), and every output of every case must equal, byte for byte, what the tuning build gives
with the shortcut switched off (IRA_STFT5_ABLATE bit 8; in a process of its own, which is how that build is loaded).
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
import test_stft5_quiet_cpu as Q  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = Q.cases()


@pytest.fixture(scope="module")
def eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def _outputs(eng, name):
    """(dB matrices, log-bin curves or None) of one case."""
    use_hann, floor_db, b = CASES[name]
    mats = D._stft(eng, b, 64, use_hann, floor_db, frame_major=True)
    curves = C._logbin(eng, b, use_hann, floor_db) if all(s is None for s in b.sel) else None
    return mats, curves


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_oracle(eng, name):
    use_hann, floor_db, b = CASES[name]
    assert np.any(b.off % 2 == 1)
    ref = b.reference(use_hann, floor_db)
    mats, curves = _outputs(eng, name)
    D.check64(list(zip(mats, ref)))
    if curves is not None:
        C._check_logbin(curves, ref)
    if name.startswith("nan"):
        nan_at = lambda s: Q.NAN_FRAMES[b.kinds[s]]
        C._only_frames_nan(ref, nan_at)                          # the inputs are what this test says they are
        C._only_frames_nan(mats, nan_at)
        full = C._logbin_set()[2] > 0
        C._only_frames_nan([c[full] for c in curves], nan_at)
        for m in mats:                                           # the quiet frames around the NaN frame: the floor itself
            assert np.all(m[~np.isnan(m)] == np.float32(floor_db))
    if name.startswith("decay"):
        zero = b.kinds.index("zero")
        assert np.all(mats[zero] == np.float32(floor_db))


def _all_outputs(eng):
    """Every output of every case as one uint32 array."""
    parts = []
    for name in CASES:
        mats, curves = _outputs(eng, name)
        parts += mats + (curves or [])
    return np.concatenate([np.ascontiguousarray(p).ravel().view(np.uint32) for p in parts])


def test_the_shortcut_changes_no_byte(eng, tmp_path):
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
