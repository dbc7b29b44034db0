"""
CPU tests of audio_analysis_amd/engine_geometry.py: the table checks several measure launchers share, at their edges; the
engine's output views; that the module stands on NumPy alone; and that engine.py re-exports its names.
"""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from audio_analysis_amd import engine
from audio_analysis_amd import engine_geometry as G
from audio_analysis_amd.engine_measure import _ptr
from host_engine import HostEngine

REPO = Path(__file__).resolve().parent.parent

CONSTANTS = """TAIL_BLOCK LUNDEBY_DOUBLES LUNDEBY_MAX_BLOCKS LUNDEBY_STAGE LUNDEBY_MAX_LEN MS_DOUBLES MS_MAX_GRID MS_MAX_ORDER
    MS_TILE MS_REFINE_R MS_REFINED ECHO_DOUBLES ECHO_CHUNK ECHO_MAX_LAG ECHO_MAX_PARAMS ECHO_PARAM_DOUBLES NED_DOUBLES NED_TILE
    NED_MAX_DELTA NED_MAX_THRESHOLDS NED_NAN_SILENT NED_NAN_NONFINITE NED_SLOTS REFL_DOUBLES REFL_FIELDS REFL_TILE
    REFL_MAX_HALF REFL_MAX_DIRECT REFL_MAX_BG REFL_MAX_KEEP REFL_MAX_SEP REFL_UNBOUNDED XSPEC_FRAMES XSPEC_ROWS
    XSPEC_MIN_FFT XSPEC_MAX_FFT FDW_FIELDS FDW_SUMS FDW_MAX_POINTS FDW_MAX_HALF FDW_CHUNK FDW_NARROW_HALF FDW_WINDOWS
    BURST_STEPS BURST_LANES BURST_CHANNELS BURST_MAX_STEPS BURST_MAX_DELTA BURST_MAX_OUT_BYTES MINPHASE_FIELDS
    MINPHASE_MAX_LOG2 MINPHASE_MIN_N MINPHASE_MIN_FLOOR_DB MINPHASE_SCRATCH_BYTES""".split()
FUNCTIONS = """xspec_frames ned_positions ned_tile_positions refl_row_room refl_tile_candidates refl_scratch_doubles fdw_chunks
    fdw_scratch_doubles burst_table_offsets burst_table_doubles minphase_scratch_bytes lundeby_layout multislope_slot_doubles
    multislope_jobs flat same_rows whole_numbers segment_tables point_grid window_weights""".split()
# the two functions that apply a budget: engine's read engine.BURST_MAX_OUT_BYTES / engine.MINPHASE_SCRATCH_BYTES at the call,
# where tests and tools set them; engine_geometry's take the budget as an argument
BUDGETED = ("burst_channels_per_call", "minphase_cut")


def test_engine_reexports_the_geometry():
    for name in CONSTANTS + FUNCTIONS:
        assert getattr(engine, name) is getattr(G, name), name
    assert engine.burst_channels_per_call(240, 61) == G.burst_channels_per_call(240, 61) == (256 << 20) // (16 * 240 * 61)
    assert engine.minphase_cut([1 << 21] * 100) == G.minphase_cut([1 << 21] * 100) == [(0, 46), (46, 92), (92, 100)]
    assert G.burst_channels_per_call(240, 61, 16 * 240 * 61 * 3 + 5) == 3 and G.minphase_cut([256] * 3, 2 * (44 * 256 + 64)) == [(0, 2), (2, 3)]
    assert engine.Engine.burst_channels_per_call is engine.burst_channels_per_call
    assert all(callable(getattr(G, name)) for name in BUDGETED)


def test_geometry_imports_without_torch_or_the_library():
    code = ("import sys; import audio_analysis_amd.engine_geometry as G; "
            "bad = [m for m in ('torch', 'audio_analysis_amd._lib', 'audio_analysis_amd.engine') if m in sys.modules]; "
            "assert not bad, bad; assert G.fdw_chunks([127, 128]).tolist() == [0, 1]")
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_flat_and_same_rows():
    a = G.flat([[1, 2], [3, 4]], np.int32)
    assert a.dtype == np.int32 and a.shape == (4,) and a.flags.c_contiguous and G.flat([], np.float64).shape == (0,)
    assert G.flat(np.arange(6)[::2], np.int64).flags.c_contiguous
    assert G.same_rows("m", [], [], np.zeros(0)) == 0 and G.same_rows("m", [1, 2, 3]) == 3 and G.same_rows("m", [1, 2], (3, 4)) == 2
    for tables in (([1, 2], [1]), ([], [1]), ([1], [1], [1, 2])):
        with pytest.raises(ValueError, match="^these must be .n,.$"):
            G.same_rows("these must be (n,)", *tables)


def test_whole_numbers():
    assert G.whole_numbers([], 1, 2) and G.whole_numbers([1, 2.0, 5], 1, 5) and G.whole_numbers([[-3, 3]], -3, 3)
    assert not G.whole_numbers([1.5], 1, 5) and not G.whole_numbers([0], 1, 5) and not G.whole_numbers([6], 1, 5)
    assert not G.whole_numbers([np.nan], 1, 5) and not G.whole_numbers([np.inf], 1, 5)
    assert G.whole_numbers([[1, 3], [1, 7]], 1, np.array([3, 7])[:, None])           # a bound per row
    assert not G.whole_numbers([[1, 4], [1, 7]], 1, np.array([3, 7])[:, None])


def test_segment_tables():
    off, ln, ch = G.segment_tables([0, 10], (10, 5), np.array([0.0, 1.0]))
    assert (off.dtype, ln.dtype, ch.dtype) == (np.int64, np.int64, np.int32) and ch.tolist() == [0, 1]
    assert all(v.shape == (0,) for v in G.segment_tables([], [], []))
    lay = G.lundeby_layout([0, 10], [10, 5], [0, 1], [2, 2], [5, 2], [1, 1])
    assert lay["chan_of_seg"].dtype == np.int32 and lay["nseg"] == 2 and lay["table_doubles"] == 12
    assert G.lundeby_layout([], [], [], [], [], [])["nseg"] == 0
    with pytest.raises(ValueError, match="one entry per row"):
        G.lundeby_layout([0, 10], [10], [0, 1], [2, 2], [5, 2], [1, 1])


def test_point_grid_edges():
    rho = np.array([0.5, 0.25])
    half = G.point_grid(rho, [1, G.FDW_MAX_HALF], "hann")
    assert half.dtype == np.int32 and half.tolist() == [1, G.FDW_MAX_HALF]
    assert G.point_grid(np.zeros(0), [], "rect").shape == (0,)                         # no point: nothing to check but the window
    assert G.point_grid(rho, np.array([[3.0], [4.0]]), "rect").tolist() == [3, 4]
    with pytest.raises(ValueError, match="rho and half must be"):
        G.point_grid(rho, [1], "hann")
    with pytest.raises(ValueError, match="rho and half must be"):
        G.point_grid(np.zeros(0), [1], "hann")
    for bad in (0, G.FDW_MAX_HALF + 1, 1.5, np.nan):
        with pytest.raises(ValueError, match=f"half must be whole numbers 1..{G.FDW_MAX_HALF}"):
            G.point_grid(rho, [1, bad], "hann")
    for bad in (0.0, np.nextafter(0.5, 1.0), np.nan, np.inf, -0.25):
        with pytest.raises(ValueError, match="rho must be finite and in"):
            G.point_grid(np.array([0.25, bad]), [1, 1], "hann")
    with pytest.raises(ValueError, match="window must be one of"):
        G.point_grid(rho, [1, 1], "hamming")
    with pytest.raises(ValueError, match="window must be one of"):
        G.point_grid(np.zeros(0), [], "hamming")
    full = np.full(G.FDW_MAX_POINTS, 0.25)
    assert G.point_grid(full, np.ones(G.FDW_MAX_POINTS), "hann").size == G.FDW_MAX_POINTS
    with pytest.raises(ValueError, match=f"at most {G.FDW_MAX_POINTS} frequency points, got {G.FDW_MAX_POINTS + 1}"):
        G.point_grid(np.full(G.FDW_MAX_POINTS + 1, 0.25), np.ones(G.FDW_MAX_POINTS + 1), "hann")
    # the order the launchers had: sizes, the count, the window, rho, half
    with pytest.raises(ValueError, match="window must be one of"):
        G.point_grid(np.array([0.0]), [0], "hamming")
    with pytest.raises(ValueError, match="rho must be finite"):
        G.point_grid(np.array([0.0]), [0], "hann")


def test_window_weights_edges():
    w = G.window_weights([[1, 2, 3]], 1, "delta")
    assert w.dtype == np.float64 and w.shape == (3,)
    for bad in ([1.0, 0.0, 1.0], [1.0, np.nan, 1.0], [1.0, np.inf, 1.0], [1.0, -1.0, 1.0], [1.0, 1.0], [1.0] * 4, []):
        with pytest.raises(ValueError, match=r"^weights must be 2 \* delta \+ 1 finite values > 0$"):
            G.window_weights(bad, 1, "delta")
    with pytest.raises(ValueError, match=r"^weights must be 2 \* half \+ 1 finite values > 0$"):
        G.window_weights([1.0], 1, "half")


@pytest.mark.parametrize("shape", [(0, 5), (3, 0, 6), (2, 3)])
def test_out_view_is_a_view_of_a_live_buffer(shape):
    eng = HostEngine()
    t = eng.torch
    n = int(np.prod(shape))
    view = eng.out_view(t.float64, *shape)
    assert tuple(view.shape) == shape and view.dtype == t.float64
    assert _ptr(view) != 0 and eng._pointee(_ptr(view)) == ("empty", max(n, 1), "torch.float64", 0)
    plain = eng.empty(n, t.float64)
    assert eng._pointee(_ptr(plain))[:3] == eng._pointee(_ptr(view))[:3]                # the record empty() gives
    assert len(eng._live) == 2 and eng.record == []
    if n:
        view[-1, -1] = 7.0
        assert float(eng._live[0][3][n - 1]) == 7.0                                    # it is the buffer's memory


def test_out_view_reaches_the_library_as_the_buffer_did():
    eng = HostEngine()
    b = eng.upload([])
    on, _, _ = eng.onset_index(b, 1e-4)
    out = eng.energy_windows(b.x, b.off, b.length, np.zeros(0, np.int32), on, np.zeros((0, 2), np.int64))
    args = eng.calls("ira_energy_windows")[0][1]
    assert tuple(out.shape) == (0, 4) and args[10] == ("empty", 1, "torch.float64", 0)   # not NULL: the library refuses that
