"""
The early-reflection detection on the device (ira_reflections, audio_analysis_amd.analyse.reflections) against the float64
NumPy restatement of tests/reflections_ref.py, BIT FOR BIT: the energy-time row (compared as uint64), the direct sound,
the candidate count, the first candidate, all six fields of every kept reflection and the count of non-finite row
entries.  The two energy sums of the direct-to-reverberant ratio may run in any fixed order, so they are held to
(n + 1) 2^-53 relative of the long-double sum of their n non-negative terms (n - 1 additions, one rounding each, and the
rounding of the reference's own conversion).
"""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import echodensity_ref as E
import reflections_ref as R
from oracle import ira_oracle as O

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
SR = 48000
BIG = R.UNBOUNDED
DEFAULTS = dict(d=24, window="hann", D=120, Dw=120, G=48, S=24, B=240, Tn=9600, rel=10.0 ** -4.0, prom=10.0 ** 0.6, keep=16)


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def cfg(**kw):
    return dict(DEFAULTS, **kw)


def run(eng, chans, onsets, c):
    """Engine level: one batch, one call.  onsets: explicit int64 onsets per channel, or None for the device's own
    (-20 dB).  Returns (onsets, rows: the whole float64 row of every channel, lists (nch, keep, 6), records (nch, 8))."""
    from audio_analysis_amd.analyse.echodensity import window_weights
    b = eng.upload([np.asarray(x, dtype=np.float32) for x in chans])
    if onsets is None:
        on, _, _ = eng.onset_index(b, 10.0 ** (-20.0 / 10.0))
    else:
        on = eng.to_dev(np.asarray(onsets, dtype=np.int64))
    erow, eoff, lst, rec = eng.reflections(b.x, b.off, b.length, on, window_weights(c["d"], c["window"]), c["d"], c["D"],
                                           c["Dw"], c["G"], c["S"], c["B"], c["Tn"], c["rel"], c["prom"], c["keep"])
    erow = erow.cpu().numpy()
    room = [R.row_room(len(x), c["D"], c["Tn"], c["B"]) for x in chans]
    assert list(eoff) == list(np.cumsum([0] + room[:-1])) and erow.size == sum(room)
    return on.cpu().numpy(), [erow[o : o + r] for o, r in zip(eoff, room)], lst.cpu().numpy(), rec.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_channel(x, o, c, row, lst, rec, what, flagged=False):
    """Every output of one channel against the float64 restatement, bit for bit.  flagged: the channel holds non-finite
    row entries -- the row and their count are compared, the decisions taken among NaNs are not.  Returns the restatement."""
    ref = R.detect(x, o, **c)
    want = ref["row"]
    assert np.array_equal(bits(row[: want.size]), bits(want)), (what, int(np.argmax(bits(row[: want.size]) != bits(want))))
    assert np.all(np.isnan(row[want.size:])), what                             # past R the row is NaN
    assert rec[7] == ref["nonfinite"], (what, rec[7], ref["nonfinite"])
    if flagged:
        assert rec[7] > 0
        return ref
    assert rec[0] == ref["n0"], (what, rec[0], ref["n0"])
    assert bits(rec[1]) == bits(ref["Ed"]) or (math.isnan(rec[1]) and math.isnan(ref["Ed"])), (what, rec[1], ref["Ed"])
    assert rec[2] == ref["M"] and rec[4] == ref["first"], (what, rec[2:5], ref["M"], ref["first"])
    kept = ref["kept"]
    assert rec[3] == len(kept) == min(ref["M"], c["keep"]), (what, rec[3], len(kept))
    if kept:
        got = lst[: len(kept)]
        assert np.array_equal(bits(got), bits(np.array(kept, dtype=np.float64))), (what, got, kept)
    unused = lst[len(kept):]
    assert np.all(unused[:, (0, 3, 4)] == -1.0) and np.all(np.isnan(unused[:, (1, 2, 5)])), what
    exact_dir, exact_rest, _ = R.energies(x, ref["n0"], c["Dw"]) if x.size else (0.0, 0.0, None)
    for k, name, terms, exact in ((5, "Edir", ref["terms"][0], exact_dir), (6, "Erest", ref["terms"][1], exact_rest)):
        if math.isfinite(float(exact)):
            assert abs(np.longdouble(rec[k]) - exact) <= (terms + 1) * np.longdouble(2.0) ** -53 * exact, (what, name, rec[k], exact)
    return ref


INPUTS = {"room": lambda: R.sparse_room(6000, 1), "gaussian": lambda: E.decaying_gaussian(5000),
          "poisson": lambda: E.thickening_poisson(8000)}

# d in (1, 24, 512), S in (1, 24) with G = S and G = 48, B in (S + 1, 240, 2048), keep in (1, 16, 64), both windows; a
# 0 dB prominence and a -60 dB floor where many candidates are wanted
CONFIGS = [cfg(),
           cfg(d=1, S=1, G=1, B=2, keep=1, window="rect", prom=1.0, rel=1e-6),
           cfg(d=512, S=24, G=24, B=2048, keep=64, Tn=BIG, prom=1.0, rel=1e-6),
           cfg(d=1, S=1, G=48, B=240, keep=64, Tn=BIG, prom=1.0, rel=1e-6),
           cfg(d=512, S=1, G=1, B=2048, keep=16, window="rect", prom=1.0, rel=1e-6),
           cfg(d=24, S=24, G=24, B=25, keep=1, window="rect", Tn=BIG, prom=1.0),
           cfg(d=24, S=1, G=48, B=2048, keep=64, Tn=3000, prom=1.0),
           cfg(d=1, S=24, G=48, B=25, keep=16, rel=1e-6)]


# ------------------------------------------------------------------------------------------------ 1. bit-exact
@pytest.mark.parametrize("i", range(len(CONFIGS)))
def test_bit_exact_against_the_float64_restatement(i):
    eng = _eng()
    c = CONFIGS[i]
    chans = [INPUTS[k]() for k in sorted(INPUTS)]
    on, rows, lst, rec = run(eng, chans, None, c)
    found = []
    for k, x in enumerate(chans):
        assert on[k] == R.onset_index(x)
        ref = check_channel(x, int(on[k]), c, rows[k], lst[k], rec[k], (i, sorted(INPUTS)[k]))
        found.append(ref["M"])
    print(f"config {i}: candidates {found}")
    if i == 0:
        assert found[2] == 5 and [int(v) for v in lst[2][:5, 0]] == [349, 555, 776, 1146, 2182]      # sorted: gaussian, poisson, room
    if c["prom"] == 1.0 and c["S"] == 1 and c["Tn"] == BIG:
        assert found[1] > c["keep"]                                          # the selection is at work


# ------------------------------------------------------------------------------------------------ 2. tile edges
def _pulses(n, at, seed=5):
    """Low Gaussian noise with a direct pulse at sample 10 and pulses of 0.4 at the samples `at`."""
    x = 1e-3 * np.random.default_rng(seed).standard_normal(n)
    x[10] = 1.0
    for a in at:
        if 0 <= a < n:
            x[a] = 0.4
    return x.astype(np.float32)


def test_edges_of_the_tiles():
    from audio_analysis_amd.engine import REFL_TILE
    eng = _eng()
    assert REFL_TILE == 1024
    o = 10
    counts = (REFL_TILE - 1, REFL_TILE, REFL_TILE + 1, 2 * REFL_TILE + 1)
    # R through L (no bound on the search), a reflection three entries before the row's end
    c = cfg(Tn=BIG)
    chans = [_pulses(o + r, [o + r - 3, o + 500]) for r in counts]
    on, rows, lst, rec = run(eng, chans, [o] * len(chans), c)
    for k, x in enumerate(chans):
        ref = check_channel(x, o, c, rows[k], lst[k], rec[k], ("R through L", counts[k]))
        assert ref["row"].size == counts[k] and ref["M"] >= 1
    # R through Tn on one long channel: R = D + Tn + B
    x = _pulses(6000, [o + 500, o + 1023, o + 2048])
    for r in counts:
        c = cfg(Tn=r - 120 - 240)
        on, rows, lst, rec = run(eng, [x], [o], c)
        ref = check_channel(x, o, c, rows[0], lst[0], rec[0], ("R through Tn", r))
        assert ref["row"].size == r
    # a candidate at the last entry of a tile, at the first of the next, its background across the boundary on both sides
    for at in (REFL_TILE - 1, REFL_TILE, 2 * REFL_TILE - 1, 2 * REFL_TILE):
        for c in (cfg(), cfg(B=2048, S=1, G=1, d=1), cfg(d=512, prom=1.0)):
            x = _pulses(4000, [o + at, o + at - 300, o + at + 300])
            on, rows, lst, rec = run(eng, [x], [o], c)
            ref = check_channel(x, o, c, rows[0], lst[0], rec[0], ("boundary", at, c["B"], c["d"]))
            assert o + at in [cand[0] for cand in ref["candidates"]], (at, c)


def test_edges_of_the_channel():
    eng = _eng()
    g = E.decaying_gaussian(3000, seed=21)
    # L < W: every window is clipped on both sides
    for c in (cfg(d=24), cfg(d=512, window="rect"), cfg(d=512, S=1, G=1, B=2, prom=1.0, rel=1e-6)):
        for n in (1, 2, 20, 48):
            on, rows, lst, rec = run(eng, [g[:n]], [0], c)
            check_channel(g[:n], 0, c, rows[0], lst[0], rec[0], ("L < W", n, c["d"]))
    # the onset at L - 1, L - G and L - G - 1 (the search range is empty, then one sample), D longer than L - o
    c = cfg(S=1, G=48, prom=1.0, rel=1e-9)
    L = 3000
    onsets = [L - 1, L - 48, L - 49, L - 50, L - 60, 0]
    on, rows, lst, rec = run(eng, [g] * len(onsets), onsets, c)
    for k, o in enumerate(onsets):
        ref = check_channel(g, o, c, rows[k], lst[k], rec[k], ("onset", o))
        if o >= L - 48:
            assert ref["M"] == 0 and ref["n0"] + 48 >= L
    # ragged lengths in one batch, an empty channel and a one-sample channel among them, the device's own onsets
    chans = [g[:2500], np.zeros(0, np.float32), np.array([0.5], np.float32), g[:49], g[:777], g]
    for c in (cfg(), cfg(Tn=BIG, S=1, G=1, B=2, prom=1.0)):
        on, rows, lst, rec = run(eng, chans, None, c)
        for k, x in enumerate(chans):
            assert on[k] == R.onset_index(x)
            check_channel(x, int(on[k]), c, rows[k], lst[k], rec[k], ("ragged", k))
        assert rows[1].size == 0 and rec[1][0] == 0 and math.isnan(rec[1][1]) and list(rec[1][2:]) == [0, 0, -1, 0, 0, 0]
        assert rec[2][0] == 0 and rec[2][1] == 0.25 and rec[2][5] == 0.25   # one sample: the centre weight is 1


# ------------------------------------------------------------------------------------------------ 3. selection
def test_selection():
    eng = _eng()
    p = E.thickening_poisson(8000)
    o = R.onset_index(p)
    for keep in (1, 16, 64):
        c = cfg(Tn=BIG, keep=keep, prom=1.0, rel=1e-6)
        on, rows, lst, rec = run(eng, [p], None, c)
        ref = check_channel(p, o, c, rows[0], lst[0], rec[0], ("M > keep", keep))
        assert ref["M"] > 64 and rec[0][3] == keep
        times = lst[0][:keep, 0]
        assert np.all(np.diff(times) > 0)                                    # in time order
        strongest = sorted(ref["candidates"], key=lambda q: (-q[1], q[0]))[:keep]
        assert sorted(q[0] for q in strongest) == [int(v) for v in times]
    # keep >= M
    room = R.sparse_room(6000, 1)
    for keep in (5, 6, 64):
        c = cfg(keep=keep)
        on, rows, lst, rec = run(eng, [room], None, c)
        ref = check_channel(room, 200, c, rows[0], lst[0], rec[0], ("keep >= M", keep))
        assert ref["M"] == 5 == rec[0][3]
    # M = 0 with min_level_db = 0: the first candidate is -1, the list all -1 / NaN
    c = cfg(rel=1.0)
    on, rows, lst, rec = run(eng, [room], None, c)
    check_channel(room, 200, c, rows[0], lst[0], rec[0], "M = 0")
    assert rec[0][2] == 0 and rec[0][3] == 0 and rec[0][4] == -1
    assert np.all(lst[0][:, (0, 3, 4)] == -1.0) and np.all(np.isnan(lst[0][:, (1, 2, 5)]))
    from audio_analysis_amd.analyse import reflections as D
    res = D.analyse_reflections_batch([room], SR, ["room"], D.ReflectionSettings(min_level_db=0.0))
    assert res[0].status == 0 and math.isnan(res[0].itdg_ms) and res[0].reflections == () and res[0].candidates_found == 0
    assert res[0].direct_samples == 200 and math.isfinite(res[0].drr_db)
    # two identical isolated pulses: equal e, the earlier one is kept
    twins = R.twin_pulses()
    c = cfg(keep=1)
    on, rows, lst, rec = run(eng, [twins], None, c)
    ref = check_channel(twins, 100, c, rows[0], lst[0], rec[0], "twins")
    assert rec[0][2] == 2 and rec[0][3] == 1 and lst[0][0][0] == 1500 and rec[0][4] == 1500
    assert ref["candidates"][0][1] == ref["candidates"][1][1]
    # a constant magnitude: the sums of whole windows are equal, there is no strict maximum; the direct sound is the onset
    flat = (0.25 * np.random.default_rng(1).choice([-1.0, 1.0], 3000)).astype(np.float32)
    for window in ("hann", "rect"):
        c = cfg(window=window)
        on, rows, lst, rec = run(eng, [flat, flat], [100, 0], c)
        for k, o in enumerate((100, 0)):
            check_channel(flat, o, c, rows[k], lst[k], rec[k], ("flat", window, o))
        assert rec[0][0] == 100 and rec[0][2] == 0 and rec[1][2] == 0


# ------------------------------------------------------------------------------------------------ 4. degenerate inputs
def test_degenerate_inputs_in_one_batch():
    from audio_analysis_amd.analyse import reflections as D
    eng = _eng()
    good = R.sparse_room(12000, 1)
    zeros = np.zeros(3000, np.float32)
    empty, one = np.zeros(0, np.float32), np.array([0.5], np.float32)
    nan_in, inf_in, nan_out, inf_out = good.copy(), good.copy(), good.copy(), good.copy()
    nan_in[1000], inf_in[1100] = np.nan, np.inf                             # inside the row of 9960 entries from sample 200
    nan_out[11000], inf_out[11500] = np.nan, np.inf                         # behind it: only the remaining energy sees them
    chans = [good, zeros, empty, one, nan_in, inf_in, nan_out, inf_out, good]
    onsets = [200, 0, 0, 0, 200, 200, 200, 200, 200]
    c = cfg()
    on, rows, lst, rec = run(eng, chans, onsets, c)
    for k, x in enumerate(chans):
        check_channel(x, onsets[k], c, rows[k], lst[k], rec[k], ("degenerate", k), flagged=k in (4, 5))
    assert rec[4][7] == 49 and rec[5][7] == 49                              # the windows that hold the bad sample
    assert rec[6][7] == 0 and rec[7][7] == 0 and math.isnan(rec[6][6]) and rec[7][6] == math.inf
    for k in (6, 7, 8):                                                     # the clean neighbour, and the rows the bad samples never reach
        assert np.array_equal(bits(rows[k]), bits(rows[0])) and np.array_equal(bits(lst[k]), bits(lst[0]))
        assert np.array_equal(bits(rec[k][:6]), bits(rec[0][:6]))
    assert np.array_equal(bits(rec[8]), bits(rec[0]))
    assert rec[1][2] == 0 and rec[1][1] == 0.0 and rec[1][0] == 0 and rec[2][3] == 0 and rec[3][5] == 0.25
    # through the module: status words, NaN in every value, the batch carries on
    res = D.analyse_reflections_batch([good, zeros, empty, one, nan_in, inf_in, good[:230], good], SR, list("abcdefgh"))
    assert [r.status for r in res[:2] + res[3:]] == [0, D.STATUS_SILENT, D.STATUS_TOO_SHORT, D.STATUS_NON_FINITE,
                                                     D.STATUS_NON_FINITE, D.STATUS_TOO_SHORT, 0]
    assert res[2].status & D.STATUS_TOO_SHORT and not res[2].status & D.STATUS_NON_FINITE      # the empty channel
    for r in res[1:7]:
        assert r.direct_samples == -1 and math.isnan(r.direct_seconds) and math.isnan(r.itdg_ms) and math.isnan(r.drr_db)
        assert r.reflections == () and r.candidates_found == 0 and np.all(np.isnan(r.curve))
    assert res[0].reflections == res[7].reflections and len(res[0].reflections) == 5 and res[0].drr_db == res[7].drr_db
    assert np.array_equal(res[0].curve.view(np.uint32), res[7].curve.view(np.uint32)) and res[0].direct_samples == 200
    text = D.summarise_reflections_text(res)
    assert "Status: 1 (silent)" in text and "Status: 4 (non-finite)" in text and "Status: 2 (too short)" in text


# ------------------------------------------------------------------------------------------------ 5. invariance
def test_bit_identical_whatever_the_batch():
    from audio_analysis_amd.analyse import reflections as D
    eng = _eng()
    x = E.thickening_poisson(8000, seed=41)
    others = [E.decaying_gaussian(n, seed=50 + i) for i, n in enumerate((3001, 17, 9999, 1234))]
    for c in (cfg(), cfg(Tn=BIG, S=1, G=1, B=2048, keep=64, prom=1.0, rel=1e-6), cfg(d=512, window="rect")):
        _, row_a, lst_a, rec_a = run(eng, [x], None, c)
        _, row_b, lst_b, rec_b = run(eng, [x], None, c)
        _, row_c, lst_c, rec_c = run(eng, others + [x], None, c)            # 14 251 samples in front: another alignment
        for row, lst, rec in ((row_b[0], lst_b[0], rec_b[0]), (row_c[4], lst_c[4], rec_c[4])):
            assert np.array_equal(bits(row), bits(row_a[0])) and np.array_equal(bits(lst), bits(lst_a[0]))
            assert np.array_equal(bits(rec), bits(rec_a[0]))
    # through analyse_reflections_batch, split at MAX_BATCH_CHANNELS: the channel is the second of the second batch
    room = R.sparse_room(6000, 1)
    alone = D.analyse_reflections_batch([room], SR, ["room"])[0]
    fill = [E.decaying_gaussian(300 + i, seed=100 + i) for i in range(D.MAX_BATCH_CHANNELS + 1)]
    res = D.analyse_reflections_batch(fill + [room], SR, [str(i) for i in range(len(fill) + 1)])
    r = res[-1]
    assert r.status == 0 and r.reflections == alone.reflections and len(r.reflections) == 5
    assert (r.direct_samples, r.itdg_ms, r.drr_db, r.candidates_found) == (alone.direct_samples, alone.itdg_ms, alone.drr_db, 5)
    assert np.array_equal(r.curve.view(np.uint32), alone.curve.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 6. end to end
def _expected(x, fs=SR):
    """What the module reports for a clean channel at the default settings, from the restatement."""
    o = R.onset_index(x)
    ref = R.detect(x, o, **DEFAULTS)
    n0, ed = ref["n0"], float(ref["Ed"])
    rows = []
    for n, e, bsum, cnt, m, xm in ref["kept"]:
        prom = math.inf if cnt == 0 or bsum == 0 else 10.0 * math.log10(float(e) * cnt / float(bsum))
        rows.append(dict(sample_index=n, peak_sample_index=m, delay_ms=1000.0 * (n - n0) / fs, level_db=10.0 * math.log10(float(e) / ed),
                         prominence_db=prom, polarity=int(np.sign(xm)), path_difference_m=343.0 * (n - n0) / fs))
    return dict(onset_samples=o, direct_samples=n0, candidates_found=ref["M"], reflections=rows,
                itdg_ms=1000.0 * (ref["first"] - n0) / fs if ref["first"] >= 0 else None,
                drr_db=10.0 * math.log10(float(ref["Edir"]) / float(ref["Erest"])), row=ref["row"], ed=ed)


def test_cli_on_a_stereo_wav_and_the_golden_bundle(tmp_path):
    from audio_analysis_amd.analyse import reflections as D
    from audio_analysis_amd.analyse._common import wav_channels
    st = np.stack([0.5 * R.sparse_room(12000, 1), 0.5 * R.sparse_room(12000, 3)], axis=1)
    wav = tmp_path / "room.wav"
    wav.write_bytes(O.recorder_wav_bytes(st.reshape(-1), SR))
    env = dict(os.environ, PYTHONPATH=str(REPO))
    out_json = tmp_path / "room.json"
    r = subprocess.run([sys.executable, "-m", "analyse.reflections", "--input", str(wav), "--json", str(out_json)],
                       capture_output=True, text=True, cwd=str(REPO), env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "NaN" not in out_json.read_text()
    doc = json.loads(out_json.read_text())
    rows = doc["reflections"]
    assert [d["channel_name"] for d in rows] == ["room.wav:left", "room.wav:right"]
    _, chans = wav_channels(wav, False, expected_sample_rate_hz=SR)         # the samples as the 16-bit file holds them
    for d, (_, x) in zip(rows, chans):
        want = _expected(x)
        assert d["status"] == 0 and d["window_samples"] == 49 and d["curve_step_seconds"] == 0.001
        for key in ("onset_samples", "direct_samples", "candidates_found"):
            assert d[key] == want[key], key
        assert d["direct_samples"] == 200 and d["candidates_found"] == 5 == len(d["reflections"])
        assert abs(d["itdg_ms"] - want["itdg_ms"]) <= 1e-9 and abs(d["drr_db"] - want["drr_db"]) <= 1e-9
        for got, ref in zip(d["reflections"], want["reflections"]):
            for key in ("sample_index", "peak_sample_index", "polarity"):
                assert got[key] == ref[key], key
            for key in ("delay_ms", "level_db", "prominence_db", "path_difference_m"):
                if ref[key] == math.inf:
                    assert got[key] == "+inf"
                else:
                    assert abs(got[key] - ref[key]) <= 1e-9, (key, got[key], ref[key])
        assert [q["polarity"] for q in d["reflections"]] == [1, -1, 1, 1, -1]
        with np.errstate(divide="ignore"):
            curve = (10.0 * np.log10(want["row"][::48] / want["ed"])).astype(np.float32)
        got = np.asarray([D.M.num_json(v) for v in d["curve"]], dtype=np.float32)
        assert got.size == curve.size == 208 and np.allclose(got, curve, rtol=0.0, atol=1e-5, equal_nan=True)
    assert r.stdout == D.summarise_reflections_text(D.reflections_results_from_json(doc))
    assert D.reflections_results_to_json(D.reflections_results_from_json(doc)) == doc
    # the one-file entry point: the same values under the plain channel names
    one = D.analyse_reflections_from_wav_file(wav)
    assert [q.channel_name for q in one] == ["left", "right"]
    named = D.reflections_results_to_json(one)["reflections"]
    assert [{k: v for k, v in d.items() if k != "channel_name"} for d in named] == \
        [{k: v for k, v in d.items() if k != "channel_name"} for d in rows]
    # --no-curve leaves the curve out
    r = subprocess.run([sys.executable, "-m", "analyse.reflections", "--input", str(wav), "--no-curve", "--json", str(out_json)],
                       capture_output=True, text=True, cwd=str(REPO), env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    slim = json.loads(out_json.read_text())["reflections"]
    assert all("curve" not in d for d in slim)
    assert [{k: v for k, v in d.items() if k != "curve"} for d in rows] == slim
    # the golden bundle through the native ingest: names "<tap>:<channel>", values equal to the file path's, bit for bit
    root = REPO / "tests" / "golden" / "bundle"
    api = D.analyse_reflections_bundle(root)
    taps = json.loads((root / "meta.json").read_text())["taps"]
    files = D.analyse_reflections_files([root / "taps" / f"{t}.wav" for t in taps])
    assert [r.channel_name for r in api] == [f"{t}:{c}" for t in taps for c in ("left", "right")]
    assert len(api) == len(files) and all(r.status == 0 for r in api)
    for b, f in zip(api, files):
        assert b.reflections == f.reflections and np.array_equal(b.curve.view(np.uint32), f.curve.view(np.uint32))
        assert (b.direct_samples, b.onset_samples, b.candidates_found) == (f.direct_samples, f.onset_samples, f.candidates_found)
        assert np.array_equal([b.itdg_ms, b.drr_db], [f.itdg_ms, f.drr_db], equal_nan=True)
