"""
The burst-decay map on the device (ira_burst_table, ira_burst_decay; audio_analysis_amd.analyse.burstdecay) against the
long-double restatement of tests/fdw_ref.py: a cell is fdw_ref.reference(x, p + delta, rho, H, window), held to
  |S - ref| <= (N + 16) u A        and a table entry to        |g(k) - ref| <= 16 u w(k)        (u = 2^-53)
at half widths on both sides of a round of IRA_BURST_LANES = 64 terms (63 | 65 terms, last rounds of one and of three
terms, one round | many), at step counts on both sides of a tile of IRA_BURST_STEPS = 8 steps, with steps that are
negative, zero, positive, equal, one sample and thousands of samples apart, at whole, clipped and empty windows, with
non-finite samples, across calls and batches bit for bit, against the table through a unit impulse, against
ira_fdw_response, and through the module and its command line.
Channels lie in one buffer with runs of NaN between them, at odd offsets: a term read from outside its channel would turn
the cell it enters into NaN.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import burstdecay_ref as B
import fdw_ref as R
from oracle import ira_oracle as O

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
LD = np.longdouble
U = 2.0 ** -53
T = 8                                                          # IRA_BURST_STEPS
# 2 H + 1 on both sides of one round (63 | 65 terms), of two and of four; last rounds of ONE term (H = 32, 64, 128, 2048:
# 64 q + 1 terms) and of three (H = 33, 65, 129); 1000: 31 rounds and 17 terms
HALVES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000, 2048]
RHOS = [1e-6, 0.1234567, 0.5]
# negative, zero, positive; equal neighbours (-3 -3, 0 0, 500 500); one sample apart; further apart than any window here
DELTAS = [-700, -3, -3, -2, 0, 0, 1, 2, 63, 64, 65, 500, 500, 5000, 5001, 12000, 20000]
STEP_COUNTS = [1, 2, T - 1, T, T + 1, 2 * T + 1]
GUARD = 7                                                      # NaN samples in front of every channel (odd offsets)
CELLS = B.Cells()


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def table(halves=HALVES, rhos=RHOS):
    return (np.array([r for h in halves for r in rhos], dtype=np.float64),
            np.array([h for h in halves for _ in rhos], dtype=np.int32))


def run(eng, chans, centres, rho, half, delta, window, guard=GUARD):
    """Engine level: one buffer, one table call, one map call.  Returns the (nch, J, M, 2) sums and the host copy of the
    table as a list of (2 H + 1, 2) arrays."""
    parts, offs, pos = [], [], 0
    for x in chans:
        parts += [np.full(guard, np.nan, np.float32), np.asarray(x, dtype=np.float32)]
        offs.append(pos + guard)
        pos += guard + len(x)
    parts.append(np.full(guard, np.nan, np.float32))
    x_dev = eng.to_dev(np.concatenate(parts))
    centre_dev = eng.to_dev(np.asarray(centres, dtype=np.int64))
    tab = eng.burst_table(rho, half, window)
    delta = np.asarray(delta)
    if delta.ndim == 1:
        delta = np.broadcast_to(delta, (len(rho), delta.size))
    outs = eng.burst_decay(x_dev, np.array(offs), np.array([len(x) for x in chans]), centre_dev, tab, delta)
    assert len(outs) == 1
    flat = tab.table.cpu().numpy()[: tab.doubles].reshape(-1, 2)
    tables = [flat[o : o + 2 * int(h) + 1] for o, h in zip(tab.offsets, tab.half)]
    return outs[0].cpu().numpy(), tables


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def hold(got, key, x, p, rho, half, delta, window, what):
    """Every cell of one channel's (J, M, 2) sums against the restatement; returns the worst error / bound."""
    worst = 0.0
    delta = np.broadcast_to(delta, (len(rho), np.shape(delta)[-1]))
    for j in range(len(rho)):
        for m in range(delta.shape[1]):
            ref = CELLS.ref(key, x, p + int(delta[j, m]), rho[j], int(half[j]), window)
            if ref["n"] == 0:
                assert not got[j, m].any(), (what, j, m, got[j, m])
            ratio = B.cell_ratio(got[j, m, 0], got[j, m, 1], ref)
            assert ratio <= 1.0, (what, j, m, int(half[j]), float(rho[j]), int(delta[j, m]), ratio, got[j, m])
            worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("window", R.WINDOWS)
def test_half_widths_and_step_counts_on_both_sides_of_every_boundary(window):
    rng = np.random.default_rng(201)
    rho, half = table()
    n = 30011
    chans = [rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * np.exp(-np.arange(n) / 900.0)).astype(np.float32)]
    centres = [9000, 700]                                       # whole windows; windows clipped at the front (H >= 1000, delta < 0)
    eng = _eng()
    full, tables = run(eng, chans, centres, rho, half, DELTAS, window)
    assert full.shape == (2, len(rho), len(DELTAS), 2)
    worst = [hold(full[c], c, chans[c], centres[c], rho, half, DELTAS, window, f"channel {c}") for c in range(2)]
    worst_table = max(B.table_ratio(tables[j], rho[j], int(half[j]), window) for j in range(len(rho)))
    print(f"half widths, {window}: worst cell error / bound {worst[0]:.4f} (whole), {worst[1]:.4f} (clipped); worst table "
          f"error {16 * worst_table:.2f} u w(k)")
    assert worst_table <= 1.0
    # equal neighbouring steps are the same cell, bit for bit
    for a, b in ((1, 2), (4, 5), (11, 12)):
        assert DELTAS[a] == DELTAS[b] and np.array_equal(bits(full[:, :, a]), bits(full[:, :, b]))
    # fewer steps: other tiles, the same cells, bit for bit
    for count in STEP_COUNTS[:-1]:
        got, _ = run(eng, chans, centres, rho, half, DELTAS[:count], window)
        assert got.shape[2] == count and np.array_equal(bits(got), bits(full[:, :, :count])), count
    assert len(DELTAS) == STEP_COUNTS[-1]


@pytest.mark.parametrize("window", R.WINDOWS)
def test_clipped_and_empty_windows(window):
    rng = np.random.default_rng(202)
    wide = 1000
    rho, half = table([1, 33, 129, wide], [0.1234567, 0.5])
    n = 2 * wide                                                # one shorter than the widest window
    x = rng.standard_normal(n).astype(np.float32)
    centres = [0, n - 1, n, n + wide + 3 + 40, -5, -wide - 1 - 40, n // 2]
    chans = [x] * len(centres) + [x[:0], x[:1], x[:1], x[:2], x[:2]]
    centres += [0, 0, 1, 0, 1]
    delta = [-40, -3, 0, 0, 1, 40, 700, 3 * wide + 100]
    got, _ = run(_eng(), chans, centres, rho, half, delta, window)
    for c, (xc, p) in enumerate(zip(chans, centres)):
        hold(got[c], ("clip", len(xc)), xc, p, rho, half, delta, window, f"channel {c} (length {len(xc)}, centre {p})")
    assert not got[2][:, -1].any() and not got[3][:, :6].any() and not got[5][:, :2].any() and not got[7].any()
    assert got[0, 0, 2].any() and got[8, 0, 2].any() and not got[8, 0, 5].any()   # one sample: inside at delta 0, not at 40
    assert np.isfinite(got).all()


@pytest.mark.parametrize("window", R.WINDOWS)
def test_table_entries_against_long_double(window):
    rho, half = table(HALVES + [12288], RHOS)
    x = np.zeros(8, np.float32)
    _, tables = run(_eng(), [x], [0], rho, half, [0], window)
    worst = 0.0
    for j in range(len(rho)):
        assert tables[j].shape == (2 * int(half[j]) + 1, 2)
        worst = max(worst, B.table_ratio(tables[j], rho[j], int(half[j]), window))
        if window == "rect":                                     # |g| = 1 to the sine's and the cosine's roundings
            assert np.max(np.abs(np.hypot(tables[j][:, 0], tables[j][:, 1]) - 1.0)) <= 4 * U
        assert tables[j][int(half[j]), 0] == 1.0 and tables[j][int(half[j]), 1] == 0.0   # k = 0
    print(f"table, {window}: worst error {16 * worst:.2f} u w(k)")
    assert worst <= 1.0


@pytest.mark.parametrize("window", R.WINDOWS)
def test_unit_impulse_gives_the_table_entry(window):
    """x = the unit impulse at p: S[j, m] = g_j(-delta[j, m]) as a value, exactly 0 where |delta| > H."""
    rho, half = table()
    n, p = 30001, 12345
    x = np.zeros(n, np.float32)
    x[p] = 1.0
    got, tables = run(_eng(), [x], [p], rho, half, DELTAS, window)
    for j in range(len(rho)):
        h = int(half[j])
        for m, d in enumerate(DELTAS):
            if abs(d) > h:
                assert got[0, j, m, 0] == 0.0 and got[0, j, m, 1] == 0.0, (j, m)
            else:
                assert got[0, j, m, 0] == tables[j][h - d, 0] and got[0, j, m, 1] == tables[j][h - d, 1], (j, m, d, h)
        assert got[0, j, 4, 0] == 1.0 and got[0, j, 4, 1] == 0.0    # t = 0: 0 dB at every frequency


@pytest.mark.parametrize("window", R.WINDOWS)
def test_fdw_response_of_a_unit_impulse_is_the_table_entry(window):
    """What csrc/ira_wavelet.h holds by construction, as a value: for a channel that is zero but for x[p + k] = 1,
    ira_fdw_response at the point (rho, H) returns (Re S0, Im S0) equal to entry k of ira_burst_table for that point and
    window (np.array_equal: signed zeros are equal), A = |w(k)| and N = 2 H + 1.  One term is summed into zeros,
    fma(v, cs, 0) is v * cs rounded once, and the sums of every other lane and chunk are exact zeros.  H: the last narrow
    point, the first wide one, one full chunk of IRA_FDW_CHUNK terms, a second chunk of a single term.  The weight itself is
    read from the table where the phasor is exactly +-1 or +-i: at rho = 0.5 (every k) and rho = 0.25 (odd k)."""
    eng = _eng()
    rho = np.array([0.5, 0.25, 1.0 / 3.0, 20.0 / 48000.0])
    for h in (1, 127, 128, 2047, 2048):
        ks = [-h, -1, 0, 1, h]
        half = np.full(rho.size, h, dtype=np.int32)
        chans = np.zeros((len(ks), 2 * h + 1), np.float32)
        chans[np.arange(len(ks)), h + np.array(ks)] = 1.0
        x_dev = eng.to_dev(np.concatenate([np.full(GUARD, np.nan, np.float32), chans.reshape(-1)]))
        off = GUARD + np.arange(len(ks), dtype=np.int64) * (2 * h + 1)
        centre_dev = eng.to_dev(np.full(len(ks), h, dtype=np.int64))
        got = eng.fdw_response(x_dev, off, np.full(len(ks), 2 * h + 1), centre_dev, rho, half, window).cpu().numpy()
        tab = eng.burst_table(rho, half, window)
        entries = tab.table.cpu().numpy()[: tab.doubles].reshape(rho.size, 2 * h + 1, 2)
        for c, k in enumerate(ks):
            w = abs(entries[0, h + k, 0])                        # rho = 0.5: the phasor is (+-1, 0)
            assert entries[0, h + k, 1] == 0.0 and (w == 1.0 if window == "rect" else 0.0 < w <= 1.0), (h, k, w)
            if k % 2:
                assert entries[1, h + k, 0] == 0.0 and abs(entries[1, h + k, 1]) == w, (h, k)   # rho = 0.25: (0, +-1)
            for j in range(rho.size):
                assert np.array_equal(got[c, j, :2], entries[j, h + k]), (window, h, float(rho[j]), k, got[c, j], entries[j, h + k])
                assert got[c, j, 4] == w and got[c, j, 5] == 2 * h + 1, (window, h, float(rho[j]), k, got[c, j], w)


def test_a_cell_does_not_depend_on_the_call_or_the_batch():
    rng = np.random.default_rng(204)
    rho, half = table([2, 33, 129, 1000], [0.1234567, 0.5])
    eng = _eng()
    x = rng.standard_normal(9001).astype(np.float32)
    others = [rng.standard_normal(n).astype(np.float32) for n in (12345, 1, 30001, 777, 5000)]
    for window in R.WINDOWS:
        alone, _ = run(eng, [x], [4200], rho, half, DELTAS, window)
        again, _ = run(eng, [x], [4200], rho, half, DELTAS, window)
        assert np.array_equal(bits(alone), bits(again))
        for m in (0, 6, 7, 8, 16):                                             # a call with that single step
            one, _ = run(eng, [x], [4200], rho, half, DELTAS[m : m + 1], window)
            assert np.array_equal(bits(one[0, :, 0]), bits(alone[0, :, m])), (window, m)
        for j in (0, 3, 7):                                                     # a call with that single point
            one, _ = run(eng, [x], [4200], rho[j : j + 1], half[j : j + 1], DELTAS, window)
            assert np.array_equal(bits(one[0, 0]), bits(alone[0, j])), (window, j)
        for place, guard in ((0, 7), (2, 1), (4, 2), (5, 3)):                   # other places, other alignments
            chans = others[:place] + [x] + others[place:] + [x]
            centres = [int(c) for c in rng.integers(-50, 12000, len(chans))]
            centres[place] = centres[-1] = 4200
            got, _ = run(eng, chans, centres, rho, half, DELTAS, window, guard=guard)
            assert np.array_equal(bits(got[place]), bits(alone[0])), (window, place)
            assert np.array_equal(bits(got[-1]), bits(alone[0])), (window, place)


def test_a_non_finite_sample_reaches_exactly_the_cells_whose_window_covers_it():
    rng = np.random.default_rng(205)
    rho, half = table([1, 100, 199, 200, 201, 1029, 1030, 1031], [0.1234567])
    n, p = 8000, 4000
    a, b, clean = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    a[p + 200] = np.nan
    b[p - 1030] = np.inf
    delta = np.array([-900, -1, 0, 0, 1, 2, 199, 200, 201, 400, 1231, 3000])
    for window in R.WINDOWS:
        got, _ = run(_eng(), [a, b, clean], [p, p, p], rho, half, delta, window)
        bad = ~np.isfinite(got).all(axis=3)
        h = half.astype(np.int64)[:, None]
        assert np.array_equal(bad[0], np.abs(delta[None, :] - 200) <= h), window
        assert np.array_equal(bad[1], np.abs(delta[None, :] + 1030) <= h), window
        assert not bad[2].any()
        for c, x in enumerate((a, b, clean)):                                     # the other cells are the usual sums
            for j in range(len(rho)):
                for m in np.flatnonzero(~bad[c, j]):
                    ref = CELLS.ref(("nf", c), x, p + int(delta[m]), rho[j], int(half[j]), window)
                    assert B.cell_ratio(got[c, j, m, 0], got[c, j, m, 1], ref) <= 1.0, (window, c, j, m)


def test_ms_axis_hann_columns_against_the_fdw_response():
    """On the ms axis every step is one ira_fdw_response call with the centres p + delta_m: both hold the restatement's
    bound, so they lie within its double of each other."""
    from audio_analysis_amd.analyse import burstdecay as D
    rng = np.random.default_rng(206)
    eng = _eng()
    st = D.BurstDecaySettings(axis="ms", stop=12.0, step=2.0, points_per_octave=2, f_min_hz=100.0, max_window_ms=30.0)
    f, rho, half, t, delta = D.burst_grid(st, 48000)
    assert t.size == 7 and half.max() == 1440 and list(delta[0]) == [0, 96, 192, 288, 384, 480, 576]
    chans = [(rng.standard_normal(n) * np.exp(-np.arange(n) / 700.0)).astype(np.float32) for n in (6000, 3001)]
    centres = [40, 1500]
    got, _ = run(eng, chans, centres, rho, half, delta, "hann")
    for m in range(t.size):
        parts, offs, pos = [], [], 0
        for x in chans:
            parts += [np.full(GUARD, np.nan, np.float32), x]
            offs.append(pos + GUARD)
            pos += GUARD + len(x)
        x_dev = eng.to_dev(np.concatenate(parts))
        centre_dev = eng.to_dev(np.asarray(centres, dtype=np.int64) + int(delta[0, m]))
        col = eng.fdw_response(x_dev, np.array(offs), np.array([len(x) for x in chans]), centre_dev, rho, half, "hann").cpu().numpy()
        for c in range(2):
            for j in range(len(rho)):
                ref = CELLS.ref(("ms", c), chans[c], centres[c] + int(delta[j, m]), rho[j], int(half[j]), "hann")
                assert col[c, j, 5] == ref["n"]
                gap = np.hypot(LD(got[c, j, m, 0]) - LD(col[c, j, 0]), LD(got[c, j, m, 1]) - LD(col[c, j, 1]))
                assert gap <= 2 * LD(ref["n"] + 16) * LD(U) * ref["a"], (m, c, j, float(gap))


# ------------------------------------------------------------------------------------------------ module level
def _module_case(sample_rate_hz, lengths):
    from audio_analysis_amd.synth import synth_ir
    return [synth_ir(30 + i, 0, n, sample_rate_hz) for i, n in enumerate(lengths)]


SMALL = dict(cycles=6.0, points_per_octave=3, f_min_hz=100.0, max_window_ms=20.0, stop=4.0, step=0.5, start=-1.0)


def test_module_and_command_line_on_a_stereo_wav(tmp_path):
    """analyse_burst_decay_files and the command line on a two-channel file: every value is burst_arithmetic applied to the
    device's own sums, exactly; the sums hold the restatement's bound; the level lies within that bound's image in dB
    around the level burst_arithmetic gives for the restatement's sums, 20 log10(1 + (N + 16) u A / |S|) and 3e-14 dB for
    the host arithmetic's own roundings (as in test_gpu_fdw.py), at every cell with |S| / A > 1e-6; the JSON round trip."""
    from audio_analysis_amd.analyse import burstdecay as D
    eng = _eng()
    chans = _module_case(48000, (6000, 6000))
    wav = tmp_path / "room.wav"
    wav.write_bytes(O.recorder_wav_bytes(0.5 * np.stack(chans, axis=1).reshape(-1), 48000))
    st = D.BurstDecaySettings(window="rect", **SMALL)
    api = D.analyse_burst_decay_files([wav], st)
    assert [r.channel_name for r in api] == ["room.wav:left", "room.wav:right"]
    from audio_analysis_amd.analyse._common import wav_channels
    heard = [c for _, c in wav_channels(wav, False, expected_sample_rate_hz=48000)[1]]
    rec = D.burst_decay_device(eng, eng.upload(heard), 48000, st)
    f, rho, half, t, delta = D.burst_grid(st, 48000)
    assert t.size == 11 and t[0] == -1.0 and rec.sums.shape == (2, f.size, 11, 2)
    left_out = 0
    for c, (r, x) in enumerate(zip(api, heard)):
        peak = int(np.argmax(np.abs(x)))
        assert (r.centre, r.centre_samples, r.centre_seconds, r.axis, r.window) == ("peak", peak, peak / 48000, "periods", "rect")
        assert np.array_equal(r.frequencies_hz, f) and np.array_equal(r.half_samples, half) and np.array_equal(r.axis_values, t)
        want = D.burst_arithmetic(rec.sums[c], half, delta, f, t, "periods", peak, len(x), st.decay_db, st.magnitude_floor_db)
        for name, v in want.items():
            got = getattr(r, name)
            assert got.dtype == v.dtype and np.array_equal(got, v, equal_nan=v.dtype != bool), name
        ref_sums = np.zeros_like(rec.sums[c])
        refs = {}
        for j in range(f.size):
            for m in range(t.size):
                ref = refs[j, m] = R.reference(x, peak + int(delta[j, m]), rho[j], int(half[j]), "rect")
                assert B.cell_ratio(rec.sums[c, j, m, 0], rec.sums[c, j, m, 1], ref) <= 1.0, (c, j, m)
                ref_sums[j, m] = float(ref["re0"]), float(ref["im0"])
        restated = D.burst_arithmetic(ref_sums, half, delta, f, t, "periods", peak, len(x), st.decay_db, st.magnitude_floor_db)
        assert np.array_equal(restated["clipped"], r.clipped) and r.clipped.any() and not r.clipped.all()
        assert np.array_equal(np.isnan(restated["level_db"]), np.isnan(r.level_db))
        for (j, m), ref in refs.items():
            mag = np.hypot(ref["re0"], ref["im0"])
            if ref["n"] == 0 or not mag / ref["a"] > 1e-6:
                left_out += 1
                continue
            tol = 20.0 * np.log10(LD(1) + LD(ref["n"] + 16) * LD(U) * ref["a"] / mag) + LD(3e-14)
            assert abs(LD(r.level_db[j, m]) - LD(restated["level_db"][j, m])) <= tol, (c, j, m)
    print(f"module: {left_out} of {2 * f.size * t.size} cells left out (|S| / A <= 1e-6 or empty)")
    # the command line: the same text and the same JSON; --no-map drops the maps alone
    env = dict(os.environ, PYTHONPATH=str(REPO))
    out_json = tmp_path / "room.json"
    args = ["--cycles", "6", "--points-per-octave", "3", "--window", "rect", "--f-min", "100", "--max-window-ms", "20",
            "--start", "-1", "--stop", "4", "--step", "0.5"]
    r = subprocess.run([sys.executable, "-m", "analyse.burstdecay", "--input", str(wav), *args, "--json", str(out_json)],
                       capture_output=True, text=True, cwd=str(REPO), env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "NaN" not in out_json.read_text()
    doc = json.loads(out_json.read_text())
    assert doc == D.burst_decay_results_to_json(api) and r.stdout == D.summarise_burst_decay_text(api)
    back = D.burst_decay_results_from_json(doc)
    assert D.burst_decay_results_to_json(back) == doc and np.array_equal(back[1].level_db, api[1].level_db, equal_nan=True)
    assert len(doc["burst_decay"][0]["level_db"]) == f.size and len(doc["burst_decay"][0]["level_db"][0]) == 11


def test_defaults_and_the_onset_as_the_centre():
    """The default settings through the module on two channels (240 points, 61 steps): the unit impulse reads 0 dB at
    t = 0 at every frequency and never reaches -30 dB later than its own window; with centre "onset" the centre is the
    device's onset."""
    from audio_analysis_amd.analyse import burstdecay as D
    eng = _eng()
    x = np.zeros(30000, np.float32)
    x[777] = 1.0
    room = _module_case(48000, (30000,))[0]
    a, b = D.analyse_burst_decay_batch([x, room], 48000, ["impulse", "room"])
    assert a.level_db.shape == (240, 61) and a.centre_samples == 777 and np.all(a.level_db[:, 0] == 0.0)
    assert np.nanmax(a.relative_db) == 0.0 and np.all(a.peak_position == 0.0) and np.all(a.peak_level_db == 0.0)
    assert np.all(a.decay_periods <= 4.0 + 0.5) and np.isnan(a.level_db[:, 9:]).all()   # hann of 8 cycles: 0 past 4 periods
    f, rho, half, t, delta = D.burst_grid(D.BurstDecaySettings(), 48000)
    inside = D.terms_inside(b.centre_samples, delta, half, room.size)            # 30 periods of 20 Hz end past the channel
    assert b.centre_samples == int(np.argmax(np.abs(room))) and np.array_equal(np.isnan(b.level_db), inside == 0)
    assert np.isfinite(b.level_db[-1]).all() and np.isnan(b.level_db[0, -1]) and np.array_equal(b.clipped, inside < 2 * half[:, None] + 1)
    st = D.BurstDecaySettings(centre="onset", onset_db=-30.0, axis="ms", stop=10.0, points_per_octave=3)
    r = D.analyse_burst_decay_for_channel(room, 48000, "room", st)
    onset = int(eng.onset_index(eng.upload([room]), st.rel_energy)[0].cpu().numpy()[0])
    assert r.centre == "onset" and r.centre_samples == onset <= b.centre_samples and r.level_db.shape == (30, 6)
