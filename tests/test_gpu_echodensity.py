"""
The normalized echo density on the device (ira_echo_density, audio_analysis_amd.analyse.echodensity) against the
long-double NumPy restatement of tests/echodensity_ref.py.

Every profile value is held to echodensity_ref.bound: (2 W + 16) 2^-53 eta + ambiguous_weight / (A E) + one float32 ulp,
derived there; the ambiguous weight is asserted to be 0 at every position of these seeded inputs, so the bound is the
arithmetic's own.  Records are compared EXACTLY with what NumPy reduces from the device's own float32 profile.
"""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import echodensity_ref as R
from oracle import ira_oracle as O

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
SR = 48000
BIG = 1 << 31
DELTAS = (1, 2, 31, 32, 33, 480, 2048)


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def steps_for(delta):
    w = 2 * delta + 1
    return (1, 7, 48, 64, w, w + 5)


def run(eng, chans, onsets, delta, window, step, kmax=BIG, thresholds=(1.0,)):
    """Engine level: one batch, one call.  onsets: explicit int64 onsets per channel, or None for the device's own
    (-20 dB).  Returns (onsets, rows: the whole float32 row of every channel, records (nch, 8))."""
    from audio_analysis_amd.analyse.echodensity import window_weights
    b = eng.upload([np.asarray(c, dtype=np.float32) for c in chans])
    if onsets is None:
        on, _, _ = eng.onset_index(b, 10.0 ** (-20.0 / 10.0))
    else:
        on = eng.to_dev(np.asarray(onsets, dtype=np.int64))
    prof, poff, rec = eng.echo_density(b.x, b.off, b.length, on, window_weights(delta, window), delta, step, kmax, thresholds)
    prof = prof.cpu().numpy()
    room = [R.count(len(c), 0, step, kmax) for c in chans]
    assert list(poff) == list(np.cumsum([0] + room[:-1])) and prof.size == sum(room)
    return on.cpu().numpy(), [prof[o : o + r] for o, r in zip(poff, room)], rec.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_channel(x, o, delta, window, step, kmax, thresholds, row, rec, what):
    """The issue's conditions for one channel.  Returns (K, the worst error over its bound)."""
    from audio_analysis_amd.engine import NED_NAN_NONFINITE, NED_NAN_SILENT
    k = R.count(len(x), o, step, kmax)
    assert rec[0] == k, (what, rec[0], k)
    assert np.all(bits(row[k:]) == NED_NAN_SILENT), what                      # past K the row is NaN
    got = row[:k]
    eta, kind, amb, a = R.profile(x, o, delta, window, step, kmax)
    assert np.all(amb == 0), (what, "ambiguous samples: change the seed", int(np.argmax(amb != 0)))
    ok = kind == 0
    assert np.array_equal(np.isnan(got), ~ok), (what, int(np.argmax(np.isnan(got) != ~ok)))
    assert np.all(bits(got[kind == 1]) == NED_NAN_SILENT) and np.all(bits(got[kind == 2]) == NED_NAN_NONFINITE), what
    worst = 0.0
    if np.any(ok):
        ref = eta[ok].astype(np.float64)
        err = np.abs(got[ok].astype(np.float64) - ref)
        bound = R.bound(eta[ok], amb[ok], a[ok], delta)
        worst = float(np.max(err / bound))
        assert np.all(err <= bound), (what, int(np.argmax(err / bound)), worst)
    want = R.record(got, thresholds)
    assert np.array_equal(rec, want, equal_nan=True), (what, rec, want)
    assert rec[1] == int(np.sum(kind == 1)) and rec[2] == int(np.sum(kind == 2)), what
    return k, worst


INPUTS = {"gaussian": lambda n: R.decaying_gaussian(n, rt_samples=n / 2.0), "poisson": R.thickening_poisson,
          "dc": R.dc_offset, "tiny": R.tiny_values}


# ------------------------------------------------------------------------------------------------ 1. profile
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_profile_against_the_restatement_over_windows_and_steps(name):
    """Every delta x step x window kind on a 1500-sample signal: at one sample per step two tiles, clipped windows at
    both ends (W = 4097 is longer than the signal: every window is clipped on both sides), steps beyond the window."""
    eng = _eng()
    x = INPUTS[name](1500)
    worst = 0.0
    for delta in DELTAS:
        for step in steps_for(delta):
            for window in ("hann", "rect"):
                thr = (0.5, 1.0)
                on, rows, rec = run(eng, [x], [0], delta, window, step, thresholds=thr)
                k, w = check_channel(x, 0, delta, window, step, BIG, thr, rows[0], rec[0], (name, delta, step, window))
                worst = max(worst, w)
    print(f"{name}: worst error / bound {worst:.3f}")


def test_profile_of_the_long_signals_at_the_default_window():
    eng = _eng()
    g, p = R.decaying_gaussian(12000), R.thickening_poisson(20000)
    for window in ("hann", "rect"):
        on, rows, rec = run(eng, [g, p], None, 480, window, 48, thresholds=(0.5, 0.9, 1.0))
        assert list(on) == [R.onset_index(g), R.onset_index(p)]
        for c, x in enumerate((g, p)):
            check_channel(x, int(on[c]), 480, window, 48, BIG, (0.5, 0.9, 1.0), rows[c], rec[c], ("long", c, window))
        inner = rows[0][12 : int(rec[0][0]) - 12].astype(np.float64)
        assert abs(inner.mean() - 1.0) <= 0.02                              # Gaussian noise sits at 1
        q = int(rec[1][0]) // 4
        means = [float(rows[1][i * q : (i + 1) * q].mean()) for i in range(4)]
        assert means[0] < means[1] < means[2] < means[3] and rec[1][7] > rec[1][5] >= 0       # rising: 0.5 before 1.0
    # one sample per step: whole windows only in the middle tiles, all four positions of a thread at work
    on, rows, rec = run(eng, [g], [0], 480, "hann", 1)
    k, w = check_channel(g, 0, 480, "hann", 1, BIG, (1.0,), rows[0], rec[0], "gaussian, one sample per step")
    assert k == 12000


def test_the_longest_window():
    """W = 4097 on the 12 000-sample Gaussian: whole windows from an onset at 3000, 1100 positions at one sample per step
    (a full tile of the largest span and a second one), and every 7th sample over the whole channel."""
    eng = _eng()
    g = R.decaying_gaussian(12000)
    on, rows, rec = run(eng, [g], [3000], 2048, "hann", 1, kmax=1100)
    k, _ = check_channel(g, 3000, 2048, "hann", 1, 1100, (1.0,), rows[0], rec[0], "W 4097, step 1")
    assert k == 1100
    on, rows, rec = run(eng, [g], [0], 2048, "rect", 7)
    k, _ = check_channel(g, 0, 2048, "rect", 7, BIG, (1.0,), rows[0], rec[0], "W 4097, step 7")
    assert k == 1715


# ------------------------------------------------------------------------------------------------ 2. records
def test_records_equal_numpy_on_the_device_profile():
    eng = _eng()
    x = R.thickening_poisson(20000)
    for thr in ((1.0,), (0.3, 0.8), (0.2, 0.6, 1.0), (0.5, 50.0), ()):
        on, rows, rec = run(eng, [x, x[:5000]], [0, 7], 480, "hann", 48, thresholds=thr)
        for c, (sig, o) in enumerate(((x, 0), (x[:5000], 7))):
            k = R.count(len(sig), o, 48, BIG)
            want = R.record(rows[c][:k], thr)
            assert np.array_equal(rec[c], want, equal_nan=True), (thr, c, rec[c], want)
            assert np.all(rec[c][5 + len(thr):] == -1)
        if thr == (0.5, 50.0):
            assert rec[0][5] >= 0 and rec[0][6] == -1                       # eta never reaches 50: -1
        if thr == (0.2, 0.6, 1.0):
            assert 0 <= rec[0][5] < rec[0][6] < rec[0][7]
    # a maximum that occurs twice: the first index wins (constant rows of zeros: every position ties)
    flat = (0.25 * np.random.default_rng(1).choice([-1.0, 1.0], 3000)).astype(np.float32)
    on, rows, rec = run(eng, [flat], [0], 31, "rect", 1)
    assert rec[0][3] == 0.0 and rec[0][4] == 0 and rec[0][5] == -1


# ------------------------------------------------------------------------------------------------ 3. edges
def test_edges_of_the_position_grid():
    eng = _eng()
    g = R.decaying_gaussian(6000, seed=21)
    delta, w = 100, 201
    # onset at sample 0 (left-clipped windows), within delta of the end, and L - o around W
    onsets = [0, 6000 - 50, 6000 - (w - 1), 6000 - w, 6000 - (w + 1), 5999]
    for step in (1, 48):
        on, rows, rec = run(eng, [g] * len(onsets), onsets, delta, "hann", step)
        for c, o in enumerate(onsets):
            check_channel(g, o, delta, "hann", step, BIG, (1.0,), rows[c], rec[c], ("onset", o, step))
    # max_time_ms cutting K to 1
    from audio_analysis_amd.analyse import echodensity as D
    assert D.max_positions(0.0, SR, 48) == 1
    on, rows, rec = run(eng, [g], [100], delta, "hann", 48, kmax=1)
    assert check_channel(g, 100, delta, "hann", 48, 1, (1.0,), rows[0], rec[0], "kmax 1")[0] == 1
    res = D.analyse_echo_density_batch([g], SR, ["g"], D.EchoDensitySettings(max_time_ms=0.0, window_ms=201 / 48.0))
    assert len(res[0].profile) == 1 and res[0].status == 0
    # ragged lengths in one batch, an empty channel and a one-sample channel among them
    chans = [g[:4000], np.zeros(0, np.float32), np.array([0.5], np.float32), g[:201], g[:777], g]
    for step in (1, 7):
        on, rows, rec = run(eng, chans, None, delta, "rect", step, thresholds=(0.5, 1.0))
        for c, x in enumerate(chans):
            assert on[c] == R.onset_index(x)
            check_channel(x, int(on[c]), delta, "rect", step, BIG, (0.5, 1.0), rows[c], rec[c], ("ragged", c, step))
        assert rec[1][0] == 0 and np.isnan(rec[1][3]) and rec[1][4] == -1 and rec[2][0] == 1 and rec[2][3] == 0.0


def _tile_edge_counts(tile):
    return (tile - 1, tile, tile + 1, 2 * tile + 1)


@pytest.mark.parametrize("step", [1, 48])
def test_edges_of_the_tiles(step):
    """K one below, at and one above a tile of IRA_NED_TILE positions, and two tiles and one, at one sample and at 48
    samples per step.  At 48 samples per step a workgroup takes fewer positions at a time (engine.ned_tile_positions:
    the span of IRA_NED_TILE positions does not fit), so K is placed at the multiples of THAT tile as well.  The window
    is short (delta = 2) to keep the 98 000-sample signals of the first set cheap."""
    from audio_analysis_amd.engine import NED_TILE, ned_tile_positions
    eng = _eng()
    delta = 2
    sets = [_tile_edge_counts(NED_TILE)]
    if ned_tile_positions(delta, step) != NED_TILE:
        sets.append(_tile_edge_counts(ned_tile_positions(delta, step)))
        sets.append(_tile_edge_counts(ned_tile_positions(31, step)))
    base = R.decaying_gaussian((2 * NED_TILE + 1) * step + 10, seed=22, rt_samples=30000.0)
    for i, counts in enumerate(sets):
        d = 31 if i == 2 else delta
        o = 5
        chans = [base[: o + (k - 1) * step + 1] for k in counts]             # L - 1 - o == (K - 1) S
        on, rows, rec = run(eng, chans, [o] * len(chans), d, "hann", step)
        for c, k in enumerate(counts):
            assert check_channel(chans[c], o, d, "hann", step, BIG, (1.0,), rows[c], rec[c], ("tile", step, k))[0] == k
        # the same counts cut by kmax from one long channel
        for k in counts:
            on, rows, rec = run(eng, [base], [o], d, "hann", step, kmax=k)
            assert check_channel(base, o, d, "hann", step, k, (1.0,), rows[0], rec[0], ("kmax", step, k))[0] == k


# ------------------------------------------------------------------------------------------------ 4. degenerate inputs
def test_degenerate_inputs():
    from audio_analysis_amd.analyse import echodensity as D
    from audio_analysis_amd.engine import NED_NAN_NONFINITE, NED_NAN_SILENT
    eng = _eng()
    rng = np.random.default_rng(31)
    good = R.decaying_gaussian(6000, seed=32)
    zeros = np.zeros(3000, np.float32)
    burst = np.concatenate([np.zeros(2000, np.float32), R.decaying_gaussian(4000, seed=33)])
    burst[100] = 1e-5                                                       # -100 dB and less: the onset a low onset_db finds
    flat = [(a * rng.choice([-1.0, 1.0], 4000)).astype(np.float32) for a in (0.25, 0.3)]
    bad_nan, bad_inf = good.copy(), good.copy()
    bad_nan[3000], bad_inf[3100] = np.nan, np.inf
    delta, step = 100, 7
    chans = [good, zeros, burst, flat[0], flat[1], bad_nan, bad_inf, good]
    onsets = [0, 0, 100, 0, 0, 0, 0, 0]
    for window in ("hann", "rect"):
        on, rows, rec = run(eng, chans, onsets, delta, window, step)
        for c, x in enumerate(chans):
            check_channel(x, onsets[c], delta, window, step, BIG, (1.0,), rows[c], rec[c], ("degenerate", c, window))
        k = [int(r[0]) for r in rec]
        assert rec[1][1] == k[1] and np.all(bits(rows[1][: k[1]]) == NED_NAN_SILENT) and np.isnan(rec[1][3])
        # windows of pure zeros in the pre-delay: centres 100 + 7 j with 100 + 7 j + 100 < 2000, 101 was the only sample
        silent = [j for j in range(k[2]) if 100 + 7 * j - delta > 100 and 100 + 7 * j + delta < 2000]
        assert rec[2][1] == len(silent) > 200 and np.all(np.isnan(rows[2][silent])) and rec[2][2] == 0
        for c in (3, 4):                                                    # constant magnitude: 0 everywhere, bit for bit
            assert np.all(bits(rows[c][: k[c]]) == 0) and rec[c][3] == 0.0 and rec[c][5] == -1
        for c, at in ((5, 3000), (6, 3100)):                                # exactly the windows that hold the bad sample
            hit = np.array([abs(7 * j - at) <= delta for j in range(k[c])])
            assert np.array_equal(bits(rows[c][: k[c]]) == NED_NAN_NONFINITE, hit) and rec[c][2] == int(hit.sum()) >= 28
            assert np.array_equal(bits(rows[c][: k[c]])[~hit], bits(rows[0][: k[0]])[~hit])
        assert np.array_equal(bits(rows[7]), bits(rows[0])) and np.array_equal(rec[7], rec[0])      # the clean neighbour
    # through the module: status words, NaN in every value, the batch carries on
    st = D.EchoDensitySettings(window_ms=201 / 48.0, step_ms=7 / 48.0, onset_db=-130.0)
    res = D.analyse_echo_density_batch([good, zeros, burst, bad_nan, bad_inf, good[:150], good], SR, list("abcdefg"), st)
    assert [r.status for r in res] == [0, D.STATUS_SILENT, 0, D.STATUS_NON_FINITE, D.STATUS_NON_FINITE, D.STATUS_TOO_SHORT, 0]
    assert res[2].onset_samples == 100 and sum(math.isnan(v) for v in res[2].profile) > 200 and math.isfinite(res[2].eta_max)
    for r in (res[1], res[3], res[4], res[5]):
        assert math.isnan(r.eta_max) and math.isnan(r.tau_max_seconds) and all(math.isnan(v) for v in r.mixing_time_seconds)
        assert all(math.isnan(v) for v in r.profile)
    assert np.array_equal(bits(res[0].profile), bits(res[6].profile)) and res[0].eta_max == res[6].eta_max and math.isfinite(res[0].eta_max)
    text = D.summarise_echo_density_text(res)
    assert "Status: 1 (silent)" in text and "Status: 4 (non-finite)" in text and "Status: 2 (too short)" in text


# ------------------------------------------------------------------------------------------------ 5. invariance
def test_bit_identical_whatever_the_batch():
    from audio_analysis_amd.analyse import echodensity as D
    eng = _eng()
    x = R.thickening_poisson(20000, seed=41)
    o = R.onset_index(x)
    others = [R.decaying_gaussian(n, seed=50 + i) for i, n in enumerate((3001, 17, 9999, 1234))]
    for delta, step in ((480, 48), (480, 1), (31, 7)):
        _, alone, alone_rec = run(eng, [x], None, delta, "hann", step)
        _, again, again_rec = run(eng, [x], None, delta, "hann", step)
        assert np.array_equal(bits(alone[0]), bits(again[0])) and np.array_equal(alone_rec.view(np.uint64), again_rec.view(np.uint64))
        _, many, many_rec = run(eng, others + [x], None, delta, "hann", step)       # 14 251 samples in front: another alignment
        assert np.array_equal(bits(many[4]), bits(alone[0])), (delta, step)
        assert np.array_equal(many_rec[4].view(np.uint64), alone_rec[0].view(np.uint64)), (delta, step)
    # through analyse_echo_density_batch, split at MAX_BATCH_CHANNELS: the channel is the second of the second batch
    _, alone, alone_rec = run(eng, [x], None, 480, "hann", 48)
    fill = [R.decaying_gaussian(300 + i, seed=100 + i) for i in range(D.MAX_BATCH_CHANNELS + 1)]
    res = D.analyse_echo_density_batch(fill + [x], SR, [str(i) for i in range(len(fill) + 1)])
    r = res[-1]
    k = int(alone_rec[0][0])
    assert r.status == 0 and r.onset_samples == o and len(r.profile) == k
    assert r.profile.dtype == np.float32 and np.array_equal(bits(r.profile), bits(alone[0][:k]))
    assert r.eta_max == alone_rec[0][3] and r.tau_max_seconds == alone_rec[0][4] * 48 / SR
    assert r.mixing_time_seconds == (alone_rec[0][5] * 48 / SR,) and alone_rec[0][5] > 0


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_cli_on_a_stereo_wav_and_the_golden_bundle(tmp_path):
    from audio_analysis_amd.analyse import echodensity as D
    from audio_analysis_amd.analyse._common import wav_channels
    n = 20000
    st = np.stack([0.5 * R.thickening_poisson(n, seed=61), 0.5 * R.decaying_gaussian(n, seed=62)], axis=1)
    wav = tmp_path / "room.wav"
    wav.write_bytes(O.recorder_wav_bytes(st.reshape(-1), SR))
    env = dict(os.environ, PYTHONPATH=str(REPO))
    out_json = tmp_path / "room.json"
    r = subprocess.run([sys.executable, "-m", "analyse.echodensity", "--input", str(wav), "--thresholds", "0.5", "1.0",
                        "--json", str(out_json)], capture_output=True, text=True, cwd=str(REPO), env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    doc = json.loads(out_json.read_text())
    rows = doc["echo_density"]
    assert [d["channel_name"] for d in rows] == ["room.wav:left", "room.wav:right"]
    assert set(rows[0]) == {"channel_name", "sample_rate_hz", "onset_samples", "onset_seconds", "status", "window_ms",
                            "window", "window_samples", "step_seconds", "thresholds", "mixing_time_seconds", "eta_max",
                            "tau_max_seconds", "profile"}
    _, chans = wav_channels(wav, False, expected_sample_rate_hz=SR)         # the samples as the 16-bit file holds them
    for d, (_, x) in zip(rows, chans):
        o = R.onset_index(x)
        eta, kind, amb, a = R.profile(x, o, 480, "hann", 48)
        assert d["onset_samples"] == o and d["status"] == 0 and d["window_samples"] == 961 and d["step_seconds"] == 0.001
        assert len(d["profile"]) == eta.size and np.all(kind == 0) and np.all(amb == 0)
        bound = R.bound(eta, amb, a, 480)
        got = np.asarray(d["profile"], dtype=np.float64)
        assert np.all(np.abs(got - eta.astype(np.float64)) <= bound)
        j = int(np.argmax(eta))
        assert abs(d["eta_max"] - float(eta[j])) <= bound[j]
        for thr, t in zip(d["thresholds"], d["mixing_time_seconds"]):
            hit = np.flatnonzero(eta.astype(np.float64) >= thr)
            if hit.size == 0:
                assert t is None
            else:
                assert t is not None and abs(t - hit[0] * 0.001) <= 0.001 + 1e-12      # within one step
    assert rows[0]["mixing_time_seconds"][0] is not None and rows[0]["mixing_time_seconds"][0] > 0.01   # sparse at first
    assert r.stdout == D.summarise_echo_density_text(D.echo_density_results_from_json(doc))
    assert D.echo_density_results_to_json(D.echo_density_results_from_json(doc)) == doc
    # null for NaN: a threshold the profile never reaches; --no-profile leaves the profile out
    r = subprocess.run([sys.executable, "-m", "analyse.echodensity", "--input", str(wav), "--thresholds", "50", "--no-profile",
                        "--json", str(out_json)], capture_output=True, text=True, cwd=str(REPO), env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = json.loads(out_json.read_text())["echo_density"]
    assert all(d["mixing_time_seconds"] == [None] and "profile" not in d for d in rows) and "NaN" not in out_json.read_text()
    # the golden bundle through the native ingest: names "<tap>:<channel>", values equal to the file path's.  The 16-bit
    # taps decay into digital silence after some 5800 samples, so the profile is evaluated over the first 100 ms (the
    # last window ends at sample 5660 at the latest); over the whole file the tail is NaN, as the definition has it
    root = REPO / "tests" / "golden" / "bundle"
    first = D.EchoDensitySettings(max_time_ms=100.0)
    api = D.analyse_echo_density_bundle(root, first)
    taps = json.loads((root / "meta.json").read_text())["taps"]
    files = D.analyse_echo_density_files([root / "taps" / f"{t}.wav" for t in taps], first)
    whole = D.analyse_echo_density_bundle(root)
    assert all(r.status == 0 and np.isnan(r.profile[-1]) and len(r.profile) > 240 for r in whole)
    assert all(np.array_equal(bits(r.profile[:101]), bits(b.profile)) for r, b in zip(whole, api))
    assert [r.channel_name for r in api] == [f"{t}:{c}" for t in taps for c in ("left", "right")]
    assert len(api) == len(files) and all(r.status == 0 for r in api)
    for b, f in zip(api, files):
        assert np.array_equal(bits(b.profile), bits(f.profile)) and len(b.profile) == 101 and np.all(np.isfinite(b.profile))
        assert (b.eta_max, b.tau_max_seconds, b.onset_samples) == (f.eta_max, f.tau_max_seconds, f.onset_samples)
        assert np.array_equal(b.mixing_time_seconds, f.mixing_time_seconds, equal_nan=True)
