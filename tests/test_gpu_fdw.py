"""
The frequency-dependent-window sums on the device (ira_fdw_response, audio_analysis_amd.analyse.fdw) against the
long-double restatement of tests/fdw_ref.py, held to its derived bounds (u = 2^-53):
  |S0 - ref| <= (N + 16) u A     |S1 - ref| <= (N + 16) u A1     |A - ref| <= (N + 4) u A     N exact
at half widths on both sides of every boundary the kernels have (a wavefront's rounds of 64 terms, the narrow / wide
switch at H = 127 / 128, a chunk of IRA_FDW_CHUNK terms), at clipped and empty windows, with non-finite samples, across
batches bit for bit, against two closed forms, and through the module and its command line.
Channels lie in one buffer with runs of NaN between them, at odd offsets: a term read from outside its channel would
turn the sums it enters into NaN.
"""
import json
import math
import os
import subprocess
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import fdw_ref as R
from oracle import ira_oracle as O

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
LD = np.longdouble
U = 2.0 ** -53
C = 4096                                                       # IRA_FDW_CHUNK
# both sides of: 64, 128, 192 terms (a narrow wave's rounds), H = 127 | 128 (narrow | wide), one chunk | two (2 H + 1 =
# 4095 | 4097), a last chunk of 11 terms (H = C + C / 2 + 5: 12299 = 3 C + 11) and of ONE term (H = 3 C: 24577 = 6 C + 1)
HALVES = [1, 2, 31, 32, 33, 63, 64, 95, 96, 127, 128, 129, C // 2 - 1, C // 2, C // 2 + 1, C + C // 2 + 5, 3 * C]
RHOS = [1e-6, 0.1234567, 0.5]
GUARD = 7                                                      # NaN samples in front of every channel (odd offsets)


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def table(halves=HALVES, rhos=RHOS):
    return (np.array([r for h in halves for r in rhos], dtype=np.float64),
            np.array([h for h in halves for _ in rhos], dtype=np.int32))


def run(eng, chans, centres, rho, half, window):
    """Engine level: one buffer, one call.  Returns the (nch, J, 6) float64 fields."""
    parts, offs, pos = [], [], 0
    for x in chans:
        parts += [np.full(GUARD, np.nan, np.float32), np.asarray(x, dtype=np.float32)]
        offs.append(pos + GUARD)
        pos += GUARD + len(x)
    parts.append(np.full(GUARD, np.nan, np.float32))
    x_dev = eng.to_dev(np.concatenate(parts))
    centre_dev = eng.to_dev(np.asarray(centres, dtype=np.int64))
    out = eng.fdw_response(x_dev, np.array(offs), np.array([len(x) for x in chans]), centre_dev, rho, half, window)
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def hold(got, x, p, rho, half, window, what):
    """Every point of one channel against the restatement; returns the worst error / bound."""
    worst = 0.0
    for j in range(len(rho)):
        ref = R.reference(x, p, rho[j], int(half[j]), window)
        assert got[j, 5] == ref["n"], (what, j, int(half[j]), got[j, 5], ref["n"])
        if ref["n"] == 0:
            assert not got[j].any(), (what, j, got[j])
        ratio = R.worst_ratio(got[j], ref)
        assert ratio <= 1.0, (what, j, int(half[j]), float(rho[j]), ratio, got[j], R.errors(got[j], ref), R.bounds(ref))
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("window", R.WINDOWS)
def test_half_widths_on_both_sides_of_every_boundary(window):
    rng = np.random.default_rng(101)
    rho, half = table()
    n = 2 * 3 * C + 501
    chans = [rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * np.exp(-np.arange(n) / 900.0)).astype(np.float32)]
    centres = [n // 2, 700]                                     # whole windows; windows clipped at the front from H = 2047 on
    got = run(_eng(), chans, centres, rho, half, window)
    assert got.shape == (2, len(rho), 6)
    worst = [hold(got[c], chans[c], centres[c], rho, half, window, f"channel {c}") for c in range(2)]
    print(f"half widths, {window}: worst error / bound {worst[0]:.4f} (whole), {worst[1]:.4f} (clipped)")
    whole = got[0, :, 5] == 2 * half + 1
    assert whole.all() and np.array_equal(got[1, :, 5] < 2 * half + 1, half > 700)


@pytest.mark.parametrize("window", R.WINDOWS)
def test_clipped_and_empty_windows(window):
    rng = np.random.default_rng(102)
    wide = C + C // 2 + 5
    rho, half = table([1, 33, 129, C // 2 + 1, wide], [0.1234567, 0.5])
    n = 2 * wide                                                # one shorter than the widest window
    x = rng.standard_normal(n).astype(np.float32)
    centres = [0, n - 1, n, n + wide + 3, -5, -wide - 1, n // 2]
    chans = [x] * len(centres) + [x[:0], x[:1], x[:1], x[:2], x[:2]]
    centres += [0, 0, 1, 0, 1]
    got = run(_eng(), chans, centres, rho, half, window)
    for c, (xc, p) in enumerate(zip(chans, centres)):
        hold(got[c], xc, p, rho, half, window, f"channel {c} (length {len(xc)}, centre {p})")
        inside = np.array([max(0, min(p + h, len(xc) - 1) - max(p - h, 0) + 1) for h in half.astype(np.int64)])
        assert np.array_equal(got[c, :, 5], inside), (c, got[c, :, 5], inside)
        assert not got[c][inside == 0].any()
    assert not got[3].any() and not got[5].any() and not got[7].any()           # past the end, before the start, no sample
    assert got[6, -1, 5] == n and got[6, 0, 5] == 3 and got[8, 0, 5] == 1 and got[11, 0, 5] == 2


def test_a_non_finite_sample_reaches_exactly_the_points_whose_window_covers_it():
    rng = np.random.default_rng(103)
    rho, half = table([1, 100, 199, 200, 201, 1029, 1030, 1031, C + C // 2 + 5], [0.1234567])
    n, p = 8000, 4000
    a, b, clean = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    a[p + 200] = np.nan
    b[p - 1030] = np.inf
    for window in R.WINDOWS:
        got = run(_eng(), [a, b, clean], [p, p, p], rho, half, window)
        assert np.array_equal(~np.isfinite(got[0, :, :5]).all(axis=1), half >= 200), window
        assert np.array_equal(~np.isfinite(got[1, :, :5]).all(axis=1), half >= 1030), window
        assert np.isfinite(got[2]).all() and np.isfinite(got[:, :, 5]).all()
        assert np.isinf(got[1, half >= 1030, 4]).all()                           # A = sum |v| of an infinity
        for c, x in enumerate((a, b, clean)):                                     # the other points are the usual sums
            keep = np.isfinite(got[c, :, :5]).all(axis=1)
            hold(got[c][keep], x, p, rho[keep], half[keep], window, f"channel {c}")


def test_sums_do_not_depend_on_the_batch():
    rng = np.random.default_rng(104)
    rho, half = table()
    eng = _eng()
    x = rng.standard_normal(9001).astype(np.float32)
    others = [rng.standard_normal(n).astype(np.float32) for n in (12345, 1, 30001, 777)]
    for window in R.WINDOWS:
        alone = run(eng, [x], [4200], rho, half, window)
        again = run(eng, [x], [4200], rho, half, window)
        assert np.array_equal(bits(alone), bits(again))
        for place in (0, 2, 4):
            chans = others[:place] + [x] + others[place:]
            centres = [int(c) for c in rng.integers(-50, 12000, 5)]
            centres[place] = 4200
            got = run(eng, chans, centres, rho, half, window)
            assert np.array_equal(bits(got[place]), bits(alone[0])), (window, place)
            assert np.array_equal(bits(run(eng, chans, centres, rho, half, window)), bits(got))


def _exact_turn(rho, d):
    """frac(rho d) of the float64 rho and a whole d, exactly, as a long double in [0, 1)."""
    t = (Fraction(float(rho)) * int(d)) % 1
    return LD(t.numerator) / LD(t.denominator)


@pytest.mark.parametrize("window", R.WINDOWS)
def test_unit_impulse_closed_form_on_the_device(window):
    """x = delta at p + d: S0 = w(d) e^{-2 pi i rho d} and S1 = d S0 within the bounds (A = w(d), A1 = |d| w(d)), so the
    group delay is d samples to 2 (N + 16) u |d| and the host arithmetic's roundings (8 u |d|)."""
    from audio_analysis_amd.analyse.fdw import fdw_arithmetic
    rho, half = table([1, 33, 127, 128, 700, C // 2 + 1, C + C // 2 + 5], [1e-6, 0.1234567, 0.5])
    n, p = 2 * (C + C // 2 + 5) + 301, C + C // 2 + 155
    chans, shifts = [], []
    for d in (0, 1, -1, 33, -127, 128, -700, C // 2 + 1, -(C + C // 2 + 5)):
        x = np.zeros(n, np.float32)
        x[p + d] = 1.0
        chans.append(x)
        shifts.append(d)
    got = run(_eng(), chans, [p] * len(chans), rho, half, window)
    for c, d in enumerate(shifts):
        curves = fdw_arithmetic(got[c], half, 1.0)
        for j in range(len(rho)):
            h, f = int(half[j]), got[c, j].astype(LD)
            assert f[5] == 2 * h + 1
            if abs(d) > h:
                assert not got[c, j, :5].any() and math.isnan(curves["group_delay_seconds"][j])
                continue
            w = np.sin(R.PI * LD(h + 1 - abs(d)) / LD(2 * h + 2)) ** 2 if window == "hann" else LD(1)
            ang = LD(2) * R.PI * _exact_turn(rho[j], d)
            re, im = w * np.cos(ang), -w * np.sin(ang)
            bound = LD(2 * h + 1 + 16) * LD(U)
            assert np.hypot(f[0] - re, f[1] - im) <= bound * w, (c, j, d, h)
            assert np.hypot(f[2] - d * re, f[3] - d * im) <= bound * abs(d) * w, (c, j, d, h)
            assert abs(f[4] - w) <= LD(2 * h + 1 + 4) * LD(U) * w
            delay = curves["group_delay_seconds"][j]                             # fs = 1: in samples
            assert abs(delay - d) <= (2.0 * (2 * h + 17) + 8.0) * U * abs(d) * 1.001, (c, j, d, h, delay)
            assert curves["cancellation"][j] == pytest.approx(1.0, abs=(2 * h + 40) * U) and not curves["clipped"][j]


def test_rect_window_over_the_whole_channel_is_the_rfft_on_the_device():
    """rect, H = n (every sample inside from any centre), rho = fl(m / n): S0 = rfft(x)[m] e^{+2 pi i m p / n} to the
    device's bound (n + 16) u A, the transform's own error (under 8 log2(n) u A: A = sum |x| bounds every bin), the phase
    factor's (2 u A), and what rho's rounding moves the phasors by: |rho - m / n| <= rho u and |k| <= n, 2 pi n rho u A."""
    rng = np.random.default_rng(105)
    eng = _eng()
    for n, centres in ((375, (0, 17, 374)), (1000, (0, 999)), (2 * C + 3, (C,))):
        x = rng.standard_normal(n).astype(np.float32)
        spec = np.fft.rfft(x.astype(np.float64))
        a = float(np.sum(np.abs(x.astype(np.float64))))
        ms = [1, 2, n // 5, n // 2]
        rho = np.array([m / n for m in ms])
        got = run(eng, [x] * len(centres), list(centres), rho, np.full(len(ms), n, np.int32), "rect")
        for c, p in enumerate(centres):
            for j, m in enumerate(ms):
                want = spec[m] * np.exp(2j * np.pi * ((m * p) % n) / n)
                tol = (n + 16 + 8.0 * math.log2(n) + 2.0 + 2.0 * math.pi * n * rho[j]) * U * a
                assert got[c, j, 5] == n and abs(complex(got[c, j, 0], got[c, j, 1]) - want) <= tol, (n, p, m)
                assert abs(got[c, j, 4] - a) <= (n + 4) * U * a


# ------------------------------------------------------------------------------------------------ module level
def _module_case(sample_rate_hz, lengths):
    from audio_analysis_amd.synth import synth_ir
    return [synth_ir(20 + i, 0, n, sample_rate_hz) for i, n in enumerate(lengths)]


@pytest.mark.parametrize("sample_rate_hz,lengths", [(48000, (24000, 9001)), (44100, (12000,))])
def test_module_at_the_defaults(sample_rate_hz, lengths):
    """analyse_fdw_batch at the defaults: every curve is the host arithmetic applied to the device's own sums, exactly,
    and the level lies within the image of the S0 bound in dB around the restatement's, 20 log10(1 + (N + 16) u A / |S0|)
    and 3e-14 dB for the host arithmetic (the power's three roundings, 4.3 u dB, and one rounding of a level below 128 dB,
    2^-46 dB), at every point with |S0| / A > 1e-6.  The share of points that leaves out is asserted to be 0 here."""
    from audio_analysis_amd.analyse import fdw as D
    eng = _eng()
    chans = _module_case(sample_rate_hz, lengths)
    names = [f"ir{i}" for i in range(len(chans))]
    res = D.analyse_fdw_batch(chans, sample_rate_hz, names)
    rec = D.fdw_device(eng, eng.upload(chans), sample_rate_hz, D.FdwSettings())
    f, rho, half = D.fdw_grid(D.FdwSettings(), sample_rate_hz)
    left_out = 0
    for c, (r, x) in enumerate(zip(res, chans)):
        peak = int(np.argmax(np.abs(x)))
        assert (r.channel_name, r.centre, r.centre_samples, r.centre_seconds) == (names[c], "peak", peak, peak / sample_rate_hz)
        assert r.centre_samples == rec.centre[c] and np.array_equal(r.frequencies_hz, f) and np.array_equal(r.half_samples, half)
        curves = D.fdw_arithmetic(rec.sums[c], half, sample_rate_hz, -120.0)
        for name, want in curves.items():
            got = getattr(r, name)
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=want.dtype != bool), name
        assert np.isfinite(r.level_db).all() and r.clipped.any() and not r.clipped.all()
        for j in range(len(f)):
            ref = R.reference(x, peak, rho[j], int(half[j]), "hann")
            assert R.worst_ratio(rec.sums[c, j], ref) <= 1.0, (c, j)
            mag = np.hypot(ref["re0"], ref["im0"])
            if not mag / ref["a"] > 1e-6:
                left_out += 1
                continue
            tol = 20.0 * np.log10(LD(1) + LD(ref["n"] + 16) * LD(U) * ref["a"] / mag) + LD(3e-14)
            assert abs(LD(r.level_db[j]) - 20.0 * np.log10(mag)) <= tol, (c, j, float(f[j]), r.level_db[j], float(tol))
    print(f"{sample_rate_hz} Hz: {left_out} of {len(f) * len(chans)} points left out (|S0| / A <= 1e-6)")
    assert left_out == 0


def test_centre_onset_is_the_device_onset():
    from audio_analysis_amd.analyse import fdw as D
    eng = _eng()
    chans = _module_case(48000, (9001, 6000))
    st = D.FdwSettings(centre="onset", onset_db=-30.0, points_per_octave=3, window="rect")
    res = D.analyse_fdw_batch(chans, 48000, ["a", "b"], st)
    onset = eng.onset_index(eng.upload(chans), st.rel_energy)[0].cpu().numpy()
    f, rho, half = D.fdw_grid(st, 48000)
    for r, x, o in zip(res, chans, onset):
        assert r.centre == "onset" and r.centre_samples == int(o) <= int(np.argmax(np.abs(x))) and r.window == "rect"
        got = r.level_db
        for j in range(len(f)):
            ref = R.reference(x, int(o), rho[j], int(half[j]), "rect")
            mag = np.hypot(ref["re0"], ref["im0"])
            tol = 20.0 * np.log10(LD(1) + LD(ref["n"] + 16) * LD(U) * ref["a"] / mag) + LD(3e-14)
            assert abs(LD(got[j]) - 20.0 * np.log10(mag)) <= tol, (j, got[j])


def test_cli_on_a_stereo_wav_equals_the_python_api(tmp_path):
    from audio_analysis_amd.analyse import fdw as D
    chans = _module_case(48000, (6000, 6000))
    wav = tmp_path / "room.wav"
    wav.write_bytes(O.recorder_wav_bytes(0.5 * np.stack(chans, axis=1).reshape(-1), 48000))
    env = dict(os.environ, PYTHONPATH=str(REPO))
    out_json = tmp_path / "room.json"
    args = ["--cycles", "6", "--points-per-octave", "6", "--window", "rect", "--f-min", "50", "--max-window-ms", "20"]
    r = subprocess.run([sys.executable, "-m", "analyse.fdw", "--input", str(wav), *args, "--json", str(out_json)],
                       capture_output=True, text=True, cwd=str(REPO), env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "NaN" not in out_json.read_text()
    doc = json.loads(out_json.read_text())
    st = D.FdwSettings(cycles=6.0, points_per_octave=6, window="rect", f_min_hz=50.0, max_window_ms=20.0)
    api = D.analyse_fdw_files([wav], st)
    assert [d["channel_name"] for d in doc["fdw"]] == ["room.wav:left", "room.wav:right"]
    assert doc == D.fdw_results_to_json(api) and r.stdout == D.summarise_fdw_text(api)
    assert max(doc["fdw"][0]["half_samples"]) == 960 and len(doc["fdw"][0]["level_db"]) == 52
