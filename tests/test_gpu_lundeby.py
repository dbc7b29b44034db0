"""
The Lundeby kernels (ira_block_energy, ira_lundeby_estimate, ira_edc_truncated; ira_lundeby.hip) and
audio_analysis_amd.analyse.lundeby on the device, against the long-double restatement of tests/lundeby_ref.py.

Integer outputs (t1, m1, kmax, k0, k1, rounds, status) are compared exactly, on inputs whose decision margin in the
restatement is at least 1e-6 dB and 1e-6 of an interval: a condition on the input that the tests assert for the
restatement alone.  Float outputs (Ln, slope, intercept, C) are held to FLOAT_BOUND (below): ten times the largest
deviation measured on the device.  The curve is held to the allowance tests/decay_ref.py states for ira_edc_db's float32
curve (the kernel is the same chain plus one addition).
"""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import lundeby_ref as R
from oracle import ira_oracle as O

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
SR = 48000
EPS, FLOOR_DB = 1e-20, -120.0
SENTINEL = np.float32(12345.0)
# The largest relative deviation of Ln, slope, intercept and C from the restatement, measured on an MI355X over the cases
# of test_estimate_against_the_restatement (4.8e-15) and test_bands_on_the_oracles_band_signals (1.1e-12, the 16 kHz
# band's intercept of 0.0058 dB, the difference of two terms of 19.6 dB: DESIGN.md 4.9; every other value below 5.4e-15).  Both tests print their figure and assert ten times the larger one.
FLOAT_MEASURED = 1.1e-12
FLOAT_BOUND = 10.0 * FLOAT_MEASURED
INT_FIELDS = ("t1", "m1", "kmax", "k0", "k1", "rounds")
REC = dict(status=0, Ln=1, t1=2, slope=3, intercept=4, C=5, rounds=6, m1=7, kmax=8, k0=9, k1=10, tx0=11, tx=12, mmax=13,
           edc0=14, ncurve=15)


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def device_rows(eng, chans, rates, compensate=True, curves=True, chan_of_row=None):
    """Engine level: every channel a row (or chan_of_row[j] the channel whose start index row j uses) through the three
    kernels.  Returns per row: s, L, B, nb, E (nb + 1 block energies), rec, length, curve (float32, the sentinel behind it)."""
    t = eng.torch
    b = eng.upload([np.asarray(c, dtype=np.float32) for c in chans])
    pk, _ = eng._batch_peak_pick(b)
    pk = pk[: b.count]
    s_ch = pk.cpu().numpy().astype(np.int64)
    ch = np.arange(b.count, dtype=np.int32) if chan_of_row is None else np.asarray(chan_of_row, dtype=np.int32)
    s = s_ch[ch]
    L = b.length.astype(np.int64) - s
    B = np.array([R.block_size(fs, l) for fs, l in zip(rates, L)], dtype=np.int32)
    nb = (L // B).astype(np.int32)
    m0 = np.array([R.first_interval(fs, v) for fs, v in zip(rates, B)], dtype=np.int32)
    rows = eng.lundeby_rows(b.off, b.length, ch, B, nb, m0)
    blk = eng.block_energy(b.x, rows, pk)
    rec, lens, suf = eng.lundeby_estimate(rows, pk, blk, compensate)
    out = []
    gap = 5
    edc_off = np.cumsum(L + gap) - (L + gap) + 1                          # odd offsets, a gap behind every curve
    edc = t.full((int((L + gap).sum()) + 1,), float(SENTINEL), dtype=t.float32, device=b.x.device)
    if curves:
        eng.edc_truncated(b.x, rows, pk, rec, lens, suf, EPS, FLOOR_DB, edc, edc_off)
    blk_h, rec_h, lens_h, edc_h = blk.cpu().numpy(), rec.cpu().numpy(), lens.cpu().numpy(), edc.cpu().numpy()
    for j in range(len(chans)):
        o = int(rows["blk_off"][j])
        out.append(dict(s=int(s[j]), L=int(L[j]), B=int(B[j]), nb=int(nb[j]), E=blk_h[o : o + int(nb[j]) + 1].copy(),
                        rec=rec_h[j].copy(), length=int(lens_h[j]),
                        curve=edc_h[edc_off[j] : edc_off[j] + int(L[j]) + gap].copy()))
    assert edc_h[0] == SENTINEL
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if np.asarray(a).dtype == np.float64 else np.uint32)


# ------------------------------------------------------------------------------------------------ 1: block energies
def _odd_start(x):
    """x with an odd index of its first maximum"""
    return x if int(np.argmax(np.abs(x))) % 2 else np.concatenate([np.zeros(1, np.float32), x])


def test_block_energies_against_long_double():
    R.need_longdouble()
    eng = _eng()
    long_x = R.decaying_noise(SR, 4.3, 0.8, -55, 5)
    short_x = R.decaying_noise(SR, 0.2, 0.1, -40, 6)
    chans, rates = [], []
    for tail in (0, 1, 47):
        chans.append(R.after_peak(short_x, 31 * 48 + tail)); rates.append(SR)            # noqa: E702
    chans.append(R.after_peak(long_x, 4096 * 48)); rates.append(SR)                       # noqa: E702
    chans.append(R.after_peak(long_x, 4096 * 48 + 1)); rates.append(SR)                   # noqa: E702
    before = sum(c.size for c in chans)
    chans.append(np.full(3 if before % 2 == 0 else 4, 0.01, np.float32)); rates.append(SR)   # an odd batch offset behind it  # noqa: E702
    chans.append(_odd_start(R.after_peak(short_x, 40 * 48 + 13))); rates.append(SR)       # noqa: E702
    chans.append(R.after_peak(R.decaying_noise(44100, 0.2, 0.1, -40, 7), 45 * 40 + 7)); rates.append(44100)   # noqa: E702
    got = device_rows(eng, chans, rates, curves=False)
    assert [g["B"] for g in got] == [48, 48, 48, 48, 49, 48, 48, 45]
    assert [g["L"] - g["nb"] * g["B"] for g in got[:5]] == [0, 1, 47, 0, 4096 * 48 + 1 - 4012 * 49]
    assert got[6]["s"] % 2 == 1 and sum(c.size for c in chans[:6]) % 2 == 1
    worst = 0.0
    for g, x in zip(got, chans):
        E, tail = R.block_energies(x[g["s"]:], g["B"])
        assert E.size == g["nb"]
        ref = np.concatenate([E, [tail]])
        terms = np.array([g["B"]] * g["nb"] + [g["L"] - g["nb"] * g["B"]])
        dev = np.abs((g["E"].astype(R.LD) - ref).astype(np.float64))
        bound = (terms + 1) * 2.0 ** -53 * ref.astype(np.float64)
        assert np.all(dev <= bound), (g["B"], g["L"], float((dev / np.maximum(bound, 1e-300)).max()))
        nz = ref > 0
        worst = max(worst, float((dev[nz] / bound[nz]).max()))
    print(f"block energies: worst deviation / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 2, 3: estimate, curve
def estimate_cases():
    """(name, fs, samples): a plain decay with a floor, one that needs the 3-point widening, one whose m1 hits the nb // 16
    clamp, two without a noise floor inside the file, the 4096 * 48 + 1 shape.  A pure exponential decay to the end of
    the file gives status 32 only where its noisy tail happens to lie on or below the fitted line (the mean of the tail
    lies on the line in expectation, which puts the cross-point inside the file about as often as behind it): "clean" is
    such a decay, its seed chosen on the CPU; "no floor" ends in a 12 % fade-out, as exported responses do, which puts
    the tail below the line whatever the seed."""
    fs = 8000
    return [("floor", fs, R.decaying_noise(fs, 1.5, 0.5, -50, 0)),
            ("widened", fs, R.two_slope_noise(fs, 2.5, 2.0, 0.6, 0.08, -60, 0)),
            ("clamped", fs, R.decaying_noise(fs, 1.0, 2.5, -18, 0)),
            ("clean", fs, R.decaying_noise(fs, 1.5, 6.0, None, 0)),
            ("no floor", fs, R.decaying_noise(fs, 2.0, 3.0, None, 0, fade=0.12)),
            ("4096 * 48 + 1", SR, R.after_peak(R.decaying_noise(SR, 4.2, 0.8, -55, 0), 4096 * 48 + 1))]


def check_case_conditions(refs):
    """What the cases must show, for the restatement alone (also run on the CPU by tests/test_lundeby_cpu.py)."""
    by = {name: r for name, r in refs}
    for name, r in refs:
        assert r["margin"].ok(), (name, r["margin"].db, r["margin"].interval)
    assert by["floor"]["status"] == 0 and not by["floor"]["widened"] and not by["floor"]["clamped"]
    assert by["widened"]["status"] == 0 and by["widened"]["widened"]
    assert by["clamped"]["status"] == 0 and by["clamped"]["clamped"]
    assert by["clean"]["status"] == R.S_NO_FLOOR and by["no floor"]["status"] == R.S_NO_FLOOR
    assert by["4096 * 48 + 1"]["B"] == 49 and by["4096 * 48 + 1"]["status"] == 0


_SHARED = {}


def estimate_batch():
    """The six cases through the device once, and their restatements (shared by the estimate and the curve test)."""
    if "est" not in _SHARED:
        R.need_longdouble()
        cases = estimate_cases()
        got = device_rows(_eng(), [x for _, _, x in cases], [fs for _, fs, _ in cases])
        refs = [(name, R.estimate(x[g["s"]:], fs)) for (name, fs, x), g in zip(cases, got)]
        _SHARED["est"] = (cases, got, refs)
    return _SHARED["est"]


def compare_estimate(name, g, r):
    """Integers exact, floats relative; returns the largest relative deviation of Ln, slope, intercept, C."""
    rec = g["rec"]
    assert int(rec[REC["status"]]) == r["status"], (name, rec[REC["status"]], r["status"])
    for f in INT_FIELDS:
        assert int(rec[REC[f]]) == r[f], (name, f, rec[REC[f]], r[f])
    assert g["length"] == r["length"], name
    rels = {}
    for f in ("Ln", "slope", "intercept", "C"):
        want = r[f]
        dev = abs(float(R.LD(rec[REC[f]]) - want))
        rels[f] = dev / abs(float(want)) if float(want) != 0.0 else dev
    print(f"  {name}: " + "  ".join(f"{f} {float(r[f]):.6g} (deviation {v:.2e})" for f, v in rels.items()))
    return max(rels.values())


def test_estimate_against_the_restatement():
    cases, got, refs = estimate_batch()
    check_case_conditions(refs)
    worst = 0.0
    for (name, _, _), g, (_, r) in zip(cases, got, refs):
        w = compare_estimate(name, g, r)
        print(f"estimate {name}: status {r['status']} t1 {r['t1']} m1 {r['m1']} rounds {r['rounds']} largest relative deviation {w:.3e}")
        worst = max(worst, w)
    print(f"estimate: largest relative deviation {worst:.3e}")
    assert worst <= FLOAT_BOUND, worst


def test_truncated_curve_against_the_restatement():
    """ira_edc_truncated fed the GPU's own record (length and C) against the long-double curve: the allowance of
    decay_ref.py's comparison A (float64 sums of length + 2 terms, two table logarithms) plus one float32 ulp; nothing
    written at or after t1.  The kernel's float32 curve starts at exactly 0 dB and never lies above it; that it falls from
    sample to sample holds to this allowance only (neighbouring samples may be summed in different orders)."""
    cases, got, refs = estimate_batch()
    same = total = 0
    for (name, fs, x), g in zip(cases, got):
        n = g["length"]
        y = x[g["s"]:]
        C = g["rec"][REC["C"]]
        _, ref32 = R.curve(y, n, C, EPS, FLOOR_DB)
        bound = R.curve_bound_db(y, n, C, EPS)
        cur = g["curve"]
        assert np.all(cur[n:] == SENTINEL), name
        assert cur[0] == 0.0 and np.all(cur[:n] <= 0.0), name             # no sample above the first one
        d = np.abs(cur[:n].astype(np.float64) - ref32.astype(np.float64))
        allow = bound + np.spacing(np.abs(ref32)).astype(np.float64)
        assert np.all(d <= allow), (name, int(np.argmax(d / allow)), float((d / allow).max()))
        same += int(np.sum(_bits(cur[:n]) == _bits(ref32)))
        total += n
    print(f"curve: {same} of {total} float32 samples bit-identical to the long-double curve ({100.0 * same / total:.4f} %)")
    assert same >= 0.99 * total


# ------------------------------------------------------------------------------------------------ 4, 5: fits, physics
PHYSICS = ((1.0, -45, 10), (1.5, -50, 6), (0.3, -60, 2))


def physics_files():
    if "phys" not in _SHARED:
        _SHARED["phys"] = [(rt, R.decaying_noise(SR, sec, rt, nz, seed)) for rt, nz, sec in PHYSICS for seed in range(3)]
    return _SHARED["phys"]


def test_fits_come_from_curve_fits_with_device_lengths():
    """The lens_dev path of Engine.curve_fits: the module's fit records equal ira_curve_fits run with HOST lengths on the
    same curves, bit for bit.  Both launches take their workgroup size from the longest length the host knows (which
    fixes the order of the regression sums): the rows are long enough for both bounds to fall in the same class."""
    from audio_analysis_amd.analyse import lundeby as L
    eng = _eng()
    files = [x for _, x in physics_files()[2:5]]
    st = L.LundebySettings(bands=None)
    dev = L.lundeby_device(eng, eng.upload(files), SR, st)
    # the result owns the memory its curves live in (samples and broadband curves; no bands here)
    assert len(dev.buffers) == 2 and dev.edc.data_ptr() == min(b.data_ptr() for b in dev.buffers)
    lens = dev.lens_dev.cpu().numpy()
    assert lens.min() > 32768                                           # both launches: 1024 threads, pre-searched crossings
    _, ranges = L.decay_fit_specs(st.decay)
    fits, cross = eng.curve_fits(dev.edc, dev.edc_off, lens, 1.0, float(SR), ranges, 8, cross=(0.0, -10.0))
    assert np.array_equal(_bits(fits.cpu().numpy()), _bits(dev.fits.cpu().numpy()))
    assert np.array_equal(_bits(cross.cpu().numpy()), _bits(dev.cross.cpu().numpy()))
    assert np.all(dev.fits.cpu().numpy()[:, :, 0] == 1.0)


def test_compensated_decay_times_on_noisy_decays():
    """Why the feature exists: T30 on the truncated, compensated curve is within 5 % of the true reverberation time where
    the plain full-length Schroeder integration of analyse.decay is off by more than 10 %."""
    from audio_analysis_amd.analyse import decay as D
    from audio_analysis_amd.analyse import lundeby as L
    files = physics_files()
    chans = [x for _, x in files]
    names = [f"c{i}" for i in range(len(chans))]
    comp = L.analyse_lundeby_batch(chans, SR, names, L.LundebySettings(bands=None))
    trunc = L.analyse_lundeby_batch(chans, SR, names, L.LundebySettings(bands=None, mode="truncate"))
    plain = D.analyse_decay_batch(chans, SR, names, D.DecayAnalysisSettings())
    for (rt, _), c, tr, p in zip(files, comp, trunc, plain):
        t30 = p.fits["T30"].rt60_seconds if "T30" in p.fits else float("inf")
        print(f"RT {rt}: compensated T30 {c.broadband.t30_seconds:.4f}  truncated {tr.broadband.t30_seconds:.4f}  plain {t30:.3f}"
              f"  Ln {c.broadband.noise_db:.2f}  cross-point {c.broadband.cross_point_seconds:.3f} s")
        assert c.broadband.status == 0 and tr.broadband.status == 0
        assert abs(c.broadband.t30_seconds - rt) <= 0.05 * rt
        assert tr.broadband.compensation_energy == 0.0 and c.broadband.compensation_energy > 0.0
        assert abs(tr.broadband.t30_seconds - rt) <= 0.05 * rt
        if rt != 0.3:
            assert abs(t30 - rt) > 0.10 * rt


# ------------------------------------------------------------------------------------------------ 6, 7: status, identity
def status_rows():
    fs = 8000
    rng = np.random.default_rng(11)
    good = R.decaying_noise(fs, 1.5, 0.5, -50, 3)
    silence = np.zeros(fs, np.float32)
    short = R.after_peak(R.decaying_noise(fs, 0.1, 0.05, -40, 4), 20 * 8 + 3)
    # a click, then a ramp that rises from -35 dB to -8 dB of the click's interval, then a floor: the first interval holds
    # the maximum and the line over the ramp rises
    n = fs
    ramp = rng.standard_normal(n) * 10.0 ** (np.linspace(-35.0, -8.0, n) / 20.0) * 0.064
    floor = rng.standard_normal(n // 2) * 10.0 ** (-50.0 / 20.0) * 0.064
    rising = np.concatenate([[1.0], ramp, floor]).astype(np.float32)
    nan = good.copy()
    nan[good.size // 2] = np.nan
    return fs, good, [("silent", silence, R.S_SILENT), ("short", short, R.S_SHORT), ("rising", rising, R.S_SLOPE),
                      ("nan", nan, R.S_NON_FINITE)]


def test_status_rows_keep_the_batch():
    R.need_longdouble()
    eng = _eng()
    fs, good, bad = status_rows()
    alone = device_rows(eng, [good], [fs])[0]
    chans = [bad[0][1], bad[1][1], good, bad[2][1], bad[3][1]]
    got = device_rows(eng, chans, [fs] * len(chans))
    assert np.array_equal(_bits(got[2]["rec"]), _bits(alone["rec"])) and int(alone["rec"][0]) == 0
    assert np.array_equal(_bits(got[2]["curve"]), _bits(alone["curve"]))
    for (name, x, want), g in zip(bad, [got[0], got[1], got[3], got[4]]):
        assert R.estimate(x[g["s"]:], fs)["status"] == want, name
        assert int(g["rec"][0]) == want, (name, g["rec"][0])
        assert np.all(np.isnan(g["rec"][1:])) and g["length"] == 0, name
        assert np.all(g["curve"] == SENTINEL), name
    # through the module: NaN in every output of those rows, the good one reported
    from audio_analysis_amd.analyse import lundeby as L
    res = L.analyse_lundeby_batch(chans, fs, ["a", "b", "c", "d", "e"], L.LundebySettings(bands=None))
    assert [r.broadband.status for r in res] == [R.S_SILENT, R.S_SHORT, 0, R.S_SLOPE, R.S_NON_FINITE]
    for i in (0, 1, 3, 4):
        v = res[i].broadband
        assert all(math.isnan(getattr(v, f)) for f in L._FLOAT_FIELDS) and not (v.edt_valid or v.t20_valid or v.t30_valid)
    assert abs(res[2].broadband.t30_seconds - 0.5) < 0.05


def test_bit_identical_whatever_the_batch():
    eng = _eng()
    fs = 8000
    x = R.decaying_noise(fs, 2.2, 0.7, -48, 8)
    alone = device_rows(eng, [x], [fs])[0]
    rng = np.random.default_rng(2)
    others = [R.decaying_noise(fs, float(rng.uniform(0.6, 2.0)), 0.4, -40, 20 + k) for k in range(6)]
    for shift, before, after in ((1, others[:1], others[1:3]), (2, others[:4], []), (3, others[2:5], others[5:])):
        chans = before + [np.full(shift, 0.25, np.float32), x] + after
        g = device_rows(eng, chans, [fs] * len(chans))[len(before) + 1]
        assert np.array_equal(_bits(g["rec"]), _bits(alone["rec"])), shift
        assert np.array_equal(_bits(g["E"]), _bits(alone["E"])), shift
        assert np.array_equal(_bits(g["curve"]), _bits(alone["curve"])), shift
    assert int(alone["rec"][0]) == 0


# ------------------------------------------------------------------------------------------------ 8: bands
def oracle_band_signals(x, sr, mode="octave"):
    n = x.size
    f = np.fft.rfftfreq(n, d=1.0 / float(sr)).astype(np.float32)
    spec = np.fft.rfft(x.astype(np.float64))
    out = []
    for b in O.band_definitions(sr, band_mode=mode):
        m = O.band_mask(f, b, 1.0 / 6.0, 0.5 * float(sr))
        out.append((b["name"], np.fft.irfft(spec * m.astype(np.float64), n=n).astype(np.float32)))
    return out


def band_case():
    from audio_analysis_amd.synth import synth_ir
    rng = np.random.default_rng(5)
    x = synth_ir(61, 0, SR, SR, rt60_seconds=0.35)
    return (x + rng.standard_normal(SR).astype(np.float32) * np.float32(np.max(np.abs(x)) * 10.0 ** (-55.0 / 20.0))).astype(np.float32)


def band_references(x):
    """[(band name, band signal, restatement on it from the broadband start index on)]"""
    s = int(np.argmax(np.abs(x)))
    return s, [(name, y, R.estimate(y[s:], SR)) for name, y in oracle_band_signals(x, SR)]


def test_bands_on_the_oracles_band_signals():
    """The octave bank: the module fed the oracle's float64 band signals rounded to float32 (so that both sides see the same
    samples: integers exact where the band's margin holds, at most 2 of 9 bands skipped for it, floats to FLOAT_BOUND).
    The full device path (filter bank on the device) is NOT compared to the restatement: its band signals differ from the
    oracle's by up to 1e-6 of the peak, which is no input the margin condition was established for, so its Ln, t1, m1,
    kmax, k0, k1 and rounds are not checked at all.  It is held only to the other path: the same status, and EDT, T20 and
    T30 within 2 %, on the bands that are neither skipped for their margin nor in an error status."""
    R.need_longdouble()
    from audio_analysis_amd.analyse import lundeby as L
    from audio_analysis_amd.analyse.rt60bands import Rt60BandsAnalysisSettings, _build_band_definitions
    eng = _eng()
    x = band_case()
    s, refs = band_references(x)
    assert len(refs) == 9
    st = L.LundebySettings()
    bands = _build_band_definitions(st.bands, SR)
    assert [b.name for b in bands] == [n for n, _, _ in refs]
    full = L.lundeby_results(L.lundeby_device(eng, eng.upload([x]), SR, st), SR, ["x"], st)[0]
    batch = eng.upload([x])
    yb = eng.upload([y for _, y, _ in refs])
    dev = L.lundeby_device(eng, batch, SR, st, band_signals=(bands, yb.x, yb.off.reshape(1, 9)))
    rec = dev.records.cpu().numpy()
    lens = dev.lens_dev.cpu().numpy()
    assert int(dev.start[0]) == s
    res = L.lundeby_results(dev, SR, ["x"], st)[0]
    skipped, worst = 0, 0.0
    for j, (name, y, r) in enumerate(refs):
        g = dict(rec=rec[1 + j], length=int(lens[1 + j]))
        if not r["margin"].ok():
            skipped += 1
            continue
        if r["status"] & 31:
            assert int(g["rec"][0]) == r["status"], name
            continue
        worst = max(worst, compare_estimate(name, g, r))
        a, b = res.band_values_by_name[name], full.band_values_by_name[name]
        assert a.status == b.status, name
        for f in ("edt_seconds", "t20_seconds", "t30_seconds"):
            va, vb = getattr(a, f), getattr(b, f)
            assert (math.isnan(va) and math.isnan(vb)) or abs(va - vb) <= 0.02 * abs(va), (name, f, va, vb)
    assert skipped <= 2
    print(f"bands: largest relative deviation {worst:.3e}, {skipped} bands skipped")
    assert worst <= FLOAT_BOUND, worst


# ------------------------------------------------------------------------------------------------ 9: command line
def _run_cli(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=str(REPO))
    r = subprocess.run([sys.executable, "-m", "analyse.lundeby", *map(str, args)], capture_output=True, text=True,
                       cwd=str(REPO), env=env, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_cli_on_wav_and_bundle(tmp_path):
    from audio_analysis_amd.analyse import lundeby as L
    n = SR
    taps = {}
    for k, name in enumerate(["hall", "plate"]):
        st = 0.3 * np.stack([R.decaying_noise(SR, 1.0, 0.25 + 0.05 * k, -50, 30 + k),
                             R.decaying_noise(SR, 1.0, 0.3, -45, 40 + k)], axis=1)             # 16-bit PCM: keep clear of +-1
        taps[name] = O.recorder_wav_bytes(st.reshape(-1), SR)
    wav = tmp_path / "hall.wav"
    wav.write_bytes(taps["hall"])
    out = _run_cli(["--input", wav, "--bands", "three", "--json", tmp_path / "w.json"])
    from audio_analysis_amd.analyse.rt60bands import Rt60BandsAnalysisSettings
    api = L.analyse_lundeby_files([wav], L.LundebySettings(bands=Rt60BandsAnalysisSettings(band_mode="three")))
    assert out == L.summarise_lundeby_text(api)
    assert [r.channel_name for r in api] == ["hall.wav:left", "hall.wav:right"]
    lines = out.split("\n")
    assert lines[0] == "[hall.wav:left]" and lines[1].startswith("Start: ") and lines[1].endswith("Mode: compensate")
    assert lines[2] == "Band  Noise_dB  Cross_ms  Range_dB  Slope_dB_s  C  EDT_s  T20_s  T30_s  Valid  Status"
    assert lines[3].startswith("Broadband  -") and lines[3].endswith("  ok")
    assert abs(api[0].broadband.t30_seconds - 0.25) <= 0.05 * 0.25
    back = L.lundeby_results_from_json(json.loads((tmp_path / "w.json").read_text()))
    assert L.summarise_lundeby_text(back) == out
    assert back[0].broadband == api[0].broadband and back[1].band_values_by_name == api[1].band_values_by_name
    root = tmp_path / "bundle"
    (root / "taps").mkdir(parents=True)
    for name, blob in taps.items():
        (root / "taps" / f"{name}.wav").write_bytes(blob)
    (root / "meta.json").write_text(O.recorder_meta_json(SR, n, list(taps)))
    out = _run_cli(["--bundle", root, "--mono", "--bands", "none", "--mode", "truncate"])
    api = L.analyse_lundeby_bundle(root, L.LundebySettings(bands=None, mode="truncate", use_mono_downmix_for_stereo=True))
    assert out == L.summarise_lundeby_text(api)
    assert [r.channel_name for r in api] == ["hall:mono", "plate:mono"]
    assert all(r.broadband.compensation_energy == 0.0 and r.mode == "truncate" for r in api)
