"""
Equalisation on the device through its public functions (audio_analysis_amd.analyse.equalise) against the restatement of
tests/equalise_ref.py (its docstring derives every bound used here).

  * With the device's own X and F fetched, S, ref, c, the clamped counts, the prediction and every curve equal the
    restatement fed with them BIT FOR BIT.
  * The filter against the float64 restatement on that same c, per sample within FilterBounds.filter (minphase_ref's
    Bounds.response with E_X = 0 and no floor term: the chain's input is exact).
  * Against the restatement from NumPy's own X: |ln c_dev - ln c| <= 2 E_X (1 / |X|_window + 1 / min_grid |X|_window).
  * The two closed forms (a unit impulse, x = 0.5^n) on the device within those bounds.
  * average, silent / NaN / empty channels, post_ms, the sub-batch cut, the command line.

Worst error / bound observed on an MI355X over the cases of CASES (printed by the tests; DESIGN.md 4.22 has the table):
    the filter 0.024 .. 0.18, ln c at most 0.0004, the closed forms 0.0000 (impulse) and 0.095 (one pole).
Shapes stay at N <= 4096 but for one case at N = 2^14 with 2048 taps, whose pyramid takes five tiles and two passes.
"""
import functools
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import equalise_ref as R
from oracle import ira_oracle as O

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
FS = 48000


def _eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


def _eq():
    from audio_analysis_amd.analyse import equalise as D
    return D


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@functools.lru_cache(maxsize=None)
def channel(length, seed):
    """Decaying noise behind a direct sound that is the one largest sample."""
    rng = np.random.default_rng(2000 + seed)
    x = rng.standard_normal(length) * np.exp(-np.arange(length) / max(length / 6.0, 1.0))
    x[min(3, length - 1)] = 5.0
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


# name -> (channel lengths, settings)
CASES = {
    "N32 b0": ((5, 12), dict(taps=16, smoothing=0)),
    "N64 b3": ((30, 17, 25), dict(taps=16, smoothing=3, max_boost_db=3.0)),
    "N64 b1 average": ((30, 17, 25), dict(taps=32, smoothing=1, average=True)),
    "N4096 b6 tilt": ((2000, 1500), dict(taps=256, smoothing=6, tilt_db_per_octave=-1.0, regularisation_db=-30.0)),
    "N4096 b48": ((1100,), dict(taps=512, smoothing=48, n_fft=4096, f_low_hz=100.0, f_high_hz=8000.0, fade=0.5)),
    "N16384 b3": ((6000,), dict(taps=2048, smoothing=3)),
}


def settings_kw(st):
    return dict(b=st.smoothing, f_low=st.f_low_hz, f_high=st.f_high_hz, transition=st.transition_octaves,
                reg_in=st.regularisation_db, reg_out=st.outside_db, tilt=st.tilt_db_per_octave, max_boost_db=st.max_boost_db,
                points_per_octave=st.points_per_octave, f_min=st.f_min_hz, f_max=st.f_max_hz)


_RUNS = {}


def run(name):
    """The device's records of a case with everything kept, fetched once: dict(rec, chans, st, X, F, S, C, A, f)."""
    if name not in _RUNS:
        D, eng = _eq(), _eng()
        lengths, kw = CASES[name]
        st = D.EqualiseSettings(**kw)
        chans = [channel(n, q) for q, n in enumerate(lengths)]
        rec = D.equalise_device(eng, eng.upload(chans), FS, st, keep=True)
        assert len(rec.kept) == 1
        k = rec.kept[0]
        nb = rec.n_fft // 2 + 1
        cplx = lambda t, off: [t.cpu().numpy().view(np.complex128)[int(o) : int(o) + nb] for o in off]
        _RUNS[name] = dict(rec=rec, chans=chans, st=st, members=k["members"], X=cplx(k["spec"], k["spec_off"]),
                           F=cplx(k["fspec"], k["fspec_off"]), S=k["s"].cpu().numpy(), A=k["a"].cpu().numpy(),
                           C=cplx(k["c"], k["c_off"]), f=k["f"].cpu().numpy(), ref=k["ref"])
    return _RUNS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_equal_the_restatement_on_the_device_spectra(name):
    D = _eq()
    r = run(name)
    rec, st = r["rec"], r["st"]
    n = rec.n_fft
    lengths = CASES[name][0]
    assert n == int(name.split()[0][1:]) and np.array_equal(rec.segment, lengths)
    names = [f"ch{q}" for q in range(len(lengths))]
    results = D.equalise_results(rec, FS, names)
    assert len(results) == len(rec.rows) == (1 if st.average else len(lengths))
    for row, members in enumerate(r["members"]):
        specs = [r["X"][m] for m in members]
        d = R.design(specs, n, float(FS), **settings_kw(st))
        assert same(r["S"][row], d["S"]), (name, row, "S")
        assert d["ref"] == r["ref"][row] == rec.ref[row] and R.valid(d["ref"])
        assert same(r["C"][row].real, d["c"]) and not r["C"][row].imag.any(), (name, row, "c")
        assert int(rec.clamped[row]) == d["clamped"], (name, row)
        a = R.power(specs, r["F"][row])
        a_s = R.smooth(a, d["lo"], d["hi"])
        assert same(r["A"][row], a_s), (name, row, "A")
        k = d["bins"]
        assert np.array_equal(rec.bins, k) and np.array_equal(rec.in_band, d["in_band"]) and same(rec.target, d["t"][k])
        assert same(rec.s_grid[row], d["S"][k]) and same(rec.c_grid[row], d["c"][k]) and same(rec.a_grid[row], a_s[k])
        want = R.arithmetic(d["S"][k], d["c"][k], a_s[k], d["t"][k], k, d["in_band"], n, d["ref"], d["clamped"], float(FS))
        got = results[row]
        for key, v in want.items():
            assert same(getattr(got, key), v) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else np.array_equal(getattr(got, key), v), (name, key)
        assert got.fft_size == n and got.taps == st.taps and got.members == tuple(names[m] for m in rec.rows[row])
        assert got.name == ("average" if st.average else names[row])
    if name == "N64 b3":
        assert rec.clamped.sum() > 0                                         # a 3 dB ceiling engages
    if st.average:
        assert rec.rows == [[0, 1, 2]] and r["members"] == [[0, 1, 2]]       # the members in the order given
        mean = np.zeros(n // 2 + 1)
        for x in r["X"]:
            mean = mean + (x.real * x.real + x.imag * x.imag)
        assert same(R.power(r["X"]), mean / 3.0)


@pytest.mark.parametrize("name", list(CASES))
def test_filter_against_the_float64_restatement_on_the_same_c(name):
    r = run(name)
    n, taps = r["rec"].n_fft, r["st"].taps
    v = R.taper(taps, r["st"].fade)
    worst = 0.0
    for row in range(len(r["members"])):
        ch = R.filter_chain(r["C"][row].real, n)
        bound = R.FilterBounds(ch).filter(ch, v)
        err = np.abs(r["f"][row].astype(np.float64) - ch["g"][:taps] * v)
        worst = max(worst, float(np.max(err / bound)))
    print(f"equalise filter error / bound [{name}]: {worst:.4f}")
    assert worst <= 1.0, (name, worst)
    assert r["f"].dtype == np.float32 and np.all(np.isfinite(r["f"]))


@pytest.mark.parametrize("name", list(CASES))
def test_c_against_the_restatement_from_numpys_own_transform(name):
    r = run(name)
    rec, st = r["rec"], r["st"]
    n = rec.n_fft
    worst = 0.0
    for row, members in enumerate(rec.rows):
        specs = [np.fft.rfft(r["chans"][m].astype(np.float64), n=n) for m in members]
        e_x = max(R.forward_error(r["chans"][m], n) for m in members)
        d = R.design(specs, n, float(FS), **settings_kw(st))
        bound = R.log_c_bound(d["S"], d["S"][d["bins"]][d["in_band"]], e_x)
        err = np.abs(np.log(r["C"][row].real) - np.log(d["c"]))
        worst = max(worst, float(np.max(err / bound)))
    print(f"equalise ln c error / bound [{name}]: {worst:.4f}")
    assert worst <= 1.0, (name, worst)


def _closed(x, want_over_root_ref, **kw):
    D, eng = _eq(), _eng()
    st = D.EqualiseSettings(**kw)
    rec = D.equalise_device(eng, eng.upload([x]), FS, st, keep=True)
    n, taps = rec.n_fft, st.taps
    assert n == 256 and taps == 128
    f = rec.kept[0]["f"].cpu().numpy()[0].astype(np.float64)
    c_dev = rec.kept[0]["c"].cpu().numpy()[0::2][: n // 2 + 1]
    d = R.design([np.fft.rfft(x.astype(np.float64), n=n)], n, float(FS), **settings_kw(st))
    v = R.taper(taps, st.fade)
    ch = R.filter_chain(c_dev, n)
    dlnc = float(np.max(R.log_c_bound(d["S"], d["S"][d["bins"]][d["in_band"]], R.forward_error(x, n))))
    root = math.sqrt(d["ref"])
    bound = R.FilterBounds(ch).filter(ch, v) + R.input_term(d["c"], dlnc, n, v) + root * R.closed_bound(n)
    ratio = float(np.max(np.abs(f - root * want_over_root_ref) / bound))
    assert ratio <= 1.0, ratio
    return ratio, rec


def test_closed_forms_on_the_device():
    delta = np.zeros(128)
    delta[0] = 1.0
    x = np.zeros(40, dtype=np.float32)
    x[0] = 1.0
    a, rec = _closed(x, delta, taps=128, smoothing=0)
    assert abs(rec.ref[0] - 1.0) < 1e-12 and np.max(np.abs(rec.c_grid - 1.0)) < 1e-12 and rec.clamped[0] == 0
    want = delta.copy()
    want[1] = -0.5
    b, rec = _closed(R.one_pole(64), want, taps=128, smoothing=0, regularisation_db=-300.0, outside_db=-300.0, max_boost_db=200.0)
    print(f"equalise closed forms error / bound: impulse {a:.4f}, one pole {b:.4f}")
    res = _eq().equalise_results(rec, FS, ["pole"])[0]
    assert res.deviation_after_db < 1e-4 < 0.5 < res.deviation_before_db     # the prediction is flat at the reference level
    assert np.max(np.abs(res.after_db)) < 1e-4


def test_rows_without_values_touch_no_other_row():
    D, eng = _eq(), _eng()
    st = D.EqualiseSettings(taps=64, smoothing=3, n_fft=1024)
    good = [channel(400, 1), channel(300, 2)]
    nan = channel(400, 3).copy()
    nan[17] = np.nan
    inf = channel(200, 4).copy()
    inf[5] = np.inf
    chans = [good[0], np.zeros(300, dtype=np.float32), nan, good[1], inf, np.zeros(0, dtype=np.float32)]
    filters = D.equalisation_filters(chans, FS, st, eng=eng)
    alone = D.equalisation_filters(good, FS, st, eng=eng)
    assert len(filters) == 6 and all(f.dtype == np.float32 and f.shape == (64,) for f in filters)
    assert np.array_equal(filters[0], alone[0]) and np.array_equal(filters[3], alone[1]) and np.isfinite(alone[0]).all()
    assert all(np.isnan(filters[q]).all() for q in (1, 2, 4, 5))
    res = D.analyse_equalise_batch(chans, FS, [f"c{q}" for q in range(6)], st)
    ok = D.analyse_equalise_batch(good, FS, ["c0", "c3"], st)
    for q, want in ((0, ok[0]), (3, ok[1])):
        assert res[q].reference_level_db == want.reference_level_db and same(res[q].after_db, want.after_db)
        assert same(res[q].correction_db, want.correction_db) and res[q].clamped_share == want.clamped_share
    for q in (1, 2, 4, 5):
        assert math.isnan(res[q].reference_level_db) and math.isnan(res[q].clamped_share) and math.isnan(res[q].deviation_after_db)
        assert np.isnan(res[q].before_db).all() and np.isnan(res[q].correction_db).all() and np.isnan(res[q].after_db).all()
        assert np.isfinite(res[q].target_db).all() and np.array_equal(res[q].bin, res[0].bin)
    assert "NaN" not in json.dumps(D.equalise_results_to_json(res))
    # an average with a silent member is the mean power of all of them; with a NaN member it has no values
    avg = D.EqualiseSettings(taps=64, smoothing=3, n_fft=1024, average=True)
    with_silence = D.analyse_equalise_batch([good[0], np.zeros(300, dtype=np.float32)], FS, ["a", "b"], avg)[0]
    assert with_silence.members == ("a", "b") and abs(with_silence.reference_level_db - (ok[0].reference_level_db - 10.0 * math.log10(2.0))) < 1e-9
    assert math.isnan(D.analyse_equalise_batch([good[0], nan], FS, ["a", "b"], avg)[0].reference_level_db)
    with pytest.raises(ValueError, match="empty"):
        D.analyse_equalise_batch([good[0], np.zeros(0, dtype=np.float32)], FS, ["a", "b"], avg)
    with pytest.raises(ValueError, match="at most"):
        D.analyse_equalise_batch([good[0]] * 257, FS, [str(q) for q in range(257)], avg)


def test_post_ms_and_the_cut_into_sub_batches(monkeypatch):
    D, eng = _eq(), _eng()
    from audio_analysis_amd import engine as E
    chans = [channel(900, 11), channel(700, 12), channel(800, 13)]
    st = D.EqualiseSettings(taps=64, smoothing=6, n_fft=2048, post_ms=5.0)
    rec = D.equalise_device(eng, eng.upload(chans), FS, st)
    assert rec.segment.tolist() == [3 + 1 + 240] * 3                         # the peak at sample 3, 5 ms = 240 samples
    cut = D.EqualiseSettings(taps=64, smoothing=6, n_fft=2048)
    short = D.equalise_device(eng, eng.upload([c[:244] for c in chans]), FS, cut)
    whole = rec.filters.cpu().numpy()
    assert np.array_equal(whole, short.filters.cpu().numpy()) and same(rec.a_grid, short.a_grid) and same(rec.ref, short.ref)
    # no result depends on the cut: a row a sub-batch
    monkeypatch.setattr(E, "equalise_cut", lambda n, members, scratch_bytes=0: [(q, q + 1) for q in range(len(members))])
    single = D.equalise_device(eng, eng.upload(chans), FS, st, keep=True)
    assert len(single.kept) == 3
    assert np.array_equal(single.filters.cpu().numpy(), whole) and same(single.a_grid, rec.a_grid) and same(single.c_grid, rec.c_grid)
    assert same(single.s_grid, rec.s_grid) and np.array_equal(single.clamped, rec.clamped)


def test_cli_on_a_stereo_wav_equals_the_python_api(tmp_path):
    D = _eq()
    chans = [channel(3000, 21), channel(3000, 22)]
    wav = tmp_path / "room.wav"
    wav.write_bytes(O.recorder_wav_bytes(0.15 * np.stack(chans, axis=1).reshape(-1), FS))
    env = dict(os.environ, PYTHONPATH=str(REPO))
    out_json, out_dir = tmp_path / "room.json", tmp_path / "eq"
    args = ["--taps", "512", "--smoothing", "3", "--post-ms", "20", "--points-per-octave", "6", "--f-min", "50",
            "--max-boost-db", "6", "--tilt-db-per-octave", "-0.5"]
    r = subprocess.run([sys.executable, "-m", "analyse.equalise", "--input", str(wav), *args, "--json", str(out_json),
                        "--write-filters", str(out_dir)], capture_output=True, text=True, cwd=str(REPO), env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "NaN" not in out_json.read_text()
    doc = json.loads(out_json.read_text())
    st = D.EqualiseSettings(taps=512, smoothing=3, post_ms=20.0, points_per_octave=6, f_min_hz=50.0, max_boost_db=6.0,
                            tilt_db_per_octave=-0.5)
    api = D.analyse_equalise_files([wav], st)
    assert [d["name"] for d in doc["equalisation"]] == ["room.wav:left", "room.wav:right"]
    assert doc == D.equalise_results_to_json(api) and r.stdout == D.summarise_equalise_text(api)
    assert doc["equalisation"][0]["fft_size"] == 2048 and len(doc["equalisation"][0]["after_db"]) == 52
    assert all(d["deviation_after_db"] < d["deviation_before_db"] for d in doc["equalisation"])
    from scipy.io import wavfile
    rate, h = wavfile.read(str(out_dir / "room_eq.wav"))
    assert rate == FS and h.dtype == np.float32 and h.shape == (512, 2)
    loaded = [c for _, c in __import__("audio_analysis_amd.analyse._common", fromlist=["wav_channels"]).wav_channels(wav, False)[1]]
    want = D.equalisation_filters(loaded, FS, st)
    assert np.array_equal(h[:, 0], want[0]) and np.array_equal(h[:, 1], want[1])
    written = D.write_filter_files([wav], tmp_path / "avg", D.EqualiseSettings(taps=512, smoothing=3, average=True))
    rate, h = wavfile.read(str(written[0]))
    assert written[0].name == "average_eq.wav" and h.shape == (512,) or h.shape == (512, 1)
