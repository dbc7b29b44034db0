"""GPU: the report blocks at sample rates other than 48 kHz (the table of tests/rates_cases.py), against the oracle, which
tests/test_rates_cpu.py pins to the reference's own outputs at these rates (tests/golden/rates.npz, rates.json).

  * masks: ira_band_mask_values for every band of every table (9 rates x 3 modes x 4 lengths) bit for bit against
    O.band_mask on the float32 axis of the rate, and against the reference's own arrays where the fixture holds them;
  * band signals: Engine.band_irfft of the device's own spectrum of a white-noise channel through the tables' records on
    the bin step sr / n -- every band of every table at all four lengths (at 23 257 and 30 007 dealt over 2 and 10 cases per
    rate) -- sparse_bands on and off, paired and alone, into sentinel-gapped output: every signal within
    longfft_ref.band_bound of irfft_masked_ref (test_gpu_longfft_edges.check_band, bound unchanged), every gap untouched.
    The degenerate records (lp_x0 == lp_x1 == Nyquist: the top octave band at 8 000, 11 025, 16 000, 22 050 and 44 100 Hz -- and at 32 000 Hz, whose masks are compared --
    the top third-octave band at 11 025 and 22 050 Hz) run as the first member of a pair, as the second, and alone (the
    half-length inverse at the direct lengths);
  * every block through its public function at 11 025, 22 050, 44 100 and 96 000 Hz with the assertions and tolerances of
    the 48 kHz tests; the modal cloud also at 8 000 Hz (no point at all) and 192 000 Hz (95 empty low log bins);
  * the whole report at these rates column by column as smoke() checks it, at 44 100 Hz also in octave and third mode (the
    M_BANDS columns past the table's band count stay NaN), one batch against channels alone (same bytes), and a bundle in
    the recorder's format whose meta.json says 44 100.

Findings.  The kernels were right at every rate: the `degenerate` branch of csrc/ira_bandmask.h, the clamp of the support
in band_compact_kernel and the Bluestein inverse hold bit for bit (masks) and within the bound (signals); the worst
error / bound ratios are printed when the module finishes (RATES-RATIO lines; recorded in DESIGN.md).  One host bug:
analyse/bundle.py run_bundle_metrics read the rate from meta.json for the ingest's header check only and ran the report
itself with FullReportSettings() -- 48 000 Hz -- so every segment bound, band table and frequency of a 44.1 kHz bundle was
that of a 48 kHz one.  Fixed there (the report runs at the bundle's rate; settings for another rate are refused);
test_bundle_at_44100_equals_the_report_on_the_uploaded_floats fails without the fix."""
import warnings
from dataclasses import replace

import numpy as np
import pytest

import rates_cases as RC
import test_gpu_longfft_edges as E
from oracle import ira_oracle as O

pytestmark = pytest.mark.gpu
NAMES = ["a", "b", "c"]


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.fixture(scope="module", autouse=True)
def _print_ratios():
    yield
    for key in sorted(k for k in E.RATIOS if k[0].startswith("inverse rates")):
        r = E.RATIOS[key]
        print(f"RATES-RATIO {key[0]:40s} worst error/bound {r[0]:.4f}  ({r[3]})")


@pytest.fixture(scope="module")
def fx():
    return RC.load_fixture()


# ================================================================================================ masks
@pytest.mark.parametrize("sr", RC.TABLE_RATES)
def test_mask_values_bit_for_bit_at_every_rate(fx, sr):
    from audio_analysis_amd.analyse import rt60bands as rb
    from audio_analysis_amd.analyse.frequency_response import rfft_bin_step
    g, meta = fx
    eng = E._eng()
    nyq = 0.5 * float(sr)
    against_reference = 0
    for mode in RC.MODES:
        st = rb.Rt60BandsAnalysisSettings(band_mode=mode)
        bands = rb._build_band_definitions(st, sr)
        obands = O.band_definitions(sr, band_mode=mode)
        assert len(bands) == len(obands)
        for n in RC.LENGTHS:
            nb, f, fv = n // 2 + 1, RC.axis(n, sr), rfft_bin_step(n, sr)
            for i, (b, ob) in enumerate(zip(bands, obands)):
                rec = rb.band_mask_record(b, st.transition_width_octaves, nyq)
                got = E._mask_values(eng, rec, fv, nb)
                assert RC.same_bits(got, O.band_mask(f, ob, RC.TRANSITION_OCT, nyq)), (sr, mode, n, b.name)
                key = f"mask/{sr}/{mode}/{n}/{i}"
                if key in g.files:
                    assert RC.same_bits(got, g[key]), (sr, mode, n, b.name)
                    against_reference += 1
    assert against_reference >= 2 * 3 * len(RC.MASK_GOLDEN_LENGTHS)


# ================================================================================================ band signals
# band-signal cases per length: the long-double reference of one band takes about 0.02 s at 4 800, 0.1 s at 28 800, 0.2 s
# at 23 257 and 1 s at 30 007 (= 37 x 811, a prime leaf of 811 by the direct sum), so the bands of a rate are dealt over this
# many cases (entries part, part + PARTS, ...): every band of every table runs at every length, each case in a few seconds
PARTS = {4800: 1, 28800: 1, 23257: 2, 30007: 10}
BAND_CASES = [(sr, n, part) for sr in RC.RATES for n in RC.LENGTHS for part in range(PARTS[n])]


def _entries(sr, n, meta):
    """(name, record, oracle mask, degenerate) of every band of every table (three, octave, third) at rate sr, length n."""
    from audio_analysis_amd.analyse import rt60bands as rb
    nyq = 0.5 * float(sr)
    f = RC.axis(n, sr)
    out = []
    for mode in RC.MODES:
        st = rb.Rt60BandsAnalysisSettings(band_mode=mode)
        bands = rb._build_band_definitions(st, sr)
        obands = O.band_definitions(sr, band_mode=mode)
        deg = set(meta["degenerate"][f"{sr}/{mode}"])
        pick = range(len(bands))
        for i in pick:
            rec = rb.band_mask_record(bands[i], st.transition_width_octaves, nyq)
            assert RC.is_degenerate(rec) == (i in deg)
            out.append((f"{mode}/{bands[i].name}", rec, O.band_mask(f, obands[i], RC.TRANSITION_OCT, nyq), i in deg))
    return out


@pytest.mark.parametrize("sr,n,part", BAND_CASES)
def test_band_signals_at_the_real_tables(fx, sr, n, part):
    from audio_analysis_amd.analyse.frequency_response import rfft_bin_step
    from audio_analysis_amd.engine_plan import band_pairs
    _, meta = fx
    eng = E._eng()
    nb, fv = n // 2 + 1, rfft_bin_step(n, sr)
    direct = n in RC.DIRECT_LENGTHS
    assert (eng.smooth_split(n) is not None) == direct
    b = eng.upload([RC.noise_channel(n)])
    spec, so = eng.rfft_any(b.x, b.off, np.array([n], np.int32), False)
    X = spec.cpu().numpy().reshape(-1, 2)
    X = X[:nb, 0] + 1j * X[:nb, 1]
    every = _entries(sr, n, meta)
    assert len(every) == sum(len(meta["tables"][f"{sr}/{mode}"]) for mode in RC.MODES)
    assert any(e[3] for e in every) == any(rate == sr for rate, _ in RC.DEGENERATE)
    ent = every[part :: PARTS[n]]
    assert len(ent) >= 2
    norms = [E.masked_norm(X, m, n) for _, _, m, _ in ent]
    roles = set()

    def run(idx, label):
        """One band_irfft call of the entries idx (in that order); every signal checked; returns the planner's pairing."""
        recs = [ent[i][1] for i in idx]
        so_all = np.full(len(idx), so[0], np.int64)
        fvs = np.full(len(idx), fv)
        got, _ = E.run_bands(eng, spec, so_all, n, recs, fvs)
        j1, j2 = band_pairs(so_all, np.full(len(idx), n, np.int32), np.stack(recs), fvs, eng._switches())
        pn, paired = E.partner_norms(j1, j2, [norms[i] for i in idx])
        for p, i in enumerate(idx):
            name, _, mask, _ = ent[i]
            E.check_band(got[p], X, mask, n, bool(paired[p]), label, f"noise {sr} {name}", pn[p])
        return j1, j2

    for sparse in (True, False):
        label = f"rates sparse={int(sparse)}"
        with E.switches(eng, sparse_bands=sparse):
            j1, j2 = run(list(range(len(ent))), label)                         # the tables as they are: pairs, one left over
            for a, c in zip(j1, j2):
                if ent[a][3] and c >= 0:
                    roles.add("first")
                if c >= 0 and ent[c][3]:
                    roles.add("second")
            for i in range(len(ent)):                                          # every band alone
                run([i], label)
                if direct:
                    assert eng.last_band_info_half == [True], (sr, n, ent[i][0])
                if ent[i][3]:
                    roles.add("alone")
            for d in [i for i, e in enumerate(ent) if e[3]]:                   # a degenerate record in either seat of a pair
                q = d - 1 if d > 0 else d + 1
                j1, j2 = run([d, q], label)
                assert (j1.tolist(), j2.tolist()) == ([0], [1])
                roles.add("first")
                j1, j2 = run([q, d], label)
                assert (j1.tolist(), j2.tolist()) == ([0], [1])
                roles.add("second")
                if direct:
                    assert eng.last_band_info_half == [False]
    has_deg = any(e[3] for e in ent)
    assert roles == ({"first", "second", "alone"} if has_deg else set()), (sr, n, part, roles)


# ================================================================================================ blocks against the oracle
@pytest.mark.parametrize("sr", RC.BLOCK_RATES)
def test_input_conditions_hold_on_the_oracle(sr):
    """Before the device is consulted: unique frequency-response peaks, T30 fits in at least half of the bands, no slice
    target on a frame boundary (rates_cases.check_input_conditions)."""
    RC.check_input_conditions(sr)


@pytest.mark.parametrize("mode", RC.MODES)
@pytest.mark.parametrize("sr", RC.BLOCK_RATES)
def test_rt60_bands_vs_oracle(sr, mode):
    from audio_analysis_amd.analyse import rt60bands as rb
    RC.check_input_conditions(sr)
    orc = RC.oracle_blocks(sr)
    st = rb.Rt60BandsAnalysisSettings(band_mode=mode, include_t20=True, include_edt=True)
    res = rb.analyse_rt60_bands_batch([r["x"] for r in orc], sr, NAMES, st)
    worst = 0.0
    for r, o in zip(res, orc):
        ob = o[f"rt60bands/{mode}"]
        assert [b.name for b in r.band_definitions] == [b["name"] for b in ob["bands"]] == list(r.band_metrics_by_name)
        for name, m in r.band_metrics_by_name.items():
            want = ob["metrics"][name]
            for got_v, want_v in zip((m.rt60_t30_seconds, m.rt60_t20_seconds, m.edt_seconds),
                                     (want["t30"], want["t20"], want["edt"])):
                assert (got_v is None) == (want_v is None), (sr, mode, name, got_v, want_v)
                if want_v is not None:
                    worst = max(worst, _rel(got_v, want_v))
    assert worst < 1e-4, worst
    mine = [{k: (m.rt60_t30_seconds, m.rt60_t20_seconds, m.edt_seconds) for k, m in r.band_metrics_by_name.items()}
            for r in res]
    assert rb.summarise_rt60_bands_results_text(res, True, True) == \
        RC.bands_summary_text(NAMES, [b.name for b in res[0].band_definitions], mine)


@pytest.mark.parametrize("sr", RC.BLOCK_RATES)
def test_fr_and_filter_vs_oracle(sr):
    from audio_analysis_amd.analyse import filterplot, frequency_response as fr
    RC.check_input_conditions(sr)
    orc = RC.oracle_blocks(sr)
    chans = [r["x"] for r in orc]
    # the white-noise channel at the smallest direct length rides along in the frequency-response batch
    noise = RC.noise_channel(4800)
    on = O.analyse_frequency_response(noise, sr)
    assert RC.fr_peak_gap_db(on, sr) > 1e-3
    res = fr.analyse_frequency_response_batch(chans + [noise], sr, NAMES + ["noise"], fr.FrequencyResponseAnalysisSettings())
    for r, o in zip(res, [x["fr"] for x in orc] + [on]):
        assert (r.analysis_start_sample_index, r.analysis_length_samples) == (o["start"], o["length"])
        np.testing.assert_array_equal(r.frequency_hz, np.fft.rfftfreq(o["length"], 1.0 / float(sr)).astype(np.float32))
        assert r.magnitude_db.shape == o["magnitude_db"].shape and r.magnitude_db.dtype == np.float32
        np.testing.assert_allclose(r.magnitude_db, o["magnitude_db"], rtol=0, atol=2e-5)
        assert r.peak_frequency_hz == o["peak_hz"]
        assert _rel(r.spectral_centroid_hz, o["centroid_hz"]) < 1e-9
    res = filterplot.analyse_filter_response_batch(chans, sr, NAMES, filterplot.FilterAnalysisSettings())
    for r, x in zip(res, orc):
        o = x["filter"]
        assert (r.analysis_start_sample_index, r.analysis_length_samples) == (o["start"], o["length"])
        np.testing.assert_array_equal(r.frequency_hz, o["frequency_hz"])
        np.testing.assert_allclose(r.magnitude_db, o["magnitude_db"], rtol=0, atol=2e-5)
        assert r.peak_frequency_hz == o["peak_hz"]
        assert abs(r.magnitude_at_1khz_db - o["mag_1k_db"]) < 2e-5
        ph_ref = o["phase"]
        assert np.max(np.abs(r.phase_response - ph_ref) / np.maximum(1.0, np.abs(ph_ref))) < 1e-6


@pytest.mark.parametrize("sr", RC.BLOCK_RATES)
def test_waterfall_and_spectrogram_vs_oracle(sr):
    from audio_analysis_amd.analyse import spectrogram, waterfall as wf
    RC.check_input_conditions(sr)
    orc = RC.oracle_blocks(sr)
    chans = [r["x"] for r in orc]
    res = wf.analyse_waterfall_batch(chans, sr, NAMES, wf.WaterfallAnalysisSettings())
    for r, x in zip(res, orc):
        o = x["waterfall"]
        assert (r.analysis_start_sample_index, r.analysis_length_samples) == (o["start"], o["length"])
        np.testing.assert_array_equal(r.slice_times_seconds, o["slice_times_seconds"])        # slice indices: exact
        ws = wf.WaterfallAnalysisSettings()
        frames = 1 + (o["length"] - ws.n_fft) // ws.hop_length
        picks = wf._select_slice_frame_indices(O.frame_times(frames, ws.hop_length, sr), ws)
        np.testing.assert_array_equal(picks, o["frame_indices"])
        np.testing.assert_array_equal(r.frequency_hz, o["frequency_hz"])                       # k_lo / nsel: exact rows
        assert r.slice_magnitude_rel_db.shape == o["slice_rel_db"].shape
        np.testing.assert_allclose(r.slice_magnitude_rel_db, o["slice_rel_db"], rtol=0, atol=3e-5)
    res = spectrogram.analyse_spectrogram_batch(chans, sr, NAMES, spectrogram.SpectrogramAnalysisSettings())
    for r, x in zip(res, orc):
        o = x["spectrogram"]
        assert (r.analysis_start_sample_index, r.analysis_length_samples) == (o["start"], o["length"])
        assert r.magnitude_db.shape == o["magnitude_db"].shape                                  # frame count: exact
        np.testing.assert_array_equal(r.frequency_hz, o["frequency_hz"])
        np.testing.assert_array_equal(r.time_seconds, o["time_seconds"])


@pytest.mark.parametrize("sr", RC.BLOCK_RATES + RC.MODAL_ONLY_RATES)
def test_modal_cloud_vs_oracle(sr):
    from audio_analysis_amd.analyse import modalcloud as mc
    eng = E._eng()
    chans = RC.block_channels(sr)
    orc = [O.analyse_modal_cloud(x, sr) for x in chans] if sr in RC.MODAL_ONLY_RATES else \
        [r["modal"] for r in RC.oracle_blocks(sr)]
    nyq = 0.5 * float(sr)
    f_lo, f_hi = float(np.clip(20.0, 1.0, nyq)), float(np.clip(20000.0, 20.0, nyq))
    freq = np.fft.rfftfreq(8192, 1.0 / float(sr)).astype(np.float32)
    sel = freq[(freq >= f_lo) & (freq <= f_hi)]
    edges = mc._build_log_bins(f_lo, f_hi, 24, 24)
    cen, first, count = mc.log_bin_rows(sel, edges)
    cen_o, first_o, count_o = O.log_bin_membership(sel, O.log_bin_edges(f_lo, f_hi, 24, 24))
    np.testing.assert_array_equal(cen, cen_o)
    np.testing.assert_array_equal(count, count_o)
    np.testing.assert_array_equal(first[count > 0], first_o[count_o > 0])
    st = mc.ModalCloudAnalysisSettings()
    dev = mc.modal_cloud_device(eng, eng.upload(chans), sr, st)
    res = mc.modal_records_to_results(dev, dev["fits"].cpu().numpy(), sr, NAMES)
    cur = dev["curves"].cpu().numpy()
    nbins, cols = int(dev["nbins"]), np.asarray(dev["cols"], np.int64)
    assert nbins == cen_o.size
    off = np.cumsum(cols * nbins) - cols * nbins
    for i, (r, o) in enumerate(zip(res, orc)):
        assert (r.analysis_start_sample_index, r.analysis_length_samples) == (o["start"], o["length"])
        ref = o["curves"]
        got = cur[off[i] : off[i] + nbins * cols[i]].reshape(nbins, cols[i])
        assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)), (sr, i)
        assert np.array_equal(np.isnan(ref[:, 0]), count_o == 0)               # the empty log bins, and only they
        ok = ~np.isnan(ref)
        np.testing.assert_allclose(got[ok], ref[ok], rtol=0, atol=2e-5)
        assert len(r.points) == len(o["points"]), (sr, i, len(r.points), len(o["points"]))
        for p, q in zip(r.points, o["points"]):
            assert p.centre_hz == q[0] and _rel(p.rt60_seconds, q[1]) < 1e-4
    if sr == 8000:
        assert all(len(r.points) == 0 for r in res)
    if sr == 192000:
        assert int((count == 0).sum()) >= 90


# ================================================================================================ the whole report
def _report(eng, sr, chans, mode="three"):
    from audio_analysis_amd import pipeline as P
    from audio_analysis_amd.analyse import rt60bands as rb
    s = replace(P.FullReportSettings(), sample_rate_hz=sr, rt60_bands=rb.Rt60BandsAnalysisSettings(band_mode=mode))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return P.FullReport(eng, s).run(eng.upload(chans))


def _check_report(m, sr, mode):
    """smoke()'s assertions, column by column, at rate sr; and the band columns past the table stay NaN."""
    from audio_analysis_amd import pipeline as P
    for i, o in enumerate(RC.oracle_blocks(sr)):
        assert m[i, P.M_STATUS] == 0 and int(m[i, P.M_NSAMPLES]) == o["x"].size
        d = o["decay"]
        assert int(m[i, P.M_START]) == d["start"]
        assert abs(m[i, P.M_FIT_T30 + 6] - d["fits"]["T30"]["rt60"]) <= 1e-6 * d["fits"]["T30"]["rt60"]
        b = o[f"rt60bands/{mode}"]
        nb = len(b["bands"])
        assert int(m[i, P.M_NBANDS]) == nb <= P.MAX_BANDS
        for k, band in enumerate(b["bands"]):
            ref = b["metrics"][band["name"]]["t30"]
            got = m[i, P.M_BANDS + 3 * k]
            assert (ref is None) == bool(np.isnan(got)), (sr, mode, i, band["name"])
            if ref is not None:
                assert abs(got - ref) <= 1e-4 * abs(ref)
        assert np.all(np.isnan(m[i, P.M_BANDS + 3 * nb : P.M_BANDS + 3 * P.MAX_BANDS])), (sr, mode, i, nb)
        f = o["fr"]
        assert m[i, P.M_FR_PEAK] == f["peak_hz"] and abs(m[i, P.M_FR_CENTROID] - f["centroid_hz"]) < 1e-6 * f["centroid_hz"]
        assert m[i, P.M_FILT_PEAK] == o["filter"]["peak_hz"]
        z = o["zplane"]
        assert abs(m[i, P.M_AR_MAX_R] - z["max_radius"]) < 1e-6 and int(m[i, P.M_AR_UNSTABLE]) == z["unstable"]
        assert int(m[i, P.M_MODAL_POINTS]) == len(o["modal"]["points"])
        assert int(m[i, P.M_SPEC_FRAMES]) == o["spectrogram"]["magnitude_db"].shape[1]
        w = o["waterfall"]
        assert (int(m[i, P.M_WF_SLICES]), int(m[i, P.M_WF_BINS])) == w["slice_rel_db"].shape


@pytest.mark.parametrize("sr,mode", [(sr, "three") for sr in RC.BLOCK_RATES] + [(44100, "octave"), (44100, "third")])
def test_full_report_columns_vs_oracle(sr, mode):
    RC.check_input_conditions(sr)
    eng = E._eng()
    m = _report(eng, sr, [r["x"] for r in RC.oracle_blocks(sr)], mode)
    _check_report(m, sr, mode)


def test_full_report_at_44100_one_batch_or_alone_gives_the_same_bytes():
    eng = E._eng()
    chans = RC.block_channels(44100)
    for mode in ("three", "third"):
        full = _report(eng, 44100, chans, mode)
        alone = [_report(eng, 44100, [x], mode) for x in chans]
        assert np.concatenate(alone, axis=0).tobytes() == full.tobytes(), mode


def test_bundle_at_44100_equals_the_report_on_the_uploaded_floats(tmp_path):
    """Three taps as the recorder writes them (16-bit stereo, 44 100 in the header) and a meta.json that says 44 100:
    run_bundle_metrics gives, byte for byte, the records of FullReport at 44 100 Hz on the floats the ingest uploads
    (int16 / 32768), and those agree with the oracle at 44 100 Hz -- not the records of a 48 kHz report."""
    from audio_analysis_amd import pipeline as P
    from audio_analysis_amd.analyse import bundle
    eng = E._eng()
    sr = 44100
    root = tmp_path / "bundle"
    (root / "taps").mkdir(parents=True)
    taps, floats = ["t0", "t1", "t2"], []
    for ti, (tap, n) in enumerate(zip(taps, RC.BLOCK_LENGTHS)):
        st = np.stack([RC.synth(RC.BLOCK_SEED + 20 + 2 * ti + c, n, sr, RC.BLOCK_DECAYS[ti]) for c in (0, 1)], axis=1)
        blob = O.recorder_wav_bytes(st, sample_rate=sr)
        (root / "taps" / f"{tap}.wav").write_bytes(blob)
        rate, pcm = O.wav_pcm16_payload(blob)
        assert rate == sr and pcm.shape == (n, 2)
        floats += [O.pcm_to_float32(pcm[:, c]) for c in (0, 1)]
    (root / "meta.json").write_text(O.recorder_meta_json(sr, max(RC.BLOCK_LENGTHS), taps))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        labels, rec = bundle.run_bundle_metrics(root)
        want = P.FullReport(eng, replace(P.FullReportSettings(), sample_rate_hz=sr)).run(eng.upload(floats))
        at48k = P.FullReport(eng).run(eng.upload(floats))
    assert labels == [(t, ch) for t in taps for ch in ("left", "right")]
    assert rec.shape == want.shape and rec.tobytes() == want.tobytes()
    assert rec.tobytes() != at48k.tobytes()
    for i, x in enumerate(floats):
        f = O.analyse_frequency_response(x, sr)
        assert RC.fr_peak_gap_db(f, sr) > 1e-3
        assert rec[i, P.M_FR_PEAK] == f["peak_hz"] and _rel(rec[i, P.M_FR_CENTROID], f["centroid_hz"]) < 1e-6
        d = O.analyse_decay(x, sr)
        assert int(rec[i, P.M_START]) == d["start"] and _rel(rec[i, P.M_FIT_T30 + 6], d["fits"]["T30"]["rt60"]) < 1e-6
    with pytest.raises(ValueError):                              # settings for another rate than the bundle's are refused
        bundle.run_bundle_metrics(root, P.FullReportSettings())
