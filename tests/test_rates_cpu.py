"""CPU: sample rates other than 48 kHz.  tests/golden/rates.npz + rates.json hold what the reference itself returns for the
table of tests/rates_cases.py (band tables, mask arrays, block scalars; tests/golden/make_rate_goldens.py).  Here

  * the oracle reproduces that fixture -- masks and integers bit for bit, floats exactly as tests/test_oracle_vs_golden.py
    does (both sides ran the same NumPy) -- so that it can stand in for the reference on the GPU machine;
  * the product's host tables reproduce it exactly: _build_band_definitions, band_mask_record (degenerate exactly where the
    fixture says so), _build_log_bins / log_bin_rows, _select_slice_frame_indices;
  * the case table rejects the obvious wrong kernels, so that tests/test_gpu_rates.py cannot pass by accident: a mask
    computed with Nyquist 24 000, one computed on the bin step 48000 / n, and one whose degenerate ramp passes the Nyquist
    bin, each differ in bits from the fixture at every rate of the table."""
import numpy as np
import pytest

import rates_cases as RC
from oracle import ira_oracle as O

NOT_48K = [sr for sr in RC.TABLE_RATES if sr != RC.CONTROL_RATE]


@pytest.fixture(scope="module")
def fx():
    return RC.load_fixture()


def _table(bands):
    return [[b["name"], b["centre_hz"], b["kind"], b["low_edge_hz"], b["high_edge_hz"]] for b in bands]


def _fit_list(f):
    return None if f is None else [f["range_hi"], f["range_lo"], f["start_t"], f["end_t"], f["slope"],
                                   f["intercept"], f["r2"], f["rt60"]]


def test_the_degenerate_rates_are_the_ones_the_case_table_names(fx):
    _, meta = fx
    got = {(int(k.split("/")[0]), k.split("/")[1]) for k, v in meta["degenerate"].items() if v}
    assert got == RC.DEGENERATE
    for key, idx in meta["degenerate"].items():
        assert idx in ([], [len(meta["tables"][key]) - 1]), key           # only ever the top band
    counts = {mode: sorted({len(meta["tables"][f"{sr}/{mode}"]) for sr in RC.TABLE_RATES}) for mode in RC.MODES}
    assert counts == {"three": [3], "octave": [7, 8, 9], "third": [20, 22, 23, 25, 26]}, counts


@pytest.mark.parametrize("sr", RC.TABLE_RATES)
def test_oracle_band_tables_and_masks_are_the_references(fx, sr):
    g, meta = fx
    nyq = 0.5 * float(sr)
    for mode in RC.MODES:
        bands = O.band_definitions(sr, band_mode=mode)
        assert _table(bands) == meta["tables"][f"{sr}/{mode}"]
        deg = meta["degenerate"][f"{sr}/{mode}"]
        for n in RC.MASK_GOLDEN_LENGTHS:
            f = RC.axis(n, sr)
            for i in RC.golden_mask_bands(len(bands), deg):
                ref = g[f"mask/{sr}/{mode}/{n}/{i}"]
                assert RC.same_bits(O.band_mask(f, bands[i], RC.TRANSITION_OCT, nyq), ref), (sr, mode, n, i)
                if i in deg and n % 2 == 0:
                    # the degenerate low-pass: every bin below Nyquist passes, the Nyquist bin does not
                    assert f[-1] == nyq and ref[-1] == 0.0 and ref[-2] > 0.0, (sr, mode, n, ref[-3:])


@pytest.mark.parametrize("sr", RC.TABLE_RATES)
def test_product_band_tables_and_records(fx, sr):
    from audio_analysis_amd.analyse import rt60bands as rb
    _, meta = fx
    nyq = 0.5 * float(sr)
    for mode in RC.MODES:
        bands = rb._build_band_definitions(rb.Rt60BandsAnalysisSettings(band_mode=mode), sr)
        assert [[b.name, b.centre_hz, b.kind, b.low_edge_hz, b.high_edge_hz] for b in bands] == meta["tables"][f"{sr}/{mode}"]
        assert len(bands) <= 26                                                    # pipeline.MAX_BANDS columns
        deg = meta["degenerate"][f"{sr}/{mode}"]
        for i, b in enumerate(bands):
            rec = rb.band_mask_record(b, RC.TRANSITION_OCT, nyq)
            assert RC.is_degenerate(rec) == (i in deg), (sr, mode, b.name, rec)
            if i in deg:
                assert rec[0] == 3.0 and rec[3] == rec[4] == nyq and rec[1] < rec[2] < nyq, rec
            # the record's edges are the ones the oracle's mask functions derive: the mask formula on the record itself
            ob = dict(kind=b.kind, low_edge_hz=b.low_edge_hz, high_edge_hz=b.high_edge_hz)
            for n in (4800, 23257):
                f = RC.axis(n, sr)
                assert RC.same_bits(RC.mask_from_record(rec, f), O.band_mask(f, ob, RC.TRANSITION_OCT, nyq)), (sr, mode, b.name)


@pytest.mark.parametrize("sr", RC.BLOCK_RATES + RC.MODAL_ONLY_RATES)
def test_modal_log_bins_and_rows(fx, sr):
    from audio_analysis_amd.analyse import modalcloud as mc
    g, _ = fx
    nyq = 0.5 * float(sr)
    f_lo, f_hi = float(np.clip(20.0, 1.0, nyq)), float(np.clip(20000.0, 20.0, nyq))
    edges = g[f"modal/edges/{sr}"]
    assert RC.same_bits(O.log_bin_edges(f_lo, f_hi, 24, 24), edges)
    assert RC.same_bits(mc._build_log_bins(f_lo, f_hi, 24, 24), edges)
    freq = np.fft.rfftfreq(8192, 1.0 / float(sr)).astype(np.float32)
    sel = freq[(freq >= f_lo) & (freq <= f_hi)]
    cen, first, count = mc.log_bin_rows(sel, edges)
    cen_o, first_o, count_o = O.log_bin_membership(sel, edges)
    assert RC.same_bits(cen, cen_o)
    np.testing.assert_array_equal(count, count_o)
    np.testing.assert_array_equal(first[count > 0], first_o[count_o > 0])
    assert np.all(first + count <= sel.size)
    if sr == 192000:
        assert int((count == 0).sum()) >= 90                    # bin step 23.4 Hz: the low log bins hold no row
    if sr == 8000:
        assert edges[-1] == np.float32(4000.0)                  # f_max clipped to Nyquist


@pytest.mark.parametrize("sr", RC.BLOCK_RATES)
def test_oracle_blocks_are_the_references(fx, sr):
    from audio_analysis_amd.analyse import waterfall as wf
    g, meta = fx
    for ci, r in enumerate(RC.oracle_blocks(sr)):
        case = meta["blocks"][f"{sr}/{ci}"]
        d, cd = r["decay"], case["decay"]
        assert (d["start"], int(d["edc_db"].size), d["early_10db"]) == (cd["start"], cd["n"], cd["early"])
        assert {k: _fit_list(v) for k, v in d["fits"].items()} == cd["fits"]
        for mode in RC.MODES:
            b = r[f"rt60bands/{mode}"]
            assert _table(b["bands"]) == meta["tables"][f"{sr}/{mode}"]
            assert {k: [m["t30"], m["t20"], m["edt"]] for k, m in b["metrics"].items()} == case[f"rt60bands/{mode}"]["metrics"]
        f, cf = r["fr"], case["fr"]
        assert (f["start"], f["length"], f["peak_hz"], f["centroid_hz"]) == (cf["start"], cf["length"], cf["peak"], cf["centroid"])
        f, cf = r["filter"], case["filter"]
        assert (f["start"], f["length"], f["peak_hz"], f["mag_1k_db"]) == (cf["start"], cf["length"], cf["peak"], cf["mag1k"])
        s, cs = r["spectrogram"], case["spectrogram"]
        assert (s["start"], s["length"], list(s["magnitude_db"].shape)) == (cs["start"], cs["length"], cs["shape"])
        w, cw = r["waterfall"], case["waterfall"]
        assert (w["start"], w["length"], w["frame_indices"].tolist()) == (cw["start"], cw["length"], cw["slices"])
        assert RC.same_bits(w["slice_times_seconds"], g[f"wf/times/{sr}/{ci}"])
        assert (float(w["frequency_hz"][0]), float(w["frequency_hz"][-1]), int(w["frequency_hz"].size)) == \
            (cw["f_first"], cw["f_last"], cw["f_bins"])
        # the product's slice selection on the float32 frame-time axis of this rate
        ws = wf.WaterfallAnalysisSettings()
        frames = 1 + (cw["length"] - ws.n_fft) // ws.hop_length
        got = wf._select_slice_frame_indices(O.frame_times(frames, ws.hop_length, sr), ws)
        assert got.tolist() == cw["slices"]
    RC.check_input_conditions(sr)


@pytest.mark.parametrize("sr", RC.BLOCK_RATES + RC.MODAL_ONLY_RATES)
def test_oracle_modal_cloud_is_the_references(fx, sr):
    _, meta = fx
    for ci, x in enumerate(RC.block_channels(sr)):
        case = meta["blocks"][f"{sr}/{ci}"]["modal"]
        r = O.analyse_modal_cloud(x, sr)
        assert (r["start"], r["length"], len(r["points"])) == (case["start"], case["length"], case["points"])
        assert [p[0] for p in r["points"]] == case["centres"]
        if sr == 8000:
            assert case["points"] == 0                           # hop 64 ms: fewer than min_fit_points frames in the decay


@pytest.mark.parametrize("sr", RC.BLOCK_RATES)
def test_band_summary_restatement_is_the_references_text(fx, sr):
    _, meta = fx
    for ci, r in enumerate(RC.oracle_blocks(sr)):
        for mode in RC.MODES:
            b = r[f"rt60bands/{mode}"]
            m = {k: (v["t30"], v["t20"], v["edt"]) for k, v in b["metrics"].items()}
            text = RC.bands_summary_text(["mono"], [d["name"] for d in b["bands"]], [m])
            assert text == meta["blocks"][f"{sr}/{ci}"][f"rt60bands/{mode}"]["summary"]


@pytest.mark.parametrize("sr", RC.TABLE_RATES)
def test_first_bin_walk_on_the_bin_steps_of_the_table(sr):
    """The cut search of csrc/ira_bandmask.h (an estimate c / step, then at most ten bins on the float32 axis) restated:
    for every edge of every record of the table, on every bin step sr / n of the table and both highest bins the kernels
    pass (n / 2 of a full-length job, the same of a half-length one), it settles, and on the bin the axis itself gives."""
    from audio_analysis_amd.analyse import rt60bands as rb
    from audio_analysis_amd.analyse.frequency_response import rfft_bin_step
    nyq = 0.5 * float(sr)
    unsettled = 0
    for mode in RC.MODES:
        st = rb.Rt60BandsAnalysisSettings(band_mode=mode)
        recs = [rb.band_mask_record(b, st.transition_width_octaves, nyq) for b in rb._build_band_definitions(st, sr)]
        for n in RC.LENGTHS:
            step = rfft_bin_step(n, sr)
            kmax = n // 2
            f = (np.arange(kmax + 1, dtype=np.float64) * step).astype(np.float32)
            assert np.array_equal(f, RC.axis(n, sr))
            for rec in recs:
                for x, strict in ((rec[1], True), (rec[2], False), (rec[3], True), (rec[4], False)):
                    c = np.float32(x)
                    want = int(np.searchsorted(f, c, side="right" if strict else "left"))
                    got = RC.first_bin_restated(c, strict, step, kmax)
                    unsettled += got < 0
                    assert got == want, (sr, mode, n, rec, x, strict, got, want)
    assert unsettled == 0


# ---------------------------------------------------------------------------------- planted errors the table must reject
def _masks(sr, mode, n, f, nyq):
    return [O.band_mask(f, b, RC.TRANSITION_OCT, nyq) for b in O.band_definitions(sr, band_mode=mode)]


def _differ(a, b):
    return [i for i, (x, y) in enumerate(zip(a, b)) if not RC.same_bits(x, y)]


@pytest.mark.parametrize("sr", NOT_48K)
def test_a_mask_computed_with_nyquist_24000_is_rejected(sr):
    """Nyquist enters the records only through the clipping of the edges, so it is the bands near the top that tell: at
    every rate of the table at least one band of the octave table differs, at both even lengths (where the axis has a
    Nyquist bin) -- and the three-band table, whose edges stay below every Nyquist here but 4 kHz, is not what tells."""
    for n in RC.DIRECT_LENGTHS:
        f = RC.axis(n, sr)
        bad = _differ(_masks(sr, "octave", n, f, 24000.0), _masks(sr, "octave", n, f, 0.5 * sr))
        assert bad, (sr, n)


@pytest.mark.parametrize("sr", NOT_48K)
def test_a_mask_computed_on_the_48k_bin_step_is_rejected(sr):
    for n in RC.LENGTHS:
        wrong = (np.arange(n // 2 + 1) * (1.0 / (n * (1.0 / 48000.0)))).astype(np.float32)
        for mode in RC.MODES:
            right = _masks(sr, mode, n, RC.axis(n, sr), 0.5 * sr)
            bad = _differ(_masks(sr, mode, n, wrong, 0.5 * sr), right)
            assert len(bad) == len(right), (sr, n, mode, bad)      # every band of every table


def test_a_degenerate_ramp_that_passes_the_nyquist_bin_is_rejected(fx):
    """ramp(f, x0, x1) with x1 <= x0 is the step f >= x1, so the low-pass 1 - ramp is 0 at f == Nyquist.  A kernel whose step
    is strict (or that leaves the bin to `f <= pass -> 1`) gives 1 there: different bits in the Nyquist bin of every
    degenerate band at the even lengths, the same bits in every other band."""
    g, meta = fx

    def lowpass_wrong(f, pass_hz, nyq):
        pass_hz = float(np.clip(pass_hz, 1.0, nyq))
        stop_hz = float(min(nyq, pass_hz * float(2.0 ** RC.TRANSITION_OCT)))
        if stop_hz <= pass_hz:
            return (f <= pass_hz).astype(np.float32)              # the planted error: the pass edge wins at f == stop == pass
        return O.lowpass_mask(f, pass_hz, RC.TRANSITION_OCT, nyq)

    seen = set()
    for sr in RC.TABLE_RATES:
        nyq = 0.5 * float(sr)
        f = RC.axis(4800, sr)
        for mode in ("octave", "third"):
            bands = O.band_definitions(sr, band_mode=mode)
            deg = meta["degenerate"][f"{sr}/{mode}"]
            for i in RC.golden_mask_bands(len(bands), deg):
                b = bands[i]
                lo, hi = float(np.clip(b["low_edge_hz"], 1.0, nyq)), float(np.clip(b["high_edge_hz"], 1.0, nyq))
                wrong = (O.highpass_mask(f, lo, RC.TRANSITION_OCT, nyq) * lowpass_wrong(f, hi, nyq)).astype(np.float32)
                same = RC.same_bits(wrong, g[f"mask/{sr}/{mode}/4800/{i}"])
                assert same == (i not in deg), (sr, mode, i)
                if i in deg:
                    seen.add((sr, mode))
    assert seen == RC.DEGENERATE
