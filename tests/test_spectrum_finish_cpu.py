"""
ira_spectrum_finish without a GPU: the entry point's argument validation through the loaded library, the library calls
spectrum_device and group_delay_device make (tests/host_engine.HostEngine records them instead of running them), and the
planted conditions of the GPU tests' inputs (tests/spectrum_finish_cases.py).
"""
import numpy as np

import spectrum_finish_cases as C
import spectrum_ref as R
from host_engine import HostEngine

OLD = ("ira_spectrum_mag_phase", "ira_phase_unwrap", "ira_spectrum_stats")
# positions in ira_spectrum_finish's argument list (include/ira.h)
A_PACKED, A_MAG, A_UNWRAP, A_DEG, A_P32, A_P64, A_WR, A_FV, A_STATS = 5, 6, 8, 9, 10, 11, 12, 13, 17


def test_argument_validation():
    from audio_analysis_amd import _lib
    lib = _lib.load()
    p = 4096                                                     # a non-NULL value: nothing is dereferenced before the checks

    def call(spec=p, spec_off=p, L=p, nb=0, packed=0, mag=p, out_off=p, p32=0, p64=0, wr=0, fv=p, stats=0):
        return lib.ira_spectrum_finish(spec, spec_off, L, nb, -120.0, packed, mag, out_off, 1, 1, p32, p64, wr, fv, 20.0, 2.0e4,
                                       1000.0, stats, 0)

    assert call() == 0 and call(mag=0, p64=p) == 0 and call(stats=p) == 0          # nb = 0: nothing to do
    for null in ("spec", "spec_off", "L", "out_off"):
        assert call(**{null: 0}) == -1, null
    assert call(mag=0) == -1                                     # no output at all
    assert call(mag=0, p32=p, stats=p) == -1                     # stats without mag_db
    assert call(stats=p, fv=0) == -1                             # stats without the bin steps
    assert call(nb=-1) == -2
    assert b"NULL" in lib.ira_error_string(call(mag=0))


def _channels(eng, lens):
    rng = np.random.default_rng(3)
    return eng.upload([rng.standard_normal(n).astype(np.float32) for n in lens])


def test_spectrum_device_makes_one_fused_call():
    from audio_analysis_amd.analyse.frequency_response import FrequencyResponseAnalysisSettings, spectrum_device
    for want_phase in (False, True):
        eng = HostEngine()
        batch = _channels(eng, (30012, 4801, 8200))
        dev = spectrum_device(eng, batch, 48000, FrequencyResponseAnalysisSettings(trim_to_peak=False), "spectrum",
                              want_phase=want_phase, unwrap=True, degrees=True)
        (name, args), = eng.calls("ira_spectrum_finish")
        assert not any(eng.calls(n) for n in OLD) and not eng.calls("ira_log_smooth_db")
        assert args[3] == 3 and args[4] == -120.0 and args[A_MAG] is not None and args[A_STATS] is not None
        assert (args[A_P32] is not None) == want_phase and args[A_P64] is None and args[A_WR] is None
        assert args[A_UNWRAP] == 1 and args[A_DEG] == 1 and args[14:17] == (20.0, 20000.0, 1000.0)
        assert (args[A_PACKED] is not None) == (dev["packed"] is not None)
        assert set(dev) == {"spec", "spec_packed", "off", "packed", "starts", "lens", "mag", "phase", "stats", "f_lo", "f_hi",
                            "smoothed"}
        assert dev["mag"].dtype == eng.torch.float32 and dev["stats"].dtype == eng.torch.float64
        assert tuple(dev["stats"].shape) == (3, 8) and (dev["phase"] is None) == (not want_phase)
        if want_phase:
            assert dev["phase"].dtype == eng.torch.float32


def test_spectrum_device_with_smoothing_keeps_the_statistics_behind_it():
    from audio_analysis_amd.analyse.frequency_response import FrequencyResponseAnalysisSettings, spectrum_device
    eng = HostEngine()
    batch = _channels(eng, (30012, 4801))
    s = FrequencyResponseAnalysisSettings(trim_to_peak=False, smoothing_log_bins=5)
    dev = spectrum_device(eng, batch, 48000, s, "spectrum", want_phase=True)
    names = [n for n, _ in eng.calls() if n in OLD + ("ira_spectrum_finish", "ira_log_smooth_db")]
    assert names == ["ira_spectrum_finish", "ira_log_smooth_db", "ira_spectrum_stats"], names
    (_, args), = eng.calls("ira_spectrum_finish")
    assert args[A_STATS] is None and args[A_FV] is None and args[A_MAG] is not None and args[A_P32] is not None
    (_, st), = eng.calls("ira_spectrum_stats")
    assert st[0] == args[A_MAG] and dev["smoothed"] is True     # the statistics read the array the smoothing worked on
    assert tuple(dev["stats"].shape) == (2, 8)


def test_group_delay_device_makes_one_fused_call_without_db_and_statistics():
    from audio_analysis_amd.analyse.group_delay import GroupDelayAnalysisSettings, group_delay_device
    eng = HostEngine()
    batch = _channels(eng, (3000, 5000))
    group_delay_device(eng, batch, 48000, GroupDelayAnalysisSettings(trim_to_peak=False))
    (name, args), = eng.calls("ira_spectrum_finish")
    assert name == "ira_spectrum_finish[gd]" and not any(eng.calls(n) for n in OLD)
    assert args[A_MAG] is None and args[A_STATS] is None and args[A_P32] is None and args[A_WR] is None
    assert args[A_P64] is not None and args[A_P64][2] == "torch.float64" and args[A_PACKED] is None
    assert args[A_UNWRAP] == 1 and args[A_DEG] == 0
    (_, gd), = eng.calls("ira_group_delay")
    assert gd[0] == args[A_P64]                                  # the gradient reads the fused call's float64 phase


def test_planted_inputs_are_what_the_gpu_tests_assume():
    nbs = {L // 2 + 1 for L, _ in C.unit_spectra()}
    assert {1, 2, 3, 5, 4095, 4096, 4097, 8192, 8193, 12289} <= nbs
    for L, s in C.unit_spectra():
        assert s.size == L // 2 + 1 and np.allclose(np.abs(s), 1.0, rtol=0, atol=1e-15)
    assert len(C.unit_spectra()) == len(R.UNWRAP_NAMES)
    halves = [L // 2 for L, _, pk, _ in C.packed_batch() if pk]
    assert set(C.PACKED_EDGE_L) <= set(halves)
    assert C.LONG_PACKED_L // 2 + 1 > 512 * 1024 + 1024 and (C.LONG_PACKED_L // 2 + 1) % 4096 != 0
    for L, z, pk, x in C.packed_batch() + [C.long_packed()[:2] + (1, C.long_packed()[2])]:
        if not pk:
            continue
        assert L % 2 == 0 and z.size == L // 2 + 1 and np.isnan(z[-1].real)
        ref = R.mag_db_phase(z, L, -120.0, packed=True)
        # the packed bins ARE the real signal's spectrum, the weights stay inside the bars' range, and no neighbouring pair
        # of angles comes close enough to +-pi for the kernel's error to turn a winding
        want = np.fft.rfft(x)
        got = ref["re"].astype(np.float64) + 1j * ref["im"].astype(np.float64)
        assert np.max(np.abs(got - want)) <= 1e-11 * np.max(np.abs(want))
        assert np.all(ref["weight"] <= R.PACKED_MAX_WEIGHT)
        margin = C.winding_margin(ref)
        assert margin.size == L // 2 and np.all(margin > 1e-6), (L, margin.min())
    for g in R.stats_cases():
        for L, _, m in g["elems"]:
            s = C.stats_spectrum(m)
            with np.errstate(divide="ignore"):
                db = 20.0 * np.log10(np.abs(s.real))
            assert np.array_equal(np.isnan(db), np.isnan(m))
            ok = ~np.isnan(m)
            assert np.array_equal(db[ok].astype(R.F32), m[ok]), (g["name"], L)
            fin = ok & np.isfinite(m) & (m != 0)
            assert np.all(R.tie_margin32(db[fin]) > 1e-9 * np.maximum(np.abs(m[fin]), 1e-30)), (g["name"], L)
