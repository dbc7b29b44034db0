"""
CPU-only tests of the host side of the long transforms: the planner (audio_analysis_amd/engine_plan.py, NumPy only) and
the launches Engine.rfft_any / Engine.band_irfft make of its plans, recorded by the host engine of host_engine.py (no
GPU: the library calls are recorded, not run).
"""
import numpy as np
import pytest
import torch

from audio_analysis_amd import engine_plan as plan
from audio_analysis_amd.engine import Engine, conv_size

from host_engine import HostEngine

# smooth (48000 twice, 6000, 2^15), even non-smooth (30012, 98302), odd (30011 twice, 4099), tiny (1 .. 8)
MIXED = np.array([48000, 48000, 30011, 30011, 30012, 7, 4099, 98302, 6000, 1 << 15, 1, 2, 3, 4, 5, 6, 8], dtype=np.int32)
SIX_ODD = np.array([30011, 4099, 1001, 65537, 98303, 77], dtype=np.int32)      # six convolution sizes, none smooth


def _switches(eng, **over):
    sw = eng._switches()
    for k, v in over.items():
        assert hasattr(sw, k)
        setattr(sw, k, v)
    return sw


def _offsets(lengths):
    return plan.exclusive_cumsum(lengths)


def _written(launches):
    """Spectrum offsets the launches of a plan write, one per element they carry."""
    out = []
    for ln in launches:
        out.append(ln.tables["so"])
        paired = ln.partner >= 0
        if paired.any():
            out.append(ln.tables["so2"][paired])
    return np.concatenate(out)


@pytest.mark.parametrize("over", [{}, {"pair_across_channels": True}, {"half_real_ffts": False},
                                  {"fuse_half_split": False}, {"three_pow2_sizes": False},
                                  {"workspace_budget_bytes": 1 << 20}])
@pytest.mark.parametrize("padded", [False, True])
def test_every_element_of_a_batch_is_written_by_exactly_one_launch(over, padded):
    eng = HostEngine()
    lengths = MIXED
    data_len = np.minimum(lengths, 5000).astype(np.int32) if padded else None
    win_len = (lengths // 2 + 3).astype(np.int32) if padded else None
    spec_off, launches, packed = plan.plan_rfft(_offsets(lengths), lengths, data_len, win_len, False,
                                                _switches(eng, **over), eng.smooth_split)
    assert packed is None
    assert np.array_equal(spec_off, _offsets(lengths.astype(np.int64) // 2 + 1))
    carried = np.concatenate([np.concatenate([ln.jobs, ln.partner[ln.partner >= 0]]) for ln in launches])
    assert np.array_equal(np.sort(carried), np.arange(lengths.size))             # every element, each once
    # the spec_off tables of all launches together are the batch's spec_off, each once
    assert np.array_equal(np.sort(_written(launches)), spec_off)
    for ln in launches:
        assert np.array_equal(ln.tables["so"], spec_off[ln.jobs])
        assert ln.family in (plan.SMOOTH, plan.BLUESTEIN) and ln.count >= 1 and ln.work == ln.count * 2 * ln.size
    families = {ln.family for ln in launches}
    assert families == {plan.SMOOTH, plan.BLUESTEIN}


@pytest.mark.parametrize("three", [True, False])
@pytest.mark.parametrize("across", [False, True])
def test_bluestein_launches_take_the_convolution_size_their_jobs_need(three, across):
    eng = HostEngine()
    sw = _switches(eng, three_pow2_sizes=three, pair_across_channels=across)
    _, launches, _ = plan.plan_rfft(_offsets(MIXED), MIXED, None, None, False, sw, eng.smooth_split)
    blue = [ln for ln in launches if ln.family == plan.BLUESTEIN]
    assert blue
    seen_half = seen_pair = False
    for ln in blue:
        l = ln.lengths.astype(np.int64)
        half = ln.tables["il"].astype(bool) if ln.tables["il"] is not None else np.zeros(ln.count, dtype=bool)
        two = half | (ln.partner >= 0)
        seen_half, seen_pair = seen_half or bool(half.any()), seen_pair or bool((ln.partner >= 0).any())
        # all l outputs of a complex transform: 2 l - 1 lags; the l/2 + 1 bins of one real signal: l + l/2
        need = np.where(two, 2 * l - 1, l + l // 2)
        for v in need:
            assert ln.size == conv_size(int(v), three)
        assert np.array_equal(l, np.where(half, MIXED[ln.jobs] // 2, MIXED[ln.jobs]))
    assert seen_half and seen_pair == across


def test_a_small_workspace_budget_cuts_the_launches():
    eng = HostEngine()
    budget = 3 << 20
    sw = _switches(eng, workspace_budget_bytes=budget)
    lengths = np.repeat(SIX_ODD, 7)
    _, launches, _ = plan.plan_rfft(_offsets(lengths), lengths, None, None, False, sw, eng.smooth_split)
    assert all(ln.family == plan.BLUESTEIN for ln in launches)
    assert any(ln.count > 1 for ln in launches) and any(ln.count == 1 for ln in launches)
    for ln in launches:
        assert ln.count * 32 * ln.size <= budget or ln.count == 1
    lengths = np.repeat(np.int32(48000), 40)
    _, launches, _ = plan.plan_rfft(_offsets(lengths), lengths, None, None, False, sw, eng.smooth_split)
    assert len(launches) > 1 and all(ln.family == plan.SMOOTH and ln.count * 32 * ln.size <= budget for ln in launches)


def _filters_built(eng):
    return sum(args[1] for _, args in eng.calls("ira_bluestein_filter"))


def test_chirp_filters_are_built_once_and_again_after_forget_filters():
    eng = HostEngine()
    x = eng.to_dev(np.zeros(int(SIX_ODD.sum()), dtype=np.float32))
    built = []
    for step in range(3):
        if step == 2:
            eng.forget_filters()
        del eng.record[:]
        eng.rfft_any(x, _offsets(SIX_ODD), SIX_ODD, True)
        assert len(eng.calls("ira_rfft_any")) == 6 and not eng.calls("ira_rfft_smooth")
        built.append(_filters_built(eng))
    assert built == [6, 0, 6]


def _band_call(eng, lengths, bands_per_element=3):
    n = lengths.size
    x = eng.to_dev(np.zeros(int(lengths.sum()), dtype=np.float32))
    spec, so = eng.rfft_any(x, _offsets(lengths), lengths, False)
    ent = np.repeat(np.arange(n), bands_per_element)
    nb = ent.size
    bp = np.zeros((nb, 8))
    bp[:, 0] = 3.0
    bp[:, 1] = 100.0 + 7.0 * np.arange(nb)
    bp[:, 4] = bp[:, 1] + 50.0 * (1 + (np.arange(nb) * 7) % 5)
    lens = lengths[ent]
    y = eng.empty(int(lens.sum()), torch.float32)
    del eng.record[:]
    return eng.band_irfft(spec, so[ent], lens, bp, 48000.0 / lens.astype(np.float64), y, _offsets(lens), want_tiles=True)


def test_paired_bands_of_one_channel_read_the_same_spectrum():
    eng = HostEngine()
    assert not eng.pair_across_channels
    big = MIXED[MIXED >= 8]
    assert _band_call(eng, big) is None                                # tile energies are off
    pairs = 0
    #                                     so, y2, so2 among the arguments of the two entry points
    for name, (i_so, i_y2, i_so2) in (("ira_band_irfft_smooth", (1, 12, 13)), ("ira_band_irfft", (1, 15, 16))):
        calls = eng.calls(name)
        assert calls
        for _, args in calls:
            if name == "ira_band_irfft_smooth":
                assert args[16] is None                               # no partial tile energies asked of the kernel
                if args[14]:                                           # the half-length launch: single bands, no so2
                    assert args[i_so2] is None and np.all(eng.table(args[i_y2])[: args[3]] == -1)
                    continue
            count = args[3]
            so, y2, so2 = (eng.table(args[i])[:count] for i in (i_so, i_y2, i_so2))
            paired = y2 >= 0
            pairs += int(paired.sum())
            assert np.array_equal(so[paired], so2[paired])
    assert pairs == big.size                                           # three bands per element: one pair, one alone
    assert eng.last_band_info_half and len(eng.last_band_info) == len(eng.calls("ira_band_irfft_smooth"))


def test_tile_energies_are_laid_out_only_when_switched_on():
    eng = HostEngine()
    eng.band_tile_energies = True
    lengths = np.array([48000, 30011], dtype=np.int32)
    part, part_off, part_wgs, part_tiles = _band_call(eng, lengths)
    smooth = np.repeat(lengths == 48000, 3)
    assert np.all(part_off[smooth] >= 0) and np.all(part_off[~smooth] == -1)          # Bluestein lengths leave none
    assert np.unique(part_off[smooth]).size == int(smooth.sum())
    assert np.all(part_wgs[smooth] > 0) and np.all(part_tiles[smooth] > 0)
    assert (part_off[smooth] + part_wgs[smooth].astype(np.int64) * part_tiles[smooth]).max() <= part.numel()
    for _, args in eng.calls("ira_band_irfft_smooth"):
        assert args[16] is not None and args[16][:3] == ("empty", int(part.numel()), "torch.float64")


def test_the_same_call_records_the_same_launches():
    records = []
    for _ in range(2):
        eng = HostEngine()
        x = eng.to_dev(np.arange(int(MIXED.sum()), dtype=np.float32))
        spec, so, packed = eng.rfft_any_packed(x, _offsets(MIXED), MIXED, True)
        # the even lengths >= 8 without a direct transform ride half-length Bluestein transforms and stay packed
        assert packed is not None and MIXED[packed.astype(bool)].tolist() == [30012, 98302, 8]
        eng.spectrum_mag_phase(spec, so, MIXED, -120.0, True, packed=packed)
        _band_call_record = list(eng.record)
        _band_call(eng, MIXED[MIXED >= 8])
        records.append(_band_call_record + list(eng.record))
    assert records[0] == records[1] and len(records[0]) > 20


def test_planning_and_pairing_are_reachable_from_engine():
    assert Engine._pair_bands is plan.pair_bands and conv_size is plan.conv_size
    off = plan.exclusive_cumsum(np.array([3, 0, 5], dtype=np.int32))
    assert off.dtype == np.int64 and off.tolist() == [0, 3, 3] and plan.exclusive_cumsum([]).size == 0


def test_event_tag_is_restored_when_a_call_is_refused():
    eng = HostEngine()
    with eng.tagged("[outer]"):
        with pytest.raises(RuntimeError):
            with eng.tagged("[f64,n8192]"):
                assert eng.event_tag == "[f64,n8192]"
                raise RuntimeError("refused")
        assert eng.event_tag == "[outer]"
    assert eng.event_tag == ""


def test_engines_share_no_state():
    a, b = HostEngine(), HostEngine()
    a.group_delay(a.empty(10, torch.float64), np.zeros(1, np.int64), np.array([16]), np.array([3000.0]), 48000.0)
    assert any(k[0] == "gd nonuniform" for k in a._tables) and not b._tables
    assert a._filter_pools is not b._filter_pools
