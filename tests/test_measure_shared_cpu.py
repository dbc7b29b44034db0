"""
CPU-only tests of what the measure modules share: the row tables over several device buffers
(audio_analysis_amd.analyse._common.band_row_offsets) on plain torch CPU tensors, and the channel-batch driver and the
file loader of audio_analysis_amd.analyse._measure on the recording engine.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from audio_analysis_amd.analyse import _measure as M
from audio_analysis_amd.analyse._common import band_row_offsets, common_base

# ------------------------------------------------------------------------------------------------ row tables
LENGTHS = np.array([5, 1, 8], dtype=np.int64)          # ragged channels
NBANDS = 2
START = np.array([2, 0, 7], dtype=np.int64)            # lundeby's start shift, inside every channel


def _buffers(order):
    """x (the channels, with a gap in front of each), y (NBANDS band signals per channel) and bb (one curve per channel) as
    float32 views of ONE arena, laid out by address in `order`: the address order is the test's choice, whatever the
    order the three are created in."""
    x_off = np.array([3, 11, 13], dtype=np.int64)
    sizes = {"x": int(x_off[-1] + LENGTHS[-1]), "y": int(NBANDS * LENGTHS.sum()), "bb": int((LENGTHS - START).sum())}
    arena = torch.zeros(sum(sizes.values()) + 3 * 5, dtype=torch.float32)
    pos, view = 0, {}
    for name in order:
        pos += 5
        view[name] = arena[pos : pos + sizes[name]]
        pos += sizes[name]
    per_entry = np.repeat(LENGTHS, NBANDS)
    y_off = (np.cumsum(per_entry) - per_entry).reshape(LENGTHS.size, NBANDS)
    row_len = LENGTHS - START
    bb_off = np.cumsum(row_len) - row_len
    batch = SimpleNamespace(x=view["x"], off=x_off, length=LENGTHS.copy(), count=int(LENGTHS.size))
    return arena, batch, view["y"], y_off, view["bb"], bb_off


def _address(tensor, offset):
    return int(tensor.data_ptr()) + 4 * int(offset)


@pytest.mark.parametrize("order", [("y", "bb", "x"), ("bb", "x", "y"), ("x", "y", "bb"), ("y", "x", "bb")])
def test_rows_of_two_buffers_address_their_owners(order):
    _, batch, y, y_off, _, _ = _buffers(order)
    bands = ["a", "b"]
    base, seg_off = band_row_offsets(batch, (bands, y, y_off))
    assert seg_off.dtype == np.int64 and seg_off.shape == (3 * (1 + NBANDS),) and np.all(seg_off >= 0)
    assert base is (batch.x if batch.x.data_ptr() < y.data_ptr() else y)
    for c in range(3):
        assert _address(base, seg_off[c * 3]) == _address(batch.x, batch.off[c])
        for b in range(NBANDS):
            assert _address(base, seg_off[c * 3 + 1 + b]) == _address(y, y_off[c, b])
    # a subset of the channels in an order of its own (the left or right channels of stereo pairs)
    pick = np.array([2, 0])
    base2, sub = band_row_offsets(batch, (bands, y, y_off), channels=pick)
    assert base2 is base and np.array_equal(sub, seg_off.reshape(3, 3)[pick].reshape(-1))


@pytest.mark.parametrize("order", [("y", "bb", "x"), ("bb", "x", "y"), ("x", "y", "bb"), ("y", "x", "bb")])
def test_rows_and_curves_of_three_buffers_address_their_owners(order):
    _, batch, y, y_off, bb, bb_off = _buffers(order)
    base, seg_off, edc_off = band_row_offsets(batch, (["a", "b"], y, y_off), curves=(bb, bb_off, START))
    assert base is min((batch.x, y, bb), key=lambda t: t.data_ptr())
    assert seg_off.shape == edc_off.shape == (9,) and np.all(seg_off >= 0) and np.all(edc_off >= 0)
    for c in range(3):
        assert _address(base, seg_off[c * 3]) == _address(batch.x, batch.off[c])
        assert _address(base, edc_off[c * 3]) == _address(bb, bb_off[c])
        for b in range(NBANDS):
            assert _address(base, seg_off[c * 3 + 1 + b]) == _address(y, y_off[c, b])
            # a band row's curve overwrites its band signal from the channel's start index on
            assert _address(base, edc_off[c * 3 + 1 + b]) == _address(y, y_off[c, b] + START[c])
    # no bands: the broadband rows and their curves, still on one base
    base, seg_off, edc_off = band_row_offsets(batch, None, curves=(bb, bb_off, START))
    assert base is min((batch.x, bb), key=lambda t: t.data_ptr()) and np.all(seg_off >= 0) and np.all(edc_off >= 0)
    for c in range(3):
        assert _address(base, seg_off[c]) == _address(batch.x, batch.off[c])
        assert _address(base, edc_off[c]) == _address(bb, bb_off[c])


def test_rows_without_bands_are_the_batch_itself():
    _, batch, y, _, _, _ = _buffers(("y", "bb", "x"))
    for sig in (None, ([], None, np.zeros((3, 0), dtype=np.int64))):
        base, seg_off = band_row_offsets(batch, sig)
        assert base is batch.x and np.array_equal(seg_off, batch.off) and seg_off is not batch.off
        seg_off[0] += 1                                            # a copy: the batch's own table is not touched
        assert batch.off[0] == 3
    base, seg_off = band_row_offsets(batch, None, channels=[1, 1, 0])
    assert base is batch.x and np.array_equal(seg_off, batch.off[[1, 1, 0]])


def test_buffers_two_bytes_apart_are_refused():
    raw = np.zeros(64, dtype=np.int16)
    x = torch.from_numpy(raw[0:16].view(np.float32))
    y = torch.from_numpy(raw[17:49].view(np.float32))              # 2 bytes off the float32 grid of x
    assert (y.data_ptr() - x.data_ptr()) % 4 == 2
    batch = SimpleNamespace(x=x, off=np.array([0, 4], dtype=np.int64), length=np.array([4, 4], dtype=np.int64), count=2)
    y_off = np.array([[0, 4], [8, 12]], dtype=np.int64)
    with pytest.raises(ValueError, match="4-byte aligned to each other"):
        band_row_offsets(batch, (["a", "b"], y, y_off))
    with pytest.raises(ValueError, match="4-byte aligned to each other"):
        common_base([x, y])


# ------------------------------------------------------------------------------------------------ drivers
def test_channel_batches_upload_chunks_of_max_batch_channels():
    from host_engine import HostEngine
    eng = HostEngine()
    n = 2 * M.MAX_BATCH_CHANNELS + 3
    channels = [np.full(16, i, dtype=np.float64) for i in range(n)]          # converted to float32 on the way
    names = [f"c{i}" for i in range(n)]
    seen = []

    def results_of_batch(e, batch, sample_rate_hz, chunk_names, settings):
        assert e is eng and sample_rate_hz == 44100 and settings == "settings"
        assert batch.x.dtype == torch.float32 and np.all(batch.length == 16)
        seen.append((batch.count, list(chunk_names), batch.x.numpy()[:: 16].copy()))
        return [f"r:{nm}" for nm in chunk_names]

    uploads = eng.uploads
    out = M.analyse_channel_batches(channels, 44100, names, "settings", results_of_batch, eng=eng)
    assert [c for c, _, _ in seen] == [256, 256, 3]
    assert eng.uploads - uploads == 3 * 2                          # per chunk: the samples, and the offset / length tables
    assert [nm for _, chunk, _ in seen for nm in chunk] == names and out == [f"r:{nm}" for nm in names]
    assert np.array_equal(np.concatenate([first for _, _, first in seen]), np.arange(n, dtype=np.float32))
    with pytest.raises(ValueError, match="one name per channel"):
        M.analyse_channel_batches(channels, 44100, names[:-1], "settings", results_of_batch, eng=eng)
    assert len(seen) == 3                                          # refused before anything was uploaded


def test_file_channels_names_every_channel_by_its_file(tmp_path):
    from audio_analysis_amd.analyse.deconvolve import _write_wav_float32
    left = np.array([0.5, -0.25, 0.125, 0.0], dtype=np.float32)
    right = np.array([0.25, 0.75, -0.5, 1.0], dtype=np.float32)
    _write_wav_float32(tmp_path / "one.wav", 48000, left.reshape(-1, 1))
    _write_wav_float32(tmp_path / "sub" / "two.wav", 48000, np.stack([left, right], axis=1))
    paths = [tmp_path / "one.wav", str(tmp_path / "sub" / "two.wav")]
    got = list(M.file_channels(paths, False))
    assert [n for n, _ in got] == ["one.wav:mono", "two.wav:left", "two.wav:right"]
    for (_, c), want in zip(got, (left, left, right)):
        assert c.dtype == np.float32 and np.array_equal(c, want)
    got = list(M.file_channels(paths, True, expected_sample_rate_hz=48000))
    assert [n for n, _ in got] == ["one.wav:mono", "two.wav:mono"]
    assert np.array_equal(got[0][1], left) and np.array_equal(got[1][1], 0.5 * (left + right))
    with pytest.raises(ValueError, match="Expected sample rate 44100 Hz"):
        list(M.file_channels(paths, False, expected_sample_rate_hz=44100))
