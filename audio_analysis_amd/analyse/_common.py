"""Host-side helpers shared by the drop-in modules: time selection, batching, WAV channel loading, and the row tables of a
launch that reads several device buffers."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from ..engine import ChannelBatch, Engine, get_engine
from .io import get_analysis_channels, load_wav_file


def segment_bounds(n: int, peak: int, sample_rate_hz: int, trim_to_peak: bool, ignore_leading_seconds: float,
                   duration_seconds: Optional[float]) -> Tuple[int, int]:
    """
    (start, length) of the analysed slice: drop [0, peak) when trimming, skip round(ignore*sr) samples
    (clamped), optionally keep round(duration*sr) samples (clamped).  Integer arithmetic, bit-exact with
    the prologue every reference module repeats (e.g. decay.py:135-144, spectrogram.py:180-194).
    """
    start, length = (peak, n - peak) if trim_to_peak else (0, n)
    if ignore_leading_seconds > 0.0:
        skip = int(round(float(ignore_leading_seconds) * float(sample_rate_hz)))
        skip = max(0, min(skip, length))
        start, length = start + skip, length - skip
    if duration_seconds is not None:
        keep = int(round(float(duration_seconds) * float(sample_rate_hz)))
        length = max(0, min(keep, length))
    return start, length


def segment_bounds_batch(n: np.ndarray, peak: np.ndarray, sample_rate_hz: int, trim_to_peak: bool,
                         ignore_leading_seconds: float, duration_seconds: Optional[float]) -> Tuple[np.ndarray, np.ndarray]:
    """segment_bounds for arrays of lengths and peak indices (int64 in, int64 out): the same integer arithmetic, without a
    Python call per channel (the metrics pipeline asks for 256 channels per step, several times)."""
    n = np.asarray(n, dtype=np.int64)
    peak = np.asarray(peak, dtype=np.int64)
    start = peak.copy() if trim_to_peak else np.zeros_like(n)
    length = n - peak if trim_to_peak else n.copy()
    if ignore_leading_seconds > 0.0:
        skip = int(round(float(ignore_leading_seconds) * float(sample_rate_hz)))
        sk = np.maximum(0, np.minimum(skip, length))
        start, length = start + sk, length - sk
    if duration_seconds is not None:
        keep = int(round(float(duration_seconds) * float(sample_rate_hz)))
        length = np.maximum(0, np.minimum(keep, length))
    return start, length


def as_batch(channels: Sequence[np.ndarray]) -> Tuple[Engine, ChannelBatch]:
    eng = get_engine()
    return eng, eng.upload(list(channels))


def wav_channels(path, use_mono_downmix_for_stereo: bool, **load_kw):
    loaded = load_wav_file(wav_file_path=path, expected_channel_mode="mono_or_stereo",
                           allow_mono_and_upmix_to_stereo=False, **load_kw)
    return loaded, get_analysis_channels(loaded_audio=loaded, use_mono_downmix_for_stereo=use_mono_downmix_for_stereo)


def frame_time_axis(num_frames: int, hop_length: int, sample_rate_hz: int) -> np.ndarray:
    """Frame-start times in float32 arithmetic (reference spectrogram.py:158)."""
    return (np.arange(num_frames, dtype=np.float32) * float(hop_length) / float(sample_rate_hz)).astype(np.float32)


def common_base(tensors):
    """One base pointer for float32 device buffers that one launch reads: the lowest of them, and every buffer's offset
    from it in elements (the kernels address segments as base + offset in the device's flat address space)."""
    ptrs = [int(x.data_ptr()) for x in tensors]
    lo = int(np.argmin(ptrs))
    if any((p - ptrs[lo]) % 4 for p in ptrs):
        raise ValueError("float32 buffers of one launch must be 4-byte aligned to each other")
    return tensors[lo], [(p - ptrs[lo]) // 4 for p in ptrs]


def band_row_offsets(batch, band_signals=None, channels=None, curves=None):
    """
    (base, seg_off) of the rows "channel c's broadband signal in batch.x, then its bands in y" (row c * (1 + nbands) + b),
    int64 element offsets from ONE base pointer.  band_signals = (bands, y device, y_off (nch, nbands)) as
    rt60bands.band_signals_device returns them; None or an empty bank: broadband rows only, and (batch.x, a copy of
    batch.off).  channels: the channel indices whose rows are wanted, in that order (default: every channel).
    curves = (buffer, offsets (nch,), start (nch,)): a third float32 buffer with one output curve per channel, for a
    launch that writes a curve per row; the result is then (base, seg_off, curve_off), where a broadband row's curve
    lies at its offset in that buffer and a band row's curve over its own band signal from start[c] on.

    The buffers are separate allocations, so the offsets are differences between unrelated addresses (common_base): the
    tables of a banded launch depend on where the allocator put y relative to batch.x, and two runs of the same call may
    upload different tables that address the same elements.  Every launch that reads several buffers gets its tables here.
    """
    ch = slice(None) if channels is None else np.asarray(channels, dtype=np.int64)
    bands, y, y_off = band_signals if band_signals is not None else ((), None, None)
    nb = len(bands)
    owners = [batch.x] + ([y] if nb else []) + ([curves[0]] if curves is not None else [])
    if len(owners) == 1:
        return batch.x, batch.off[ch].copy()
    base, delta = common_base(owners)
    seg_off = batch.off[ch] + delta[0]
    if nb:
        y_off = np.asarray(y_off, dtype=np.int64).reshape(batch.count, nb)[ch] + delta[1]
        seg_off = np.concatenate([seg_off[:, None], y_off], axis=1).reshape(-1)
    if curves is None:
        return base, seg_off
    curve_off = np.asarray(curves[1], dtype=np.int64)[ch] + delta[-1]
    if nb:
        start = np.asarray(curves[2], dtype=np.int64)[ch]
        curve_off = np.concatenate([curve_off[:, None], y_off + start[:, None]], axis=1).reshape(-1)
    return base, seg_off, curve_off
