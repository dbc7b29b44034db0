"""Guarded flat buffers for GPU tests that call the C-ABI on memory they own (test_gpu_modal_kernels.py,
test_gpu_deconv_kernels.py, test_gpu_minphase_kernels.py): the segments of a launch lie in one 0xDEADBEEF-filled buffer, GUARD elements in front of
the first and behind the last, gaps of 1 to 7 elements between them, so offsets take every residue and a write outside
a segment is seen when the buffer comes back."""
import numpy as np

SENT32, SENT64 = 0xDEADBEEF, 0xDEADBEEFDEADBEEF
GUARD = 16


def sentinel(n, dtype):
    dtype = np.dtype(dtype)
    if dtype.itemsize == 4:
        return np.full(n, SENT32, np.uint32).view(dtype)
    return np.full(n * dtype.itemsize // 8, SENT64, np.uint64).view(dtype)


def words(a):
    """The bits of a: uint32 words for 4-byte elements, uint64 words otherwise (two per complex128)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint64)


def untouched(a):
    """True where every word of the buffer still holds the sentinel."""
    return bool(np.all(words(a) == (SENT32 if np.asarray(a).dtype.itemsize == 4 else SENT64)))


class Flat:
    def __init__(self, lens, dtype=np.float32, phase=0):
        self.lens, self.dtype = [int(n) for n in lens], np.dtype(dtype)
        self.off, pos = [], GUARD
        for k, n in enumerate(self.lens):
            self.off.append(pos)
            pos += n + 1 + (k + phase) % 7
        self.total = pos + GUARD

    def filled(self, segs=None):
        buf = sentinel(self.total, self.dtype)
        for o, s in zip(self.off, segs or []):
            buf[o:o + len(s)] = s
        return buf

    def split(self, buf, what):
        """The segments of a buffer that came back; every guard and gap must still hold the sentinel."""
        buf = np.ascontiguousarray(buf).view(self.dtype)
        gaps = np.ones(self.total, bool)
        for o, n in zip(self.off, self.lens):
            gaps[o:o + n] = False
        sent = words(sentinel(1, self.dtype))[0]
        bad = gaps & ~np.all(words(buf).reshape(self.total, -1) == sent, axis=1)
        assert not bad.any(), f"{what}: {int(bad.sum())} elements written outside the segments, first at {int(np.argmax(bad))}"
        return [buf[o:o + n].copy() for o, n in zip(self.off, self.lens)]


def to_device(eng, arr):
    """A device copy of arr; complex128 goes as its float64 pairs, uint32 as int32."""
    import torch
    arr = np.array(arr, order="C")                    # a copy: the case tables are read-only
    if arr.dtype == np.complex128:
        arr = arr.view(np.float64)
    elif arr.dtype == np.uint32:
        arr = arr.view(np.int32)
    return torch.from_numpy(arr).to(eng.device)
