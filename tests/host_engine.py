"""
A recording engine for CPU-only tests: an Engine whose device plumbing is replaced, so that the host side of every
product call (planning, job tables, allocation sizes, the order and arguments of the library calls) runs and can be
inspected without a GPU.  Helper module, like decay_ref.py / stft_bounds.py: it holds no tests.

Tensors live in host memory, `empty` gives zeros, uploads are copies, and every ira_* launch is recorded and answered
with 0 instead of being run (the host-only entry points -- the FFT splits, the tile layout, the *_doubles sizes -- pass
through to the library).  Nothing is computed: results that come back from "the device" are zeros.

`record` is the list of what happened, in order:
    ("call", name + event tag, (argument, ...))    one per library call
    ("fetch", pointee, shape)                      one per Engine.fetch
An argument is a scalar (converted as its C type converts it), a tuple of doubles (the ranges / crossings arrays), None
for a NULL pointer, or what a pointer points AT: ("up", dtype, shape, digest, byte offset) for an uploaded host array
(tables included) and ("empty", elements, dtype, byte offset) for an allocation.  Addresses never enter the record, so
two runs, or two versions of engine.py, can be compared with ==.
"""
import ctypes
import hashlib

import numpy as np
import torch

from audio_analysis_amd import _lib
from audio_analysis_amd.engine import ChannelBatch, Engine, HostFuture

HOST_ONLY = {"ira_abi_version", "ira_error_string", "ira_fft_split", "ira_fft_smooth_split", "ira_band_tile_layout",
             "ira_ar_partial_doubles", "ira_ar_exact_doubles", "ira_energy_scratch_doubles", "ira_xcorr_scratch_doubles",
             "ira_lundeby_scratch_doubles", "ira_mtf_scratch_doubles", "ira_echo_scratch_doubles", "ira_fdw_scratch_doubles",
             "ira_burst_table_doubles"}


class _RecordingLib:
    def __init__(self, eng):
        self._lib, self._eng = _lib.load(), eng

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name in HOST_ONLY or not name.startswith("ira_"):
            return fn
        argtypes = _lib.PROTOTYPES[name][1]

        def recorded(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            self._eng._record_call(name, argtypes, args)
            return 0

        return recorded


class HostEngine(Engine):
    def __init__(self):
        self.record = []
        self.uploads = 0             # host -> device copies a real engine would have enqueued
        self._live = []              # (first byte, last byte + 1, description, tensor): everything stays alive, so that
        #                              an address names one allocation for the whole life of the engine
        self._init_state(torch, torch.device("cpu"), _RecordingLib(self))
        self.num_lanes = 1

    # ---------------------------------------------------------------- the record
    def _remember(self, tensor, desc):
        nbytes = int(tensor.numel()) * tensor.element_size()
        if nbytes:
            self._live.append((int(tensor.data_ptr()), int(tensor.data_ptr()) + nbytes, desc, tensor))
        return tensor

    def _pointee(self, address):
        if not address:
            return None
        for first, end, desc, _ in reversed(self._live):
            if first <= address < end:
                return desc + (address - first,)
        raise AssertionError(f"pointer {address:#x} points at nothing this engine allocated or uploaded")

    def _record_call(self, name, argtypes, args):
        out = []
        for ty, a in zip(argtypes, args):
            if ty is ctypes.c_void_p:
                out.append(self._pointee(a))
            elif isinstance(a, ctypes.Array):
                out.append(tuple(a))
            else:
                out.append(ty(a).value)
        self.record.append(("call", name + self.event_tag, tuple(out)))

    def calls(self, name=None):
        """The recorded library calls as (name, arguments), optionally those of one entry point."""
        return [(e[1], e[2]) for e in self.record if e[0] == "call" and (name is None or e[1].split("[")[0] == name)]

    def table(self, pointee):
        """The host array an ("up", ...) argument stands for (from its byte offset on, flat)."""
        assert pointee[0] == "up", pointee
        for _, _, desc, tensor in self._live:
            if desc == pointee[:-1]:
                flat = tensor.numpy().reshape(-1)
                return flat[pointee[-1] // flat.itemsize:]
        raise KeyError(pointee)

    # ---------------------------------------------------------------- device plumbing, replaced
    @property
    def stream(self) -> int:
        return 0

    def sync(self) -> None:
        pass

    def _host_copy(self, a):
        a = np.ascontiguousarray(a)
        desc = ("up", a.dtype.str, tuple(a.shape), hashlib.sha1(a.tobytes()).hexdigest()[:16])
        return self._remember(torch.from_numpy(a.copy()), desc)

    def to_dev(self, a):
        self.uploads += 1
        return self._host_copy(a)

    def job_tables(self, *arrays):
        self.uploads += 1
        return [None if a is None else self._host_copy(a) for a in arrays]

    def empty(self, n, dtype):
        n = int(max(n, 1))
        return self._remember(torch.zeros(n, dtype=dtype), ("empty", n, str(dtype)))

    def fetch(self, tensor) -> HostFuture:
        tensor = tensor.contiguous()
        self.record.append(("fetch", self._pointee(int(tensor.data_ptr())), tuple(tensor.shape)))
        return HostFuture(tensor.clone(), tuple(tensor.shape))

    def wrap(self, x_dev, off, lens) -> ChannelBatch:
        off = np.ascontiguousarray(off, dtype=np.int64)
        lens = np.ascontiguousarray(lens, dtype=np.int64)
        d_off, d_len = self.job_tables(off, lens)
        return ChannelBatch(x=x_dev, off=off, length=lens, off_dev=d_off, len_dev=d_len)

    def peaks_begin(self, b) -> None:
        pass

    def peaks(self, b) -> np.ndarray:
        if b.peak is None:
            x = b.x.numpy()
            mag = [np.abs(x[o : o + n]) for o, n in zip(b.off, b.length)]
            b.peak = np.array([int(np.argmax(m)) if m.size else 0 for m in mag], dtype=np.int64)
            b.peak_abs = np.array([m[p] if m.size else 0.0 for m, p in zip(mag, b.peak)], dtype=np.float32)
        return b.peak
