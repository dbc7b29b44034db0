"""ira_tail_energy (float64 suffix energies in blocks of 512 samples) and the STFT calls that take its table:
ira_stft_mag_db_tf_tail (float32 / n_fft 4096: stft6_kernel; float64 / 8192: stft5_kernel behind stft5_consts_kernel) and
ira_stft_logbin_tail (float64 / 8192: stft5_kernel).

The calls WITHOUT the table are held to the float64 NumPy oracle and to the every-shortcut-off path by
test_gpu_stft_dispatch, test_gpu_stft5_chunks, test_gpu_stft5_quiet and test_gpu_stft_quiet_chunks.  What is checked here is
BYTE EQUALITY of the whole output buffer between a call with the table and the same call without it, for both kernels
(stft5 in both output modes), hop 300 and 512, on segments of n_fft + 40 hop samples (41 frames: for stft5 five chunks of
eight and one of one) that start at odd offsets which are no multiple of 512, the last one ending where the sample buffer
ends:

  zeros      a loud head, then an all-zero tail
  decay      a noise burst that decays through the threshold in mid-segment
  gap        a loud head, a long silence, then a loud burst: the suffix must not certify the silence
  nonfinite  a quiet tail with a NaN and an infinity in the last frame
  pair       one tail at two scales: 4 N max(w^2) S[j] a part in a thousand under and over floor^2 at the first block of
             the fourth chunk (the inputs are checked to be that, with the table the GPU made)
  window     the pair with the window table scaled by 2 (certifies less, never more: bytes equal); and a constant tail
             under a rectangular window scaled by 2.5, where a rule that took max(w^2) as 1 would floor bin 0 although it
             lies 1.5 dB above the floor
  selection  dB mode with a frame selection: the table is ignored (shown with a table of zeros, which would floor all)
That the table is consulted at all is shown the other way round: a table of zeros floors every frame of a loud batch.

ira_tail_energy alone: S[j] (1 + 1e-9) >= the exact sum (math.fsum of exact squares) and |S[j] - exact| <= 1e-12 exact
for every j of segments of 0, 1, 511, 512, 513, 5000 and 300 000 samples (586 blocks: ten runs of the scan); the same
bits from a second run; a NaN or an infinity poisons exactly the entries at or before its block and changes no other bit.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 512
KERNELS = {"stft5": (8192, 64), "stft6": (4096, 32)}       # name -> (n_fft, precision)
MODES = [("stft5", "db"), ("stft5", "lb"), ("stft6", "db")]
FLOOR_DB = -120.0
SENTINEL = 0x7FC12345          # a NaN payload no kernel produces: an output value nobody stored


@pytest.fixture(scope="module")
def eng():
    from audio_analysis_amd.engine import get_engine
    return get_engine()


# ---------------------------------------------------------------------------------------------------------- inputs
class Batch:
    """Segments of n_fft + 40 hop samples at odd offsets; the last one ends where the buffer ends."""

    def __init__(self, segments, hop, n_fft):
        self.hop, self.n_fft = hop, n_fft
        self.seg_len = n_fft + 40 * hop
        assert all(s.size == self.seg_len and s.dtype == np.float32 for s in segments)
        off, pos = [], 1237
        for _ in segments:
            off.append(pos)
            pos += self.seg_len + 334
        self.off = np.array(off, dtype=np.int64)
        assert np.all(self.off % 2 == 1) and np.all(self.off % B != 0)
        self.x = np.zeros(int(self.off[-1]) + self.seg_len, dtype=np.float32)
        self.x[: int(self.off[0])] = 0.75                     # loud samples in front of and between the segments
        for o, s in zip(self.off, segments):
            self.x[o : o + self.seg_len] = s
            self.x[o + self.seg_len : o + self.seg_len + 334] = 0.75
        self.x = self.x[: int(self.off[-1]) + self.seg_len]
        self.cols = np.full(len(segments), 41, dtype=np.int32)
        self.end = self.off + self.seg_len


def _segments(hop, n_fft):
    rng = np.random.default_rng(20 + hop)
    n = n_fft + 40 * hop
    head = np.zeros(n)
    head[:3000] = 0.5 * rng.standard_normal(3000)
    zeros = head.copy()
    decay = 1e-3 * rng.standard_normal(n) * np.exp(-np.arange(n) / 600.0)
    gap = head.copy()
    gap[int(0.7 * n) : int(0.75 * n)] = 0.25 * rng.standard_normal(int(0.75 * n) - int(0.7 * n))
    bad = decay.copy()
    bad[n - 100] = np.nan
    bad[n - 50] = np.inf
    return [s.astype(np.float32) for s in (zeros, decay, gap, bad)]


def _floor_pow():
    return (10.0 ** (FLOOR_DB / 20.0)) ** 2


def _pair_segments(hop, n_fft, wmax2):
    """One tail at two scales: 4 N wmax2 (exact suffix energy from the first block of frame 24 on) = floor^2 (1 -+ 1e-3)."""
    rng = np.random.default_rng(7 + hop)
    n = n_fft + 40 * hop
    unit = rng.standard_normal(n) * np.exp(-np.arange(n) / 4000.0)
    j = (24 * hop) // B
    out = []
    for rel in (1.0 - 1e-3, 1.0 + 1e-3):
        e_unit = math.fsum((unit[j * B :] ** 2).tolist())
        seg = (unit * math.sqrt(rel * _floor_pow() / (4.0 * n_fft * wmax2 * e_unit))).astype(np.float32)
        seg[:2000] = (0.1 * rng.standard_normal(2000)).astype(np.float32)
        out.append(seg)
    return out, j


# ---------------------------------------------------------------------------------------------------------- launches
def _logbins():
    from audio_analysis_amd.analyse.modalcloud import _build_log_bins, log_bin_rows
    freq = np.fft.rfftfreq(8192, d=1.0 / 48000.0).astype(np.float32)
    rows = np.nonzero((freq >= 20.0) & (freq <= 20000.0))[0]
    _, first, count = log_bin_rows(freq[rows], _build_log_bins(20.0, 20000.0, 24, 24))
    return int(rows[0]), first.astype(np.int32), count.astype(np.int32)


def _dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _run(eng, b, mode, table=None, window=None, sel=None, use_hann=True):
    """One launch through the C-ABI -> the whole output buffer as uint32.  mode "db": ira_stft_mag_db_tf(_tail), "lb":
    ira_stft_logbin(_tail); the kernel follows from the batch's n_fft.  table: (tab device float64, tab_off host int64) or
    None.  sel: per-segment frame indices."""
    import torch
    from audio_analysis_amd._lib import check
    N_FFT = b.n_fft
    prec = 64 if N_FFT == 8192 else 32
    x = _dev(eng, b.x)
    n = b.off.size
    window = eng.window(N_FFT, use_hann, prec) if window is None else window
    cols = b.cols if sel is None else np.array([s.size for s in sel], dtype=np.int32)
    k_base, first, count = _logbins()
    per = (N_FFT // 2 + 1) if mode == "db" else first.size
    out_off = np.concatenate([[0], np.cumsum(cols.astype(np.int64) * per)])[:-1]
    total = int(np.sum(cols.astype(np.int64) * per))
    out = _dev(eng, np.full(total, SENTINEL, dtype=np.int32)).view(torch.float32)
    d_off, d_cols, d_ooff = _dev(eng, b.off), _dev(eng, cols), _dev(eng, out_off)
    extra = ()
    keep = []
    if table is not None:
        tab, tab_off = table
        d_toff = _dev(eng, tab_off)
        consts = torch.zeros(1 + (first.size + 1) // 2, dtype=torch.float64, device=eng.device)
        keep = [d_toff, consts]
        extra = (tab.data_ptr(), d_toff.data_ptr(), consts.data_ptr())
    head = (x.data_ptr(), d_off.data_ptr(), d_cols.data_ptr(), n, int(cols.max()), N_FFT, b.hop, window.data_ptr(),
            eng.twiddle(N_FFT, prec).data_ptr(), prec, FLOOR_DB)
    if mode == "db":
        d_sel = d_soff = None
        if sel is not None:
            d_sel = _dev(eng, np.concatenate(sel).astype(np.int32))
            d_soff = _dev(eng, np.concatenate([[0], np.cumsum(cols.astype(np.int64))])[:-1])
        fn = eng.lib.ira_stft_mag_db_tf_tail if table is not None else eng.lib.ira_stft_mag_db_tf
        check(fn(*head, out.data_ptr(), d_ooff.data_ptr(), d_sel.data_ptr() if sel is not None else 0,
                 d_soff.data_ptr() if sel is not None else 0, *extra, eng.stream), "ira_stft_mag_db_tf")
    else:
        d_first, d_count = _dev(eng, first), _dev(eng, count)
        fn = eng.lib.ira_stft_logbin_tail if table is not None else eng.lib.ira_stft_logbin
        check(fn(*head, k_base, d_first.data_ptr(), d_count.data_ptr(), first.size, out.data_ptr(), d_ooff.data_ptr(),
                 *extra, eng.stream), "ira_stft_logbin")
    eng.sync()
    del keep
    return out.view(torch.int32).cpu().numpy().view(np.uint32)


def _table(eng, b):
    t = eng.tail_energy(_dev(eng, b.x), b.off, b.end)
    eng.sync()
    return t


def _same_bytes(eng, b, mode, **kw):
    t = _table(eng, b)
    plain = _run(eng, b, mode, **kw)
    with_table = _run(eng, b, mode, table=(t["tab"], t["off"]), **kw)
    assert not np.any(plain == SENTINEL), "the call without the table left output values unwritten"
    assert plain.size == with_table.size and np.array_equal(plain, with_table), \
        f"{int(np.sum(plain != with_table))} of {plain.size} values differ with the table"
    return plain.view(np.float32), t


# ---------------------------------------------------------------------------------------------------------- the STFT calls
def _wmax2(eng, kernel, use_hann=True):
    n_fft, prec = KERNELS[kernel]
    w = eng.window(n_fft, use_hann, prec).double()
    return float((w * w).max().item())


@pytest.mark.parametrize("kernel,mode", MODES)
@pytest.mark.parametrize("hop", [300, 512])
def test_zeros_decay_gap_nonfinite(eng, hop, kernel, mode):
    N_FFT = KERNELS[kernel][0]
    b = Batch(_segments(hop, N_FFT), hop, N_FFT)
    out, t = _same_bytes(eng, b, mode)
    tab = t["tab"].cpu().numpy()
    s = [tab[int(o) : int(o) + int(nb) + 1] for o, nb in zip(t["off"], t["nblk"])]
    lim = _floor_pow() / (4.0 * N_FFT)                       # max(w^2) <= 1 (Hann): entries at or under it certify
    assert s[0][6] == 0.0 and s[0][0] > lim                   # zeros: everything behind the head certifies
    assert s[1][0] > lim and s[1][-2] <= lim and np.sum(s[1] <= lim) > 8      # decay: crosses in mid-segment
    first_block_of_burst = int(0.7 * b.seg_len) // B
    assert np.all(s[2][: first_block_of_burst + 1] > lim)     # gap: the silence in front of the burst does not certify
    assert not np.any(np.isfinite(s[3][:-1])) and s[3][-1] == 0.0             # nonfinite: nothing certifies
    if mode == "db":
        m = out.reshape(4, 41, N_FFT // 2 + 1)
        fl = np.float32(FLOOR_DB)
        # frames 11 .. 19 start behind the head (3000 samples) and end in front of the burst at either hop
        assert np.all(m[0, 11:] == fl) and m[0, 0].max() > -60.0
        assert np.all(m[2, 11:20] == fl) and m[2, 30:].max() > -60.0
        assert np.all(np.isnan(m[3, 40])) and not np.any(np.isnan(m[3, :40]))


@pytest.mark.parametrize("kernel,mode", MODES)
@pytest.mark.parametrize("hop", [300, 512])
def test_threshold_pair(eng, hop, kernel, mode):
    N_FFT = KERNELS[kernel][0]
    wmax2 = _wmax2(eng, kernel)
    segs, j = _pair_segments(hop, N_FFT, wmax2)
    b = Batch(segs, hop, N_FFT)
    _, t = _same_bytes(eng, b, mode)
    tab = t["tab"].cpu().numpy()
    under, over = (float(tab[int(o) + j]) * (4.0 * N_FFT) * wmax2 for o in t["off"])
    assert under <= _floor_pow() < over, (under, _floor_pow(), over)
    assert under > 0.998 * _floor_pow() and over < 1.002 * _floor_pow()


@pytest.mark.parametrize("kernel,mode", MODES)
def test_scaled_window(eng, kernel, mode):
    N_FFT, prec = KERNELS[kernel]
    w = eng.window(N_FFT, True, prec)
    segs, _ = _pair_segments(512, N_FFT, _wmax2(eng, kernel))
    _same_bytes(eng, Batch(segs + _segments(512, N_FFT)[:2], 512, N_FFT), mode, window=w * 2.0)
    # a constant tail whose last frame IS the suffix of its block: 4 N S = 0.9 floor^2, |X[0]|^2 = 2.5^2 N S = 1.41 floor^2
    n = N_FFT + 40 * 512
    a = math.sqrt(0.9 * _floor_pow() / (4.0 * N_FFT * N_FFT))
    seg = np.full(n, a, dtype=np.float32)
    seg[:2000] = 0.1
    b = Batch([seg, seg], 512, N_FFT)
    out, t = _same_bytes(eng, b, mode, window=eng.window(N_FFT, False, prec) * 2.5, use_hann=False)
    s_last = float(t["tab"].cpu().numpy()[int(t["off"][0]) + 40])
    assert 0.89 * _floor_pow() < 4.0 * N_FFT * s_last < 0.91 * _floor_pow()
    if mode == "db":
        m = out.reshape(2, 41, N_FFT // 2 + 1)
        assert np.all(m[:, 40, 0] > FLOOR_DB + 1.0) and np.all(m[:, 40, 1:] == np.float32(FLOOR_DB))


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_a_table_of_zeros_floors_everything_and_a_selection_ignores_it(eng, kernel):
    import torch
    N_FFT = KERNELS[kernel][0]
    b = Batch(_segments(512, N_FFT)[:3], 512, N_FFT)         # the finite segments
    t = _table(eng, b)
    zeros = (torch.zeros_like(t["tab"]), t["off"])
    plain = _run(eng, b, "db").view(np.float32)
    assert plain.max() > -60.0
    floored = _run(eng, b, "db", table=zeros).view(np.float32)
    assert np.all(floored == np.float32(FLOOR_DB)), "the table is not consulted"
    sel = [np.array([40, 3, 3, 0, 17, 16, 15, 14, 13, 12, 39], dtype=np.int64) for _ in range(3)]
    with_sel = _run(eng, b, "db", sel=sel)
    assert np.array_equal(with_sel, _run(eng, b, "db", sel=sel, table=zeros))
    assert np.array_equal(with_sel, _run(eng, b, "db", sel=sel, table=(t["tab"], t["off"])))
    m = with_sel.view(np.float32).reshape(3, 11, N_FFT // 2 + 1)
    assert np.array_equal(m[0, 1].view(np.uint32), plain.reshape(3, 41, -1)[0, 3].view(np.uint32))


def test_engine_plumbing_shares_one_table(eng):
    """Engine.stft_logbin / stft_mag_db with tail=Engine.tail_table(batch, starts): same bytes, one table per batch and
    start vector, and a table made for other starts is refused."""
    N_FFT = 8192
    segs = _segments(512, N_FFT)
    batch = eng.upload([np.concatenate([np.full(777, 0.3, dtype=np.float32), s]) for s in segs])
    starts = np.full(4, 777, dtype=np.int64)
    cols = np.full(4, 41, dtype=np.int32)
    k_base, first, count = _logbins()
    tail = eng.tail_table(batch, starts)
    assert eng.tail_table(batch, starts) is tail
    assert eng.tail_table(batch, starts + 1) is not tail
    tail = eng.tail_table(batch, starts)
    a, _ = eng.stft_logbin(batch.x, batch.off + starts, cols, N_FFT, 512, True, FLOOR_DB, k_base, first, count)
    c, _ = eng.stft_logbin(batch.x, batch.off + starts, cols, N_FFT, 512, True, FLOOR_DB, k_base, first, count, tail=tail)
    d, _, _ = eng.stft_mag_db(batch.x, batch.off + starts, cols, N_FFT, 512, True, FLOOR_DB, 64, frame_major=True)
    e, _, _ = eng.stft_mag_db(batch.x, batch.off + starts, cols, N_FFT, 512, True, FLOOR_DB, 64, frame_major=True, tail=tail)
    cols32 = np.full(4, 49, dtype=np.int32)                  # the same segments in frames of 4096
    f, _, _ = eng.stft_mag_db(batch.x, batch.off + starts, cols32, 4096, 512, True, FLOOR_DB, 32, frame_major=True)
    g, _, _ = eng.stft_mag_db(batch.x, batch.off + starts, cols32, 4096, 512, True, FLOOR_DB, 32, frame_major=True, tail=tail)
    import torch
    eng.sync()
    assert torch.equal(a.view(torch.int32), c.view(torch.int32)) and torch.equal(d.view(torch.int32), e.view(torch.int32))
    assert torch.equal(f.view(torch.int32), g.view(torch.int32))
    with pytest.raises(ValueError):
        eng.stft_logbin(batch.x, batch.off + starts + 1, cols, N_FFT, 512, True, FLOOR_DB, k_base, first, count, tail=tail)
    with pytest.raises(ValueError):
        eng.stft_logbin(batch.x, batch.off + starts, cols + 1, N_FFT, 512, True, FLOOR_DB, k_base, first, count, tail=tail)


# ---------------------------------------------------------------------------------------------------------- the table alone
LENGTHS = [0, 1, 511, 512, 513, 5000, 300000]


@pytest.fixture(scope="module")
def energy_case():
    rng = np.random.default_rng(3)
    off, pos = [], 1237
    for n in LENGTHS:
        off.append(pos)
        pos += n + 333
    off = np.array(off, dtype=np.int64)
    end = off + np.array(LENGTHS, dtype=np.int64)
    x = (rng.standard_normal(int(end[-1])) * np.exp(-np.arange(int(end[-1])) / 50000.0)).astype(np.float32)
    exact = []
    for o, e in zip(off, end):
        sq = x[o:e].astype(np.float64) ** 2                   # exact: 24-bit significands
        blocks = [math.fsum(sq[i : i + B].tolist()) for i in range(0, sq.size, B)]
        exact.append(np.array([math.fsum(blocks[j:]) for j in range(len(blocks) + 1)]))
    return x, off, end, exact


def _tables(eng, x, off, end):
    t = eng.tail_energy(_dev(eng, x), off, end)
    eng.sync()
    tab = t["tab"].cpu().numpy()
    assert np.array_equal(t["nblk"], -(-(end - off) // B))
    return [tab[int(o) : int(o) + int(nb) + 1] for o, nb in zip(t["off"], t["nblk"])]


def test_tail_energy_against_exact_sums(eng, energy_case):
    x, off, end, exact = energy_case
    got = _tables(eng, x, off, end)
    again = _tables(eng, x, off, end)
    for g, a, ex in zip(got, again, exact):
        assert g.shape == ex.shape and g[-1] == 0.0
        assert np.array_equal(g.view(np.uint64), a.view(np.uint64))
        assert np.all(g * (1.0 + 1e-9) >= ex)
        assert np.all(np.abs(g - ex) <= 1e-12 * ex)


def test_tail_energy_poison(eng, energy_case):
    x, off, end, _ = energy_case
    clean = _tables(eng, x, off, end)
    bad = x.copy()
    at = {5: (2049, np.nan), 6: (123457, np.inf), 4: (512, -np.inf), 2: (510, np.nan)}       # segment: (sample, value)
    for s, (i, v) in at.items():
        bad[off[s] + i] = v
    got = _tables(eng, bad, off, end)
    for s, (g, c) in enumerate(zip(got, clean)):
        hit = at[s][0] // B if s in at else -1
        j = np.arange(g.size)
        assert np.array_equal(np.isfinite(g), j > hit), s
        assert np.array_equal(g[j > hit].view(np.uint64), c[j > hit].view(np.uint64)), s
