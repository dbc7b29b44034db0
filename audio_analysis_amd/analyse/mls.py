"""
Impulse responses from recordings of a maximum-length sequence (MLS), the second excitation of ISO 18233 beside the swept
sine of deconvolve.py: circular correlation over the odd period by a fast Walsh-Hadamard transform (Cohn and Lempel; Borish
and Angell; Rife and Vanderkooy).  The result has the layout of deconvolve.deconvolve_device, so the report
blocks, lundeby, sti, minphase and the rest consume it unchanged.

Order m (2 .. 21), period P = 2^m - 1, taps T (engine.MLS_TAPS[m] unless given):

  bits      a[n] = XOR over t in T of a[n - t],  a[0 .. m-1] = 1                                        (engine.mls_bits)
  stimulus  s[n] = 1 - 2 a[n], so sum s = -1 and the circular autocorrelation is P at lag 0 and -1 elsewhere

For a channel x (float32) of L samples and the settings start_samples (0), skip_periods (1: the first period carries the
transient) and periods (None: every whole period that fits):

  b      = start_samples + skip_periods P
  R      = periods, or floor((L - b) / P);  ValueError naming the channel if R < 1, b + R P > L or R > 1024
  Y[n]   = sum over r = 0 .. R-1, ascending, of float64(x[b + r P + n]),  n < P
  D      = sum over n and r of (float64(x[b + r P + n]) - Y[n] / R)^2     (what differs between periods; 0 when R = 1)
  E      = sum over n of Y[n]^2
  c[k]   = sum over n of s[n] Y[(n + k) mod P]
  h[k]   = (c[k] - sum Y) / (2^m R),  k < P

The last line is exact, DC included: for y = h (*) s circularly, c[k] = R ((P + 1) h[k] - sum h) and sum Y = -R sum h.
h is the response to the +-1 sequence: the level the stimulus was played at (0.5 from `generate`) stays in it as a factor.
On the device (ira_mls_fold -> ira_mls_hadamard -> ira_mls_finish, one order and one R per chain):

  w     = zeros(2^m);  w[G[j]] = Y[j]                                      (engine.mls_tables gives G and out)
  W     = FWHT(w) in natural order, stages h = 1, 2, 4 .. 2^(m-1) in that order, (lo, hi) -> (lo + hi, lo - hi)
  h[k]  = float32((W[out[k]] - W[0]) / float64(2^m R))                     (W[0] = sum Y)

The stage order fixes every rounding: the device equals tests/mls_ref.py's float64 restatement bit for bit for any input,
and for samples on the PCM16 grid (k / 32768) nothing rounds before the division (m + 16 + ceil(log2 R) <= 53 always).

Then deconvolve.py's conventions (Engine.deconv_finish): the mean is removed per channel (remove_dc) and every file is
scaled so that its largest |h| is target_peak (normalise_peak).  Per channel the result records the order, P, R, b, the peak
(first index of max |h| and that |h|, before DC removal and scaling) and

  period_snr_db = 10 log10((E / R) / D): the energy of the averaged period over what differs between periods; NaN when
                  R = 1, +inf when D = 0.

A channel of digital silence gives zeros.  A channel with a NaN or an infinity among its samples comes back all NaN and
touches no other channel: it is kept out of its file's peak.  (A finite channel whose response overflows float32 -- samples
beyond 1.7e38 -- is not caught before the scaling.)

The defaults (order 16: 1.37 s at 48 kHz; one skipped period) are conventions of measurement tools, not citations.

Command line:
  python -m analyse.mls generate   --order 16 --periods 4 [--amplitude 0.5] [--sample-rate 48000] --output S.wav
  python -m analyse.mls deconvolve --recorded A.wav [B.wav ...] --order 16 [--skip-periods 1] [--periods N]
                                   [--start-samples 0] [--mono] [--no-normalise] [--keep-dc] [--output-dir DIR]
                                   [--expected-sample-rate 48000] [--json OUT.json]
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _measure as M
from .. import engine as E
from ..engine import MLS_MAX_ORDER, MLS_MAX_PERIODS, MLS_MIN_ORDER, MLS_TAPS, mls_bits, mls_tables, mls_taps  # noqa: F401
from ._measure import MAX_BATCH_CHANNELS  # noqa: F401  (part of this module's surface)
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ


@dataclass(frozen=True)
class MlsSettings:
    order: int = 16
    taps: Optional[Tuple[int, ...]] = None         # None: engine.MLS_TAPS[order]
    start_samples: int = 0                         # where the first period of the stimulus begins in the recording
    skip_periods: int = 1                          # periods left out in front (the transient)
    periods: Optional[int] = None                  # None: every whole period that fits
    use_mono_downmix_for_stereo: bool = False
    normalise_peak: bool = True
    target_peak: float = 0.95
    remove_dc: bool = True

    def __post_init__(self):
        def whole(name, least, most=None):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least or (most is not None and v > most):
                rng = f">= {least}" if most is None else f"{least}..{most}"
                raise ValueError(f"{name} must be a whole number {rng}, got {v!r}")
            return int(v)

        order = whole("order", MLS_MIN_ORDER, MLS_MAX_ORDER)
        start, skip = whole("start_samples", 0), whole("skip_periods", 0)
        periods = None if self.periods is None else whole("periods", 1, MLS_MAX_PERIODS)
        try:
            peak = float(self.target_peak)
        except (TypeError, ValueError):
            raise ValueError(f"target_peak must be a number, got {self.target_peak!r}") from None
        if not (math.isfinite(peak) and peak > 0.0):
            raise ValueError(f"target_peak must be finite and > 0, got {self.target_peak}")
        taps = None
        if self.taps is not None:
            taps = mls_taps(order, self.taps)
            mls_tables(order, taps)                # ValueError unless the taps give the full period
        for k, v in (("order", order), ("start_samples", start), ("skip_periods", skip), ("periods", periods),
                     ("target_peak", peak), ("taps", taps)):
            object.__setattr__(self, k, v)

    @property
    def period_samples(self) -> int:
        return (1 << self.order) - 1


@dataclass(frozen=True, eq=False)
class MlsChannelResult:
    channel_name: str
    sample_rate_hz: int
    order: int
    period_samples: int                            # P
    periods: int                                   # R
    begin_samples: int                             # b
    peak_samples: int                              # first index of max |h|, before DC removal and scaling
    peak_value: float                              # that |h|; NaN for a channel without finite values
    period_snr_db: float                           # 10 log10((E / R) / D); NaN when R = 1, +inf when D = 0


def mls_sequence(order: int, taps=None) -> np.ndarray:
    """One period of the stimulus s[n] = 1 - 2 a[n] as int8 (+1 / -1); its sum is -1."""
    return (1 - 2 * mls_bits(order, taps).astype(np.int8)).astype(np.int8)


def mls_stimulus(order: int, periods: int, amplitude: float = 0.5, taps=None) -> np.ndarray:
    """`periods` periods of the sequence at +-amplitude, float32 (periods * P,)."""
    if isinstance(periods, bool) or not isinstance(periods, (int, np.integer)) or periods < 1:
        raise ValueError(f"periods must be a whole number >= 1, got {periods!r}")
    if not (math.isfinite(float(amplitude)) and 0.0 < float(amplitude) <= 1.0):
        raise ValueError(f"amplitude must lie in (0, 1], got {amplitude}")
    return np.tile(mls_sequence(order, taps).astype(np.float32) * np.float32(amplitude), int(periods))


def mls_layout(lengths, settings: MlsSettings, channel_names: Optional[Sequence[str]] = None) -> Tuple[int, np.ndarray]:
    """(b, R): the first averaged sample and the periods of every channel (int64).  ValueError naming the channel where
    R < 1, b + R P > L or R > MLS_MAX_PERIODS."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    p = settings.period_samples
    b = settings.start_samples + settings.skip_periods * p
    out = np.zeros(lengths.size, dtype=np.int64)
    for c, n in enumerate(lengths.tolist()):
        name = f"channel {c}" if channel_names is None else str(channel_names[c])
        r = settings.periods if settings.periods is not None else (n - b) // p
        if r < 1 or b + r * p > n:
            raise ValueError(f"{name}: {n} samples do not hold {max(r, 1)} period(s) of {p} samples from sample {b} on "
                             f"(order {settings.order}, start_samples {settings.start_samples}, skip_periods "
                             f"{settings.skip_periods})")
        if r > MLS_MAX_PERIODS:
            raise ValueError(f"{name}: {r} periods fit, at most {MLS_MAX_PERIODS} are averaged: set periods")
        out[c] = r
    return b, out


def period_snr_db(e: float, d: float, periods: int) -> float:
    """10 log10((E / R) / D); NaN when R = 1 (or a sum is not a number), +inf when D = 0."""
    if periods <= 1 or math.isnan(e) or math.isnan(d):
        return math.nan
    if d == 0.0:
        return math.inf
    ratio = (e / float(periods)) / d
    return 10.0 * math.log10(ratio) if ratio > 0.0 else (-math.inf if ratio == 0.0 else math.nan)


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def mls_device(eng, recorded, file_of_channel: Sequence[int], settings: Optional[MlsSettings] = None,
               channel_names: Optional[Sequence[str]] = None) -> Dict:
    """Batched MLS measurement on the device.  `recorded`: the channels of one or many recordings; file_of_channel[e] = the
    recording channel e belongs to (the channels of a file share the peak normalisation).  Returns dict(h=flat float32
    device buffer, off, n_out, n_fft, sums, periods, begin, peak, peak_abs): channel e's response is
    h[off[e] : off[e] + n_out[e]], n_out = P, n_fft = 2^order (the layout of deconvolve_device); sums (nb, 2) float64 host:
    E and D; periods: R per channel; peak / peak_abs: the first index of max |h| and that |h| before deconv_finish.
    Channels are grouped by R and cut into chains of calls whose workspace stays under engine.MLS_SCRATCH_BYTES; no result
    depends on the grouping."""
    settings = settings or MlsSettings()
    t = eng.torch
    nb, m, p = recorded.count, settings.order, settings.period_samples
    group = np.array(file_of_channel, dtype=np.int32).reshape(-1)
    if group.size != nb:
        raise ValueError("one file index per channel")
    b, periods = mls_layout(recorded.length, settings, channel_names)
    off = np.arange(nb, dtype=np.int64) << m
    n_out, n_fft = np.full(nb, p, dtype=np.int32), np.full(nb, 1 << m, dtype=np.int32)
    sums = np.zeros((nb, 2))
    if nb == 0:
        return dict(h=eng.empty(0, t.float32), off=off, n_out=n_out, n_fft=n_fft, sums=sums, periods=periods, begin=b,
                    peak=np.zeros(0, np.int64), peak_abs=np.zeros(0, np.float32))
    h = eng.empty(nb << m, t.float32)
    h.zero_()
    per_chain = max(1, min(65535, E.MLS_SCRATCH_BYTES // E.mls_scratch_bytes(1, m)))
    for r in np.unique(periods).tolist():
        idx_r = np.nonzero(periods == r)[0]
        for a in range(0, idx_r.size, per_chain):
            idx = idx_r[a : a + per_chain]
            w, s = eng.mls_fold(recorded.x, recorded.off[idx] + b, m, r, settings.taps)
            eng.mls_hadamard(w, idx.size, m)
            eng.mls_finish(w, idx.size, m, r, h, off[idx], settings.taps)
            sums[idx] = s.cpu().numpy().reshape(idx.size, 2)
    pk, pa = eng.harmonic_peaks(h, off, n_out.astype(np.int64))
    peak, peak_abs = pk.cpu().numpy().astype(np.int64)[:nb].copy(), pa.cpu().numpy().astype(np.float32)[:nb].copy()
    # a channel whose folded period is not finite is a file of its own for the epilogue: its NaN stays out of its file's peak
    bad = np.nonzero(~np.isfinite(sums[:, 0]))[0]
    if bad.size:
        group[bad] = (int(group.max()) + 1 if nb else 0) + np.arange(bad.size, dtype=np.int32)
    eng.deconv_finish(h, off, n_out, group, bool(settings.remove_dc), bool(settings.normalise_peak),
                      float(settings.target_peak))
    return dict(h=h, off=off, n_out=n_out, n_fft=n_fft, sums=sums, periods=periods, begin=b, peak=peak, peak_abs=peak_abs)


def _results_of_device(dev: Dict, sample_rate_hz: int, names: Sequence[str], settings: MlsSettings,
                       responses: Sequence[np.ndarray]) -> List[MlsChannelResult]:
    out = []
    for c, name in enumerate(names):
        finite = bool(np.all(np.isfinite(responses[c])))
        out.append(MlsChannelResult(
            channel_name=str(name), sample_rate_hz=int(sample_rate_hz), order=settings.order,
            period_samples=settings.period_samples, periods=int(dev["periods"][c]), begin_samples=int(dev["begin"]),
            peak_samples=int(dev["peak"][c]), peak_value=float(dev["peak_abs"][c]) if finite else math.nan,
            period_snr_db=period_snr_db(float(dev["sums"][c, 0]), float(dev["sums"][c, 1]), int(dev["periods"][c]))))
    return out


def mls_impulse_responses(channels: Sequence[np.ndarray], sample_rate_hz: int, settings: Optional[MlsSettings] = None,
                          eng=None, file_of_channel: Optional[Sequence[int]] = None,
                          channel_names: Optional[Sequence[str]] = None) -> Tuple[List[np.ndarray], List[MlsChannelResult]]:
    """The response of every channel: (float32 arrays of P samples each, an MlsChannelResult per channel).
    file_of_channel: which channels share a peak normalisation (default: all of them, one recording); files are never
    split between device batches.  A channel of silence comes back as zeros, a channel with a non-finite sample as NaN."""
    settings = settings or MlsSettings()
    eng = eng or E.get_engine()
    chans = [np.asarray(c, dtype=np.float32).reshape(-1) for c in channels]
    files = np.zeros(len(chans), dtype=np.int64) if file_of_channel is None else np.asarray(file_of_channel, dtype=np.int64)
    names = [f"channel {c}" for c in range(len(chans))] if channel_names is None else [str(n) for n in channel_names]
    if files.size != len(chans) or len(names) != len(chans):
        raise ValueError("one file index and one name per channel")
    mls_layout([c.size for c in chans], settings, names)          # every channel's error before anything is uploaded
    hs: List[Optional[np.ndarray]] = [None] * len(chans)
    results: List[Optional[MlsChannelResult]] = [None] * len(chans)
    # batches of whole files: files are added while the batch stays within MAX_BATCH_CHANNELS channels
    batches: List[List[int]] = []
    for f in np.unique(files).tolist():
        members = np.nonzero(files == f)[0].tolist()
        if batches and len(batches[-1]) + len(members) <= MAX_BATCH_CHANNELS:
            batches[-1] += members
        else:
            batches.append(members)
    for idx in batches:
        batch = eng.upload([chans[i] for i in idx])
        sub = [names[i] for i in idx]
        dev = mls_device(eng, batch, np.unique(files[idx], return_inverse=True)[1], settings, sub)
        host = dev["h"].cpu().numpy()
        part = []
        for o, n in zip(dev["off"], dev["n_out"]):
            v = host[int(o) : int(o) + int(n)].astype(np.float32)
            part.append(v if np.all(np.isfinite(v)) else np.full(int(n), np.nan, dtype=np.float32))
        for i, v, r in zip(idx, part, _results_of_device(dev, sample_rate_hz, sub, settings, part)):
            hs[i], results[i] = v, r
    return hs, results


# ---------------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------------


def default_output_ir_path(recorded_wav_file_path: str | Path, output_dir: Optional[str | Path] = None) -> Path:
    """<recorded stem>_ir.wav, beside the recording or in output_dir."""
    p = Path(recorded_wav_file_path)
    return (p.parent if output_dir is None else Path(output_dir)) / f"{p.stem}_ir.wav"


def mls_from_wav_files(recorded_paths: Sequence[str | Path], settings: Optional[MlsSettings] = None,
                       expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
                       output_dir: Optional[str | Path] = None, write: bool = False):
    """Every channel of every recording (mono or stereo WAV, rate checked; named "<file name>:<channel>"), the channels of
    a file sharing the peak normalisation.  Returns (responses: per file a float32 (P, C) array, results: an
    MlsChannelResult per channel, written: the paths of the <stem>_ir.wav files, float32, when write is set)."""
    from ._common import wav_channels
    from .deconvolve import _write_wav_float32

    settings = settings or MlsSettings()
    chans, names, files = [], [], []
    for f, p in enumerate(recorded_paths):
        _, cs = wav_channels(p, settings.use_mono_downmix_for_stereo, expected_sample_rate_hz=expected_sample_rate_hz)
        for n, c in cs:
            chans.append(c)
            names.append(f"{Path(p).name}:{n}")
            files.append(f)
    hs, results = mls_impulse_responses(chans, int(expected_sample_rate_hz), settings, file_of_channel=files,
                                        channel_names=names)
    responses, written = [], []
    for f, p in enumerate(recorded_paths):
        cols = [h for h, g in zip(hs, files) if g == f]
        responses.append(np.stack(cols, axis=1).astype(np.float32))
        if write:
            target = default_output_ir_path(p, output_dir)
            _write_wav_float32(target, int(expected_sample_rate_hz), responses[-1])
            written.append(target)
    return responses, results, written


def write_mls_stimulus(path: str | Path, order: int, periods: int, amplitude: float = 0.5,
                       sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ, taps=None) -> Path:
    """`periods` periods of the sequence as a mono float32 WAV."""
    from .deconvolve import _write_wav_float32
    _write_wav_float32(Path(path), int(sample_rate_hz), mls_stimulus(order, periods, amplitude, taps).reshape(-1, 1))
    return Path(path)


# ---------------------------------------------------------------------------------------------------
# text, Markdown, JSON
# ---------------------------------------------------------------------------------------------------

_COLUMNS = ["periods", "begin_samples", "peak_samples", "peak_ms", "peak_value", "period_snr_dB"]
_MD_COLUMNS = ["periods", "begin (samples)", "peak (samples)", "peak (ms)", "peak value", "period SNR (dB)"]


def _row(r: MlsChannelResult) -> List[str]:
    return [str(r.periods), str(r.begin_samples), str(r.peak_samples),
            M.fmt(1000.0 * r.peak_samples / float(r.sample_rate_hz), 3), M.fmt(r.peak_value, 6), M.fmt(r.period_snr_db, 2)]


def _head(r: MlsChannelResult, sep: str, end: str) -> str:
    return (f"Order: {r.order}{sep}Period: {r.period_samples} samples "
            f"({r.period_samples / float(r.sample_rate_hz):.4f} s at {r.sample_rate_hz} Hz){end}")


def summarise_mls_text(channel_results: List[MlsChannelResult]) -> str:
    """
    Fixed text format, one block per channel followed by an empty line:
        [<channel name>]
        Order: <m>  Period: <P> samples (<P / fs, 4 decimals> s at <fs> Hz)
        value  periods  begin_samples  peak_samples  peak_ms  peak_value  period_snr_dB
        response  <R>  <b>  <index>  <3 decimals>  <6 decimals>  <2 decimals>
    Cells are separated by two spaces; NaN is "NA", an infinity "+inf".  The peak is taken before DC removal and scaling.
    """
    return M.join_blocks(M.text_block(r.channel_name, _head(r, "  ", ""), _COLUMNS, [["response", *_row(r)]], first="value")
                         for r in channel_results)


def summarise_mls_markdown(channel_results: List[MlsChannelResult]) -> str:
    """The same values as a Markdown section per channel: a '### <channel name>' heading, the order / period line and a
    one-row table."""
    return M.join_blocks(M.markdown_block(r.channel_name, _head(r, ". ", "."), _MD_COLUMNS, [["response", *_row(r)]],
                                          first="value") for r in channel_results)


_INT_FIELDS = ("sample_rate_hz", "order", "period_samples", "periods", "begin_samples", "peak_samples")
_NUM_FIELDS = ("peak_value", "period_snr_db")


def mls_results_to_json(channel_results: List[MlsChannelResult]) -> Dict:
    """Plain JSON: NaN is null, an infinity the string "+inf" / "-inf"."""
    return {"mls": [dict(channel_name=r.channel_name, **{k: int(getattr(r, k)) for k in _INT_FIELDS},
                         **{k: M.json_num(float(getattr(r, k))) for k in _NUM_FIELDS}) for r in channel_results]}


def mls_results_from_json(doc: Dict) -> List[MlsChannelResult]:
    return [MlsChannelResult(channel_name=str(d["channel_name"]), **{k: int(d[k]) for k in _INT_FIELDS},
                             **{k: M.num_json(d[k]) for k in _NUM_FIELDS}) for d in doc["mls"]]


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.mls",
        description="Impulse responses from maximum-length-sequence recordings by the fast Hadamard transform (ISO 18233), "
                    "and the stimulus to record them with.")
    sub = p.add_subparsers(dest="command", required=True)
    g = sub.add_parser("generate", help="write the stimulus as a mono float32 WAV")
    g.add_argument("--order", type=int, default=16, help=f"sequence order m, {MLS_MIN_ORDER} to {MLS_MAX_ORDER}: the period is "
                                                          "2^m - 1 samples (default: 16)")
    g.add_argument("--periods", type=int, required=True, help="periods to write (one more than will be averaged)")
    g.add_argument("--amplitude", type=float, default=0.5, help="level of the +-1 sequence, 0 to 1 (default: 0.5)")
    g.add_argument("--sample-rate", type=int, default=DEFAULT_EXPECTED_SAMPLE_RATE_HZ, help="sample rate in Hz (default: 48000)")
    g.add_argument("--output", type=Path, required=True, help="the WAV file to write")
    d = sub.add_parser("deconvolve", help="recordings -> impulse responses, <stem>_ir.wav per recording")
    d.add_argument("--recorded", nargs="+", type=Path, required=True,
                   help="recorded WAV files (every channel of every file is measured)")
    d.add_argument("--order", type=int, default=16, help="order of the sequence that was played (default: 16)")
    d.add_argument("--skip-periods", type=int, default=1, help="periods left out in front, the transient (default: 1)")
    d.add_argument("--periods", type=int, default=None, help="periods to average (default: every whole period that fits)")
    d.add_argument("--start-samples", type=int, default=0,
                   help="where the first period of the stimulus begins in the recording (default: 0)")
    d.add_argument("--mono", action="store_true", help="measure stereo recordings as their mono downmix 0.5 * (L + R)")
    d.add_argument("--no-normalise", action="store_true", help="keep the measured scale (default: peak 0.95 per file)")
    d.add_argument("--keep-dc", action="store_true", help="keep the mean of the response (default: removed)")
    d.add_argument("--output-dir", type=Path, default=None, help="where the responses go (default: beside each recording)")
    M.add_output_arguments(d)
    return p


def settings_from_args(args) -> MlsSettings:
    return MlsSettings(order=args.order, start_samples=args.start_samples, skip_periods=args.skip_periods,
                       periods=args.periods, use_mono_downmix_for_stereo=bool(args.mono),
                       normalise_peak=not args.no_normalise, remove_dc=not args.keep_dc)


def main(argv: Optional[Sequence[str]] = None) -> None:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.command == "generate":
        try:
            path = write_mls_stimulus(args.output, args.order, args.periods, args.amplitude, args.sample_rate)
        except ValueError as e:
            parser.error(str(e))
        p = (1 << args.order) - 1
        sys.stdout.write(f"{path}: order {args.order}, {args.periods} periods of {p} samples, +-{args.amplitude:g}\n")
        return
    try:
        settings = settings_from_args(args)
    except ValueError as e:
        parser.error(str(e))
    _, results, written = mls_from_wav_files(args.recorded, settings, args.expected_sample_rate, args.output_dir, write=True)
    sys.stdout.write(summarise_mls_text(results))
    for w in written:
        sys.stdout.write(f"wrote {w}\n")
    sys.stdout.flush()
    if args.json is not None:
        args.json.write_text(json.dumps(mls_results_to_json(results), indent=2) + "\n")


if __name__ == "__main__":
    main()
