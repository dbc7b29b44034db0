"""
Speech transmission index (STI, IEC 60268-16:2011 Annex A, male speech) and the modulation transfer matrix behind it,
from impulse responses by Schroeder's indirect method.

The reference computes neither; this module adds the figure an impulse-response analyser prints beside the ISO 3382
numbers, and the 7 x 14 matrix that shows how a tail smears 1 - 12 Hz envelope detail.

Sums.  For one float32 row x of L samples at rate fs (a band signal of a channel):
  e[n]   = float64(x[n])**2
  w_i    = float64(F_i) / float64(fs), turns per sample, formed on the host, for the modulation frequencies F_i, i < nf
  E      = sum e[n]
  A_i    = sum e[n] cos(2 pi frac(w_i n))
  B_i    = sum e[n] sin(2 pi frac(w_i n))
  m_i    = hypot(A_i, B_i) / E
The sums run over the whole row (ira_mtf_sums, float64, on the device).  No onset is taken because |.| does not depend on a
time shift; for the same reason the circular pre-ringing of the zero-phase band filters does not matter.

Bands: the project's own bank, Rt60BandsAnalysisSettings(band_mode="octave", f_min_hz=125.0, f_max_hz=8000.0): the seven
octaves 125Hz .. 8000Hz made by the engine calls of rt60_bands_device (circular irfft(rfft(x) * mask) over the full
file).  They have the bank's 1/6-octave cosine transitions; they are NOT IEC 61260 filters.  A sample rate at which the
bank has fewer than seven bands is an argument error.
Modulation frequencies (default): 0.63, 0.8, 1.0, 1.25, 1.6, 2.0, 2.5, 3.15, 4.0, 5.0, 6.3, 8.0, 10.0, 12.5 Hz.

Noise: optional snr_db (one value or 7):  m <- m / (1 + 10**(-snr_k / 10)).
Levels: optional band_levels_db (7 values, dB SPL, signal plus noise) switch on auditory masking and the reception
threshold:
  I_k    = 10**(L_k / 10)
  I_am,k = I_{k-1} * 10**(a / 10) for k >= 1, a from L = L_{k-1}:  L < 63: a = 0.5 L - 65;  63 <= L < 67: a = 1.8 L - 146.9;
           67 <= L < 100: a = 0.5 L - 59.8;  L >= 100: a = -10.   I_am,0 = 0.
  I_rt,k = 10**(A_rt,k / 10), A_rt = 46, 27, 12, 6.5, 7.5, 8, 12 dB
  m <- m * I_k / (I_k + I_am,k + I_rt,k)
The noise factor is applied first, the level factor second.

Index arithmetic:
  SNR_eff = clip(10 log10(m / (1 - m)), -15, 15); +15 at m >= 1, -15 at m <= 0
  TI      = (SNR_eff + 15) / 30
  MTI_k   = mean of TI over the modulation frequencies
  STI     = sum alpha_k MTI_k - sum beta_k sqrt(MTI_k MTI_{k+1})
  alpha   = 0.085, 0.127, 0.230, 0.233, 0.309, 0.224, 0.173;  beta = 0.085, 0.078, 0.065, 0.011, 0.047, 0.095
  (sum alpha - sum beta = 1, so m = 1 everywhere gives STI = 1.)
Rating word: bad < 0.30 <= poor < 0.45 <= fair < 0.60 <= good < 0.75 <= excellent.

Per-channel status (bit flags):
  1 silent      E == 0 (a silent channel has E == 0 in every band; a channel with one empty band has no m there and is
                reported the same way).  Every output is NaN.
  2 non-finite  E or any sum not finite, in any band.  Every output is NaN.
  4 short       L / fs < 1 / 0.63 s, less than one period of the lowest standard modulation.  Informational; values are kept.

Command line (no plots): python -m analyse.sti --input A.wav [B.wav ...] | --bundle DIR [--mono] [--snr-db V [V x 7]]
  [--levels-db V x 7] [--expected-sample-rate 48000] [--json OUT.json]
"""
from __future__ import annotations

import argparse
import math
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _measure as M
from ._measure import MAX_BATCH_CHANNELS  # noqa: F401  (part of this module's surface)
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ
from .rt60bands import Rt60BandsAnalysisSettings, band_signals_device

STATUS_SILENT = 1
STATUS_NON_FINITE = 2
STATUS_SHORT = 4
_STATUS_WORDS = ((STATUS_SILENT, "silent"), (STATUS_NON_FINITE, "non-finite"), (STATUS_SHORT, "short"))

NUM_BANDS = 7
BAND_NAMES = ("125Hz", "250Hz", "500Hz", "1000Hz", "2000Hz", "4000Hz", "8000Hz")
MODULATION_FREQUENCIES_HZ = (0.63, 0.8, 1.0, 1.25, 1.6, 2.0, 2.5, 3.15, 4.0, 5.0, 6.3, 8.0, 10.0, 12.5)
MAX_MODULATION_FREQUENCIES = 16   # IRA_MTF_MAX_FREQS
MTF_CHUNK = 16384                 # IRA_MTF_CHUNK: samples per workgroup of ira_mtf_sums
ALPHA = (0.085, 0.127, 0.230, 0.233, 0.309, 0.224, 0.173)
BETA = (0.085, 0.078, 0.065, 0.011, 0.047, 0.095)
RECEPTION_THRESHOLD_DB = (46.0, 27.0, 12.0, 6.5, 7.5, 8.0, 12.0)
RATINGS = ((0.30, "bad"), (0.45, "poor"), (0.60, "fair"), (0.75, "good"))


def sti_band_settings() -> Rt60BandsAnalysisSettings:
    return Rt60BandsAnalysisSettings(band_mode="octave", f_min_hz=125.0, f_max_hz=8000.0)


def _seven(values, what: str) -> Tuple[float, ...]:
    try:
        out = tuple(float(v) for v in values)
    except TypeError:
        out = (float(values),)
    if not all(math.isfinite(v) for v in out):
        raise ValueError(f"{what} must be finite, got {out}")
    return out


@dataclass(frozen=True)
class StiSettings:
    modulation_frequencies_hz: Tuple[float, ...] = MODULATION_FREQUENCIES_HZ
    snr_db: Optional[Tuple[float, ...]] = None             # one value for every band, or 7
    band_levels_db: Optional[Tuple[float, ...]] = None      # 7 values, dB SPL, signal plus noise
    use_mono_downmix_for_stereo: bool = False

    def __post_init__(self):
        try:
            freqs = tuple(float(v) for v in self.modulation_frequencies_hz)
        except TypeError:
            raise ValueError("modulation_frequencies_hz must be a sequence of 1 to 16 frequencies in Hz") from None
        if not 1 <= len(freqs) <= MAX_MODULATION_FREQUENCIES:
            raise ValueError(f"modulation_frequencies_hz needs 1 to {MAX_MODULATION_FREQUENCIES} frequencies, got {len(freqs)}")
        if not all(math.isfinite(v) and v > 0.0 for v in freqs):
            raise ValueError(f"modulation_frequencies_hz must be positive and finite, got {freqs}")
        object.__setattr__(self, "modulation_frequencies_hz", freqs)
        if self.snr_db is not None:
            snr = _seven(self.snr_db, "snr_db")
            if len(snr) == 1:
                snr = snr * NUM_BANDS
            if len(snr) != NUM_BANDS:
                raise ValueError(f"snr_db needs one value or {NUM_BANDS}, got {len(snr)}")
            object.__setattr__(self, "snr_db", snr)
        if self.band_levels_db is not None:
            lev = _seven(self.band_levels_db, "band_levels_db")
            if len(lev) != NUM_BANDS:
                raise ValueError(f"band_levels_db needs {NUM_BANDS} values, got {len(lev)}")
            object.__setattr__(self, "band_levels_db", lev)
        object.__setattr__(self, "use_mono_downmix_for_stereo", bool(self.use_mono_downmix_for_stereo))

    @property
    def bands(self) -> Rt60BandsAnalysisSettings:
        return sti_band_settings()


@dataclass(frozen=True)
class StiChannelResult:
    channel_name: str
    sample_rate_hz: int
    status: int
    sti: float
    rating: str                                  # "NA" when sti is NaN
    band_names: Tuple[str, ...]
    modulation_frequencies_hz: Tuple[float, ...]
    mti: Tuple[float, ...]                       # per band
    mtf: Tuple[Tuple[float, ...], ...]           # (7, nf): m after the noise and level factors


@dataclass
class StiSums:
    """What sti_device leaves on the host: per channel and band the row E, A_0, B_0, ..."""
    band_names: List[str]
    length: np.ndarray                           # int64 (nch,)
    sums: np.ndarray                             # float64 (nch, 7, 2 nf + 1)


def status_text(status: int) -> str:
    return M.status_text(status, _STATUS_WORDS)


def rating_word(sti: float) -> str:
    if math.isnan(sti):
        return "NA"
    for limit, word in RATINGS:
        if sti < limit:
            return word
    return "excellent"


def modulation_turns(modulation_frequencies_hz: Sequence[float], sample_rate_hz: float) -> np.ndarray:
    """w_i = float64(F_i) / float64(fs), turns per sample."""
    w = np.array([float(f) / float(sample_rate_hz) for f in modulation_frequencies_hz], dtype=np.float64)
    if np.any(w > 0.5):
        raise ValueError(f"modulation frequencies above half the sample rate {sample_rate_hz}")
    return w


# ---------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------


def sti_device(eng, batch, sample_rate_hz: int, settings: Optional[StiSettings] = None, band_signals=None) -> StiSums:
    """The modulation transfer sums of every band of every channel of a device batch in ONE ira_mtf_sums launch (row
    c * 7 + k is band k of channel c).  band_signals = (bands, y device, y_off (nch, 7)) as band_signals_device returns them
    for sti_band_settings() lets a caller that already built the band signals skip the filter bank."""
    settings = settings or StiSettings()
    nch = batch.count
    w = modulation_turns(settings.modulation_frequencies_hz, sample_rate_hz)
    if band_signals is None:
        band_signals = band_signals_device(eng, batch, sample_rate_hz, settings.bands)
    bands, y, y_off = band_signals
    names = [b.name for b in bands]
    if tuple(names) != BAND_NAMES:
        raise ValueError(f"STI needs the seven octave bands {', '.join(BAND_NAMES)}; the bank at {sample_rate_hz} Hz has "
                         f"{', '.join(names) or 'none'}")
    y_off = np.asarray(y_off, dtype=np.int64).reshape(nch, NUM_BANDS)
    nrec = 2 * w.size + 1
    if nch:
        out = eng.mtf_sums(y, y_off.reshape(-1), np.repeat(batch.length.astype(np.int64), NUM_BANDS),
                           np.tile(w, (nch * NUM_BANDS, 1)))
        sums = out.cpu().numpy().reshape(nch, NUM_BANDS, nrec)
    else:
        sums = np.zeros((0, NUM_BANDS, nrec))
    return StiSums(band_names=names, length=batch.length.astype(np.int64).copy(), sums=sums)


# ---------------------------------------------------------------------------------------------------
# host: sums -> m -> STI
# ---------------------------------------------------------------------------------------------------


def mtf_from_sums(sums: np.ndarray) -> np.ndarray:
    """m (..., nf) = hypot(A_i, B_i) / E from rows (..., 2 nf + 1) = E, A_0, B_0, ...; NaN where E is 0."""
    s = np.asarray(sums, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.hypot(s[..., 1::2], s[..., 2::2]) / s[..., :1]


def masking_slope_db(level_db: float) -> float:
    """a of the auditory masking of band k by the level L of band k - 1."""
    lv = float(level_db)
    if lv < 63.0:
        return 0.5 * lv - 65.0
    if lv < 67.0:
        return 1.8 * lv - 146.9
    if lv < 100.0:
        return 0.5 * lv - 59.8
    return -10.0


def level_factors(band_levels_db: Sequence[float]) -> np.ndarray:
    """I_k / (I_k + I_am,k + I_rt,k) per band."""
    lev = [float(v) for v in band_levels_db]
    out = np.empty(NUM_BANDS, dtype=np.float64)
    for k in range(NUM_BANDS):
        i_k = 10.0 ** (lev[k] / 10.0)
        i_am = 0.0 if k == 0 else 10.0 ** (lev[k - 1] / 10.0) * 10.0 ** (masking_slope_db(lev[k - 1]) / 10.0)
        i_rt = 10.0 ** (RECEPTION_THRESHOLD_DB[k] / 10.0)
        out[k] = i_k / (i_k + i_am + i_rt)
    return out


def apply_noise_and_levels(m: np.ndarray, snr_db: Optional[Sequence[float]] = None,
                           band_levels_db: Optional[Sequence[float]] = None) -> np.ndarray:
    """m (..., 7, nf) with the noise factor first and the level factor second (either may be None)."""
    out = np.array(m, dtype=np.float64, copy=True)
    if snr_db is not None:
        snr = np.asarray([float(v) for v in snr_db], dtype=np.float64)
        out = out / (1.0 + 10.0 ** (-snr / 10.0))[:, None]
    if band_levels_db is not None:
        out = out * level_factors(band_levels_db)[:, None]
    return out


def transmission_index(m: np.ndarray) -> np.ndarray:
    m = np.asarray(m, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = 10.0 * np.log10(m / (1.0 - m))
    snr = np.where(m >= 1.0, 15.0, np.where(m <= 0.0, -15.0, np.clip(snr, -15.0, 15.0)))
    snr = np.where(np.isnan(m), np.nan, snr)
    return (snr + 15.0) / 30.0


def sti_from_mtf(m: np.ndarray):
    """(STI (...), MTI (..., 7)) from m (..., 7, nf)."""
    mti = np.mean(transmission_index(m), axis=-1)
    a, b = np.asarray(ALPHA), np.asarray(BETA)
    sti = np.sum(a * mti, axis=-1) - np.sum(b * np.sqrt(mti[..., :-1] * mti[..., 1:]), axis=-1)
    return sti, mti


def sti_results(res: StiSums, sample_rate_hz: int, channel_names: Sequence[str],
                settings: StiSettings) -> List[StiChannelResult]:
    m = apply_noise_and_levels(mtf_from_sums(res.sums), settings.snr_db, settings.band_levels_db)
    sti, mti = sti_from_mtf(m)
    out = []
    nan = float("nan")
    for ch, name in enumerate(channel_names):
        rows = res.sums[ch]
        status = 0
        if not np.all(np.isfinite(rows)):
            status |= STATUS_NON_FINITE
        elif np.any(rows[:, 0] == 0.0):
            status |= STATUS_SILENT
        if float(res.length[ch]) / float(sample_rate_hz) < 1.0 / 0.63:
            status |= STATUS_SHORT
        bad = bool(status & (STATUS_SILENT | STATUS_NON_FINITE))
        v = nan if bad else float(sti[ch])
        out.append(StiChannelResult(
            channel_name=str(name), sample_rate_hz=int(sample_rate_hz), status=status, sti=v, rating=rating_word(v),
            band_names=tuple(res.band_names), modulation_frequencies_hz=tuple(settings.modulation_frequencies_hz),
            mti=tuple(nan if bad else float(x) for x in mti[ch]),
            mtf=tuple(tuple(nan if bad else float(x) for x in row) for row in m[ch])))
    return out


# ---------------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------------


def _results_of_batch(eng, batch, sample_rate_hz, names, settings) -> List[StiChannelResult]:
    return sti_results(sti_device(eng, batch, sample_rate_hz, settings), sample_rate_hz, names, settings)


def analyse_sti_batch(channels: Sequence[np.ndarray], sample_rate_hz: int, channel_names: Sequence[str],
                      settings: Optional[StiSettings] = None) -> List[StiChannelResult]:
    """Every channel through the device in batches of at most MAX_BATCH_CHANNELS channels."""
    return M.analyse_channel_batches(channels, sample_rate_hz, channel_names, settings or StiSettings(), _results_of_batch)


def analyse_sti_from_wav_file(input_wav_file_path: str | Path, settings: Optional[StiSettings] = None,
                              expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> List[StiChannelResult]:
    """One WAV file (mono or stereo, rate checked against expected_sample_rate_hz); channels named as by
    get_analysis_channels ("mono", "left", "right")."""
    return M.analyse_wav_file_channels(input_wav_file_path, settings or StiSettings(), expected_sample_rate_hz,
                                       analyse_sti_batch)


def analyse_sti_files(paths: Sequence[str | Path], settings: Optional[StiSettings] = None,
                      expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> List[StiChannelResult]:
    """Every channel of every file in one device batch per MAX_BATCH_CHANNELS channels; channels named
    "<file name>:<channel>"."""
    return M.analyse_file_channels(paths, settings or StiSettings(), expected_sample_rate_hz, analyse_sti_batch)


def analyse_sti_bundle(bundle_root: str | Path, settings: Optional[StiSettings] = None,
                       expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> List[StiChannelResult]:
    """The taps a bundle's meta.json lists (taps/<name>.wav), read by the native ingest (ingest.TapSet) a group at a
    time (at most MAX_BATCH_CHANNELS channels per group); channels named "<tap>:<channel>"."""
    return M.analyse_bundle_channels(bundle_root, settings or StiSettings(), expected_sample_rate_hz, _results_of_batch)


# ---------------------------------------------------------------------------------------------------
# text, Markdown, JSON
# ---------------------------------------------------------------------------------------------------


def _columns(r: StiChannelResult) -> List[str]:
    return ["MTI"] + [f"{f:g}Hz" for f in r.modulation_frequencies_hz]


def _rows(r: StiChannelResult) -> List[List[str]]:
    return [[name, M.fmt(mti)] + [M.fmt(v) for v in row] for name, mti, row in zip(r.band_names, r.mti, r.mtf)]


def summarise_sti_text(channel_results: List[StiChannelResult]) -> str:
    """
    Fixed text format, one block per channel followed by an empty line:
        [<channel name>]
        STI: <3 decimals> (<rating word>)  Status: ok | <flags> (<words>)
        Band  MTI  0.63Hz  0.8Hz  ...
        <band name>  <MTI, 3 decimals>  <m, 3 decimals>  ...      (one row per band, ascending)
    Cells are separated by two spaces; NaN is "NA".
    """
    return M.join_blocks(M.text_block(
        r.channel_name, f"STI: {M.fmt(r.sti)} ({r.rating})  Status: {status_text(r.status)}", _columns(r), _rows(r))
        for r in channel_results)


def summarise_sti_markdown(channel_results: List[StiChannelResult]) -> str:
    """The same values as a Markdown section per channel: a '### <channel name>' heading, an STI / status line and the
    modulation transfer matrix as a table (rows: bands; columns: MTI, then m per modulation frequency)."""
    return M.join_blocks(M.markdown_block(
        r.channel_name, f"STI: {M.fmt(r.sti)} ({r.rating}). Status: {status_text(r.status)}.", _columns(r), _rows(r))
        for r in channel_results)


def sti_results_to_json(channel_results: List[StiChannelResult]) -> Dict:
    """Plain JSON: NaN is null."""
    rows = []
    for r in channel_results:
        rows.append({
            "channel_name": r.channel_name, "sample_rate_hz": r.sample_rate_hz, "status": r.status,
            "sti": M.json_num(r.sti), "rating": r.rating,
            "modulation_frequencies_hz": list(r.modulation_frequencies_hz),
            "bands": [dict(name=n, mti=M.json_num(v), mtf=[M.json_num(x) for x in row])
                      for n, v, row in zip(r.band_names, r.mti, r.mtf)],
        })
    return {"sti": rows}


def sti_results_from_json(doc: Dict) -> List[StiChannelResult]:
    out = []
    for d in doc["sti"]:
        out.append(StiChannelResult(
            channel_name=d["channel_name"], sample_rate_hz=int(d["sample_rate_hz"]), status=int(d["status"]),
            sti=M.num_json(d["sti"]), rating=str(d["rating"]), band_names=tuple(b["name"] for b in d["bands"]),
            modulation_frequencies_hz=tuple(float(v) for v in d["modulation_frequencies_hz"]),
            mti=tuple(M.num_json(b["mti"]) for b in d["bands"]),
            mtf=tuple(tuple(M.num_json(x) for x in b["mtf"]) for b in d["bands"])))
    return out


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m analyse.sti",
        description="Speech transmission index (IEC 60268-16, male) and the modulation transfer matrix per channel.")
    M.add_source_arguments(p)
    p.add_argument("--snr-db", nargs="+", type=float, default=None,
                   help="signal-to-noise ratio in dB: one value for every band, or 7 (125 Hz .. 8 kHz)")
    p.add_argument("--levels-db", nargs=NUM_BANDS, type=float, default=None,
                   help="band levels in dB SPL (signal plus noise), 7 values: switches on masking and the reception threshold")
    M.add_output_arguments(p)
    return p


def settings_from_args(args) -> StiSettings:
    return StiSettings(snr_db=None if args.snr_db is None else tuple(args.snr_db),
                       band_levels_db=None if args.levels_db is None else tuple(args.levels_db),
                       use_mono_downmix_for_stereo=bool(args.mono))


def main(argv: Optional[Sequence[str]] = None) -> None:
    M.run_cli(build_parser(), argv, settings_from_args, analyse_sti_files, analyse_sti_bundle, summarise_sti_text,
              sti_results_to_json)


if __name__ == "__main__":
    main()
