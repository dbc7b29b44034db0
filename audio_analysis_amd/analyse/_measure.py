"""What the per-channel measure modules (energy, iacc, lundeby, sti, harmonics) share beyond their arithmetic: the batch, file and
bundle drivers, the cells, band rows and blocks of their text / Markdown / JSON output, and the command-line skeleton.
A measure module holds its settings, its device function, its host arithmetic and thin entry points built from these."""
from __future__ import annotations

import json
import math
import sys
from pathlib import Path
from typing import Callable, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from ..engine import get_engine
from ._common import wav_channels
from .io import DEFAULT_EXPECTED_SAMPLE_RATE_HZ
from .rt60bands import BandDefinition

MAX_BATCH_CHANNELS = 256          # channels per device batch (the CLI's chunk)
BAND_MODES = ("three", "octave", "third")

# ---------------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------------


def analyse_channel_batches(channels: Sequence[np.ndarray], sample_rate_hz: int, channel_names: Sequence[str], settings,
                            results_of_batch: Callable, eng=None) -> list:
    """Every channel through the device in batches of at most MAX_BATCH_CHANNELS channels: each chunk is uploaded as
    contiguous float32 and handed to results_of_batch(eng, batch, sample_rate_hz, names of the chunk, settings)."""
    if len(channels) != len(channel_names):
        raise ValueError("one name per channel")
    eng = eng or get_engine()
    out: list = []
    for a in range(0, len(channels), MAX_BATCH_CHANNELS):
        chans = [np.asarray(c, dtype=np.float32).reshape(-1) for c in channels[a : a + MAX_BATCH_CHANNELS]]
        batch = eng.upload(chans)
        out += results_of_batch(eng, batch, sample_rate_hz, channel_names[a : a + MAX_BATCH_CHANNELS], settings)
    return out


def file_channels(paths: Iterable[str | Path], use_mono_downmix_for_stereo: bool,
                  expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ) -> Iterator[Tuple[str, np.ndarray]]:
    """(name, channel) of every channel of every WAV file (mono or stereo, rate checked), named
    "<file name>:<channel>" with the channel names of get_analysis_channels ("mono", "left", "right")."""
    for p in paths:
        _, cs = wav_channels(p, use_mono_downmix_for_stereo, expected_sample_rate_hz=expected_sample_rate_hz)
        for n, c in cs:
            yield f"{Path(p).name}:{n}", c


def bundle_groups(bundle_root: str | Path, use_mono_downmix_for_stereo: bool,
                  expected_sample_rate_hz: int = DEFAULT_EXPECTED_SAMPLE_RATE_HZ, eng=None):
    """(group, batch, labels) for the taps a bundle's meta.json lists (taps/<name>.wav), read by the native ingest
    (ingest.TapSet) a group at a time: group = the tap names (at most MAX_BATCH_CHANNELS // 2 of them, a tap has one or
    two channels), batch = their channels on the device, labels = per channel (index into group, channel name)."""
    from ..ingest import TapSet

    root = Path(bundle_root)
    taps: List[str] = list(json.loads((root / "meta.json").read_text()).get("taps", []))
    eng = eng or get_engine()
    step = MAX_BATCH_CHANNELS // 2
    for a in range(0, len(taps), step):
        group = taps[a : a + step]
        ts = TapSet(eng, [root / "taps" / f"{t}.wav" for t in group], expected_sample_rate_hz)
        batch, labels = ts.view(use_mono_downmix_for_stereo)
        yield group, batch, labels


def analyse_wav_file_channels(path: str | Path, settings, expected_sample_rate_hz: int, analyse_batch: Callable) -> list:
    """One WAV file through analyse_batch(channels, the file's sample rate, names, settings); channels named as by
    get_analysis_channels ("mono", "left", "right")."""
    loaded, chans = wav_channels(path, settings.use_mono_downmix_for_stereo, expected_sample_rate_hz=expected_sample_rate_hz)
    return analyse_batch([c for _, c in chans], loaded.sample_rate_hz, [n for n, _ in chans], settings)


def analyse_file_channels(paths: Sequence[str | Path], settings, expected_sample_rate_hz: int, analyse_batch: Callable) -> list:
    """Every channel of every file (file_channels) through analyse_batch(channels, sample_rate_hz, names, settings)."""
    named = list(file_channels(paths, settings.use_mono_downmix_for_stereo, expected_sample_rate_hz))
    return analyse_batch([c for _, c in named], int(expected_sample_rate_hz), [n for n, _ in named], settings)


def analyse_bundle_channels(bundle_root: str | Path, settings, expected_sample_rate_hz: int, results_of_batch: Callable,
                            eng=None) -> list:
    """Every channel of every tap of a bundle (bundle_groups) through results_of_batch; channels named "<tap>:<channel>"."""
    out: list = []
    for group, batch, labels in bundle_groups(bundle_root, settings.use_mono_downmix_for_stereo, expected_sample_rate_hz, eng):
        names = [f"{group[i]}:{ch}" for i, ch in labels]
        out += results_of_batch(eng or get_engine(), batch, int(expected_sample_rate_hz), names, settings)
    return out


# ---------------------------------------------------------------------------------------------------
# text, Markdown, JSON
# ---------------------------------------------------------------------------------------------------


def status_text(status: int, words: Sequence[Tuple[int, str]]) -> str:
    """"ok", or the flags and the words of the bits that are set: "6 (too short, non-finite)"."""
    if status == 0:
        return "ok"
    return f"{status} (" + ", ".join(w for bit, w in words if status & bit) + ")"


def fmt(v: float, digits: int = 3) -> str:
    """A cell: NaN is "NA", an infinity "+inf" / "-inf" (only a clarity can be one: every other measure's values are
    finite or NaN)."""
    if math.isnan(v):
        return "NA"
    if math.isinf(v):
        return "+inf" if v > 0 else "-inf"
    return f"{v:.{digits}f}"


def json_num(v: float):
    """Plain JSON: NaN is null, an infinity the string "+inf" / "-inf"."""
    if math.isnan(v):
        return None
    if math.isinf(v):
        return "+inf" if v > 0 else "-inf"
    return float(v)


def num_json(v) -> float:
    return float("nan") if v is None else float(v)          # float("+inf") parses an infinity


def band_to_json(b: BandDefinition, values: Dict) -> Dict:
    return dict(name=b.name, centre_hz=b.centre_hz, kind=b.kind, low_edge_hz=b.low_edge_hz, high_edge_hz=b.high_edge_hz,
                **values)


def bands_from_json(rows: Sequence[Dict]) -> List[BandDefinition]:
    return [BandDefinition(b["name"], b["centre_hz"], b["kind"], b["low_edge_hz"], b["high_edge_hz"]) for b in rows]


def band_rows(r, values_by_name: Dict) -> List[Tuple[str, object]]:
    """("Broadband", r.broadband), then (band name, its values) per band of r, ascending."""
    return [("Broadband", r.broadband)] + [(b.name, values_by_name[b.name]) for b in r.band_definitions]


def text_block(name: str, head: str, columns: Sequence[str], rows: Iterable[Sequence[str]],
               tail: Sequence[str] = (), first: str = "Band") -> List[str]:
    """The lines of one block of a text summary: [name], the head line, the column row, a row of cells per row (cells
    separated by two spaces), the tail lines and an empty line.  first: the heading of the rows' first cell."""
    return [f"[{name}]", head, "  ".join([first, *columns])] + ["  ".join(cells) for cells in rows] + [*tail, ""]


def markdown_block(name: str, head: str, columns: Sequence[str], rows: Iterable[Sequence[str]],
                   tail: Sequence[str] = (), first: str = "Band") -> List[str]:
    """The lines of one section of a Markdown summary: '### name', the head line, a table with a right-aligned column per
    entry of columns, and the tail lines, each part followed by an empty line.  first: the heading of the rows' first cell."""
    table = [f"| {first} | " + " | ".join(columns) + " |", "|---|" + "---:|" * len(columns)]
    table += ["| " + " | ".join(cells) + " |" for cells in rows]
    return [f"### {name}", "", head, "", *table, ""] + [line for t in tail for line in (t, "")]


def join_blocks(blocks: Iterable[List[str]]) -> str:
    lines = [line for block in blocks for line in block]
    return "\n".join(lines) + ("\n" if lines else "")


# ---------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------


def add_source_arguments(p, input_help: str = "WAV files (every channel of every file is analysed)", mono: bool = True) -> None:
    """--input | --bundle and, for the per-channel measures, --mono: the first arguments of a measure's parser."""
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--input", nargs="+", type=Path, help=input_help)
    src.add_argument("--bundle", type=Path, help="bundle directory: meta.json + taps/<name>.wav")
    if mono:
        p.add_argument("--mono", action="store_true", help="analyse stereo files as their mono downmix 0.5 * (L + R)")


def add_bands_argument(p) -> None:
    p.add_argument("--bands", choices=["none", *BAND_MODES], default="octave", help="filter bank (default: octave)")


def add_output_arguments(p) -> None:
    """--expected-sample-rate and --json: the last arguments of a measure's parser (the help lists arguments in the order
    they were added, the measure's own lie between the source and these)."""
    p.add_argument("--expected-sample-rate", type=int, default=DEFAULT_EXPECTED_SAMPLE_RATE_HZ,
                   help="every file must have this sample rate (default: 48000)")
    p.add_argument("--json", type=Path, default=None, help="also write the results as JSON to this file")


def run_cli(parser, argv: Optional[Sequence[str]], settings_from_args: Callable, run_files: Callable, run_bundle: Callable,
            to_text: Callable, to_json: Callable) -> None:
    """Parse; a ValueError from the settings is a usage error; analyse the files or the bundle; write the text summary to
    stdout and, with --json, the JSON document to that file."""
    args = parser.parse_args(argv)
    try:
        settings = settings_from_args(args)
    except ValueError as e:
        parser.error(str(e))
    if args.input:
        results = run_files(args.input, settings, args.expected_sample_rate)
    else:
        results = run_bundle(args.bundle, settings, args.expected_sample_rate)
    sys.stdout.write(to_text(results))
    sys.stdout.flush()
    if args.json is not None:
        args.json.write_text(json.dumps(to_json(results), indent=2) + "\n")
