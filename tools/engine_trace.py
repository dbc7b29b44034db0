#!/usr/bin/env python3
"""Host trace of the measure launchers of one checkout, or of two compared: for a refactor of engine.py that must not
change what reaches the library.  No GPU: the checkout's tests/host_engine.py records every library call.

    python3 tools/engine_trace.py <checkout>                   the trace of a fixed corpus as JSON, one step per line
    python3 tools/engine_trace.py <checkout A> <checkout B>    both traces compared step by step: counts, then "equal" or
                                                               the steps that differ

A checkout needs its libira.so built.  Its trace is made in a subprocess with that checkout (and its tests/) on PYTHONPATH,
by the corpus of THIS file.  A step is one launcher call or one analyse.*_device call on a fresh HostEngine per group; its
events are the engine's record (every call with its scalars, table digests and allocation sizes, every fetch) and the
number of uploads it made.  The host-only sizers are passed through to the library in both checkouts (SIZERS: older
copies of host_engine.py answered some of them with 0), and tables of address differences take fixed values (trace())."""
import collections, json, os, subprocess, sys
from pathlib import Path

SIZERS = {"ira_energy_scratch_doubles", "ira_xcorr_scratch_doubles", "ira_lundeby_scratch_doubles", "ira_mtf_scratch_doubles",
          "ira_echo_scratch_doubles", "ira_fdw_scratch_doubles", "ira_burst_table_doubles"}
LENGTHS = ([], [3000], [3000, 1700, 2400])             # no channel, one, three of unequal length
GRID = ([0.25, 0.1, 0.01], [127, 128, 5000])           # the last narrow point, the first wide one, a second chunk


def launcher_steps(HostEngine, np, lens):
    """(name, thunk) of every measure launcher on one engine and batch; a thunk's result may feed the steps after it."""
    eng = HostEngine()
    t, rng, n = eng.torch, np.random.default_rng(len(lens)), len(lens)
    b = eng.upload([rng.standard_normal(m).astype(np.float32) for m in lens])
    rows, idx, keep = np.arange(n, dtype=np.int32), np.arange(n), {}
    limits = np.tile(np.array([240, 3840], dtype=np.int64), (n, 1))
    echo_params = np.array([[2.0 / 3.0, 432, 10, 2000, 48, 1.0, 1.8, 48000.0]])
    spec_total = n * 2049

    def step(name, fn, key=None):
        def run():
            out = fn()
            if key:
                keep[key] = out
        return name, run

    steps = [step("onset_index", lambda: eng.onset_index(b, 1e-4), "onset"),
             step("energy_windows", lambda: eng.energy_windows(b.x, b.off, b.length, rows, keep["onset"][0], limits))]
    for stash in (False, True):
        def echo(stash=stash):
            eng.echo_stash = stash
            try:
                return eng.echo_criterion(b.x, b.off, b.length, rows, keep["onset"][0], echo_params, np.zeros(n, np.int32))
            finally:
                eng.echo_stash = False
        steps.append(step(f"echo_criterion stash={stash}", echo))
    steps += [step("echo_density", lambda: eng.echo_density(b.x, b.off, b.length, keep["onset"][0], np.ones(21), 10, 5, 1000, [1.0])),
              step("reflections", lambda: eng.reflections(b.x, b.off, b.length, keep["onset"][0], np.hanning(11)[1:-1] + 0.5, 4, 48,
                                                          24, 20, 10, 100, 1000, 0.01, 2.0, 8))]
    for window in ("hann", "rect"):
        for rho, half in (([], []), GRID):
            tag = f"{window} J={len(rho)}"
            steps.append(step(f"fdw_response {tag}", lambda rho=rho, half=half, window=window: eng.fdw_response(
                b.x, b.off, b.length, keep["onset"][1], np.array(rho), np.array(half), window)))
            steps.append(step(f"burst_table {tag}", lambda rho=rho, half=half, window=window: eng.burst_table(
                np.array(rho), np.array(half), window), "table"))
            for nsteps in (0, 1, 9):
                steps.append(step(f"burst_decay {tag} M={nsteps}", lambda rho=rho, nsteps=nsteps: eng.burst_decay(
                    b.x, b.off, b.length, keep["onset"][1], keep["table"],
                    np.tile(np.arange(nsteps) * 7 - 3, (len(rho), 1)).reshape(len(rho), nsteps))))
    for nf in (32, 4096):
        n_fft, spec_off = np.full(n, nf), np.arange(n, dtype=np.int64) * (nf // 2 + 1)
        spec = eng.empty(2 * n * (nf // 2 + 1), t.float64)
        bins = np.tile(np.array([1, 5, nf // 2 - 1]), (n, 1))
        steps += [step(f"minphase_logmag N={nf}", lambda spec=spec, so=spec_off, nn=n_fft: eng.minphase_logmag(spec, so, nn, -120.0), "mp"),
                  step(f"minphase_excess N={nf}", lambda spec=spec, so=spec_off, nn=n_fft: eng.minphase_excess(
                      spec, keep["mp"][0], so, nn, np.zeros(n, np.int64), keep["mp"][1]), "ex"),
                  step(f"minphase_gather N={nf}", lambda spec=spec, so=spec_off, nn=n_fft, bins=bins: eng.minphase_gather(
                      spec, keep["mp"][0], keep["ex"], so, nn, bins, keep["mp"][1])),
                  step(f"minphase_spectrum N={nf}", lambda so=spec_off, nn=n_fft: eng.minphase_spectrum(
                      keep["mp"][0], keep["mp"][0], so, nn, keep["mp"][1]))]
    spec = eng.empty(2 * spec_total, t.float64)
    lo, cnt = np.array([[1, 10, 100], [2, 20, 200]], np.int32), np.array([[4, 0, 50], [8, 16, 1]], np.int32)
    blk = np.full(n, 480, np.int32)
    jobs3 = np.stack([idx, np.zeros(n, int), idx], axis=1)
    jobs4 = np.stack([idx, np.ones(n, int), idx, np.zeros(n, int)], axis=1)
    grid, grid_n = eng.empty(16, t.float64), eng.empty(1, t.int32)
    steps += [
        step("cross_spectra", lambda: eng.cross_spectra(b.x, b.off, b.off, b.length, 256, 128, True)),
        step("xcorr_windows", lambda: eng.xcorr_windows(b.x, b.off, b.off, b.length, rows, rows, keep["onset"][0], limits, 48)),
        step("mtf_sums", lambda: eng.mtf_sums(b.x, b.off, b.length, np.tile(np.linspace(0.0, 0.5, 14), (n, 1)))),
        step("harmonic_peaks", lambda: eng.harmonic_peaks(b.x, b.off, b.length), "hpk"),
        step("harmonic_windows", lambda: eng.harmonic_windows(b.x, b.off, b.length, keep["hpk"][0], np.array([100, 200]), 8, np.hanning(64))),
        step("harmonic_band_powers", lambda: eng.harmonic_band_powers(spec, np.arange(2 * n, dtype=np.int64) * 1024, lo, cnt, 1024)),
        step("lundeby_rows", lambda: eng.lundeby_rows(b.off, b.length, rows, blk, b.length // 480, np.ones(n, np.int32)), "rows"),
        step("block_energy", lambda: eng.block_energy(b.x, keep["rows"], keep["onset"][0]), "blk"),
        step("lundeby_estimate", lambda: eng.lundeby_estimate(keep["rows"], keep["onset"][0], keep["blk"]), "lun"),
        step("edc_truncated", lambda: eng.edc_truncated(b.x, keep["rows"], keep["onset"][0], *keep["lun"], 1e-12, -120.0,
                                                        eng.empty(sum(lens), t.float32), b.off)),
        step("multislope_points", lambda: eng.multislope_points(keep["rows"], keep["onset"][0], keep["blk"], 0.9), "msp"),
        step("multislope_gram", lambda: eng.multislope_gram(keep["rows"], keep["onset"][0], keep["msp"][0], keep["msp"][1], jobs3, grid,
                                                            grid_n, 16, 1, 16, 48000.0, max(n, 1)), "gram"),
        step("multislope_search refine", lambda: eng.multislope_search(n, keep["msp"][1], jobs4, grid, grid_n, 16, 1, 16, keep["gram"],
                                                                       max(n, 1), 1.5, keep["msp"][2], 0.1)),
        step("multislope_search", lambda: eng.multislope_search(n, keep["msp"][1], jobs4, grid, grid_n, 16, 1, 16, keep["gram"],
                                                                max(n, 1), 1.5, keep["msp"][2])),
        step("tail_energy", lambda: eng.tail_energy(b.x, b.off, b.off + b.length)),
        step("tail_table", lambda: eng.tail_table(b, np.zeros(n, np.int64))),
        step("tail_table again", lambda: eng.tail_table(b, np.zeros(n, np.int64)))]
    return eng, steps


def analyse_steps(HostEngine, np):
    """(name, thunk) of every analyse.*_device function of the measure modules on one two-channel batch, default settings."""
    from audio_analysis_amd import analyse as A
    from audio_analysis_amd.analyse import (burstdecay, echo, echodensity, energy, fdw, harmonics, iacc, lundeby, minphase,  # noqa: F401
                                            multislope, reflections, sti, transfer)
    from audio_analysis_amd.synth import synth_ir
    eng, sr = HostEngine(), 48000
    b = eng.upload([synth_ir(0, 0, 48000, sr), synth_ir(1, 0, 48000, sr)])      # (equal lengths: a stereo pair)
    k = np.arange(16384)
    sweep = np.sin(2 * np.pi * 20.0 * 16384 / sr / np.log(400.0) * (np.exp(k / 16384 * np.log(400.0)) - 1.0)).astype(np.float32)
    steps = [(f"analyse.{mod}.{fn}", lambda mod=mod, fn=fn: getattr(getattr(A, mod), fn)(eng, b, sr)) for mod, fn in (
        ("energy", "energy_parameters_device"), ("lundeby", "lundeby_device"), ("multislope", "multislope_device"),
        ("sti", "sti_device"), ("echo", "echo_criterion_device"), ("echodensity", "echo_density_device"),
        ("reflections", "reflections_device"), ("fdw", "fdw_device"), ("burstdecay", "burst_decay_device"),
        ("minphase", "minphase_device"), ("minphase", "minimum_phase_device"))]
    steps += [("analyse.iacc.iacc_device", lambda: A.iacc.iacc_device(eng, b, [(0, 1)], sr)),
              ("analyse.transfer.transfer_device", lambda: A.transfer.transfer_device(eng, b, [0], [1], sr)),
              ("analyse.harmonics.harmonic_distortion_device", lambda: A.harmonics.harmonic_distortion_device(
                  eng, b, [0, 0], eng.upload([sweep]), [0, 0], sr))]
    return eng, steps


def trace():
    """This interpreter's checkout (PYTHONPATH): one JSON line per step."""
    import numpy as np
    import host_engine
    host_engine.HOST_ONLY |= SIZERS
    from audio_analysis_amd.analyse import _common
    # Launches that read several buffers address them from one base (band_row_offsets): their tables hold differences of
    # unrelated addresses, other ones in every run.  The trace takes fixed ones instead: buffer k lies k * 2^32 elements on.
    _common.common_base = lambda tensors: (tensors[0], [k << 32 for k in range(len(tensors))])
    groups = [(f"{len(lens)}ch ", launcher_steps(host_engine.HostEngine, np, lens)) for lens in LENGTHS]
    groups.append(("", analyse_steps(host_engine.HostEngine, np)))
    for prefix, (eng, steps) in groups:
        for name, run in steps:
            first, uploads = len(eng.record), eng.uploads
            run()
            print(json.dumps({"step": prefix + name, "uploads": eng.uploads - uploads, "events": eng.record[first:]}))


def trace_of(checkout):
    root = str(Path(checkout).resolve())
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests")]))
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--trace"], cwd=root, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"the trace of {checkout} failed:\n{r.stderr}")
    return r.stdout.splitlines()


def main():
    if sys.argv[1:] == ["--trace"]:
        return trace()
    if len(sys.argv) == 2:
        return print("\n".join(trace_of(sys.argv[1])))
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    a, b = (trace_of(c) for c in sys.argv[1:3])
    steps = [json.loads(line) for line in a]
    calls, uploads = collections.Counter(), collections.Counter()
    for s in steps:
        names = [e[1].split("[")[0] for e in s["events"] if e[0] == "call"]
        calls.update(names)
        uploads[s["step"].split(" ")[-1] if s["step"].startswith("analyse.") else s["step"].split(" ")[1]] += s["uploads"]
    print(f"{len(steps)} steps, {sum(calls.values())} library calls, {sum(s['uploads'] for s in steps)} uploads, "
          f"{sum(e[0] == 'fetch' for s in steps for e in s['events'])} fetches (checkout A)")
    print("library calls per entry point:")
    for name, k in sorted(calls.items()):
        print(f"   {name}: {k}")
    print("uploads per launcher / analyse function (all its steps):")
    for name, k in sorted(uploads.items()):
        print(f"   {name}: {k}")
    differ = [(json.loads(x)["step"] if x else None, json.loads(y)["step"] if y else None)
              for x, y in zip(a + [""] * (len(b) - len(a)), b + [""] * (len(a) - len(b))) if x != y]
    print("equal" if not differ else f"{len(differ)} steps DIFFER (A, B): {differ}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
