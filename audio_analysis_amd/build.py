"""
Build libira.so (hand-written HIP kernels + C-ABI) in-tree for gfx950 with hipcc.

    python -m audio_analysis_amd.build            # incremental
    python -m audio_analysis_amd.build --force

hipcc cross-compiles without a GPU.  The shared object lands next to the sources
(audio_analysis_amd/csrc/libira.so) so it travels with the repo snapshot to the GPU box.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

CSRC = Path(__file__).resolve().parent / "csrc"
LIB = CSRC / "libira.so"
ARCH = "gfx950"

# per-file extra flags; -ffp-contract=off where f64 arithmetic must round like NumPy's (no FMA fusion)
SOURCES = {
    "ira_api.hip": [],
    "ira_edc.hip": ["-ffp-contract=off"],
    # -fno-slp-vectorize: hipcc otherwise packs the complex arithmetic into v_pk_{add,mul,fma}_f32.  Measured with
    # tools/pk_f32_rate.hip on MI355X: a packed op occupies the SIMD twice as long as a scalar one (0.87 vs 1.5
    # wave-instructions per CU-cycle at saturation) and the packing itself costs register moves.
    "ira_stft.hip": ["-fno-slp-vectorize"],
    "ira_stft2.hip": ["-fno-slp-vectorize"],
    "ira_stft3.hip": ["-fno-slp-vectorize"],
    "ira_stft4.hip": [],
    # suffix energies: exact float32 squares added by explicit fma in a fixed order, nothing for contraction to change
    "ira_tailenergy.hip": [],
    "ira_fftlong.hip": [],
    "ira_fftsmooth.hip": [],
    "ira_spectrum.hip": ["-ffp-contract=off"],
    "ira_modal.hip": ["-ffp-contract=off"],
    "ira_ar.hip": [],
    "ira_roots.hip": [],
    "ira_ingest.hip": ["-ffp-contract=off"],
    "ira_deconv.hip": ["-ffp-contract=off"],
    # float32 arithmetic of the reference is reproduced operation by operation: no FMA contraction
    "ira_diffusion.hip": ["-ffp-contract=off"],
    # float64 energy products and sums round one operation at a time, like NumPy's
    "ira_energy.hip": ["-ffp-contract=off"],
    # float64 lag sums of exact float32 products (explicit fma there rounds like multiply-then-add)
    "ira_xcorr.hip": ["-ffp-contract=off"],
    # float64 block energies, regression sums and suffix sums round one operation at a time
    "ira_lundeby.hip": ["-ffp-contract=off"],
    # multi-slope fits: sums and solves are compared with a long-double restatement that rounds one operation at a time, and
    # the search's argmin must not depend on what the optimiser fused; the Gram sums call fma themselves
    "ira_multislope.hip": ["-ffp-contract=off"],
    # modulation transfer sums: compared only with themselves and to 1e-10 with a long-double restatement; FMAs wanted
    "ira_mtf.hip": [],
    # a harmonic segment sample is one float64 product rounded once to float32, bit for bit NumPy's
    "ira_harmonics.hip": ["-ffp-contract=off"],
    # float64 running sums of |p|^n and their ratios round one operation at a time, like NumPy's
    "ira_echo.hip": ["-ffp-contract=off"],
    # float64 window sums w h2 and the comparison h2 A > B round one operation at a time, like the restatement's
    "ira_echodensity.hip": ["-ffp-contract=off"],
    # float64 envelope and background sums round one operation at a time: compared bit for bit with the NumPy restatement
    "ira_reflections.hip": ["-ffp-contract=off"],
    # cross-spectral sums are compared to a derived bound only (FMAs wanted in the transform); the finish kernel, whose
    # quotients are held to a few ulp, turns contraction off for itself
    "ira_xspec.hip": [],
    # the turn count k rho is reduced from its rounded product and that product's error, which a contraction would merge;
    # the sums call fma themselves and are held to a derived bound, not to bits
    "ira_fdw.hip": ["-ffp-contract=off"],
    # the wavelet table repeats ira_fdw.hip's weight and phasor term for term (the same split of k rho); the map's sums
    # call fma themselves
    "ira_burstdecay.hip": ["-ffp-contract=off"],
    # |X|^2 = re * re + im * im and the phase wrap d - 2 pi rint(d / 2 pi) round one operation at a time, like NumPy's
    "ira_minphase.hip": ["-ffp-contract=off"],
    # the residual (x - Y / R)^2 and the response (W - W[0]) / scale round one operation at a time: the chain is held bit for
    # bit to a NumPy restatement (the transform itself has only additions and subtractions, nothing to contract)
    "ira_mls.hip": ["-ffp-contract=off"],
    # power sums, the pyramid's pairwise sums, the window sums and the quotients of the inversion round one operation at a
    # time: every kernel is held bit for bit to a NumPy restatement
    "ira_equalise.hip": ["-ffp-contract=off"],
    # the row sums, the suffix sums of the backward integration and the noise subtraction round one operation at a time:
    # the integration is held bit for bit to a NumPy restatement (the transform calls fma itself where it wants one)
    "ira_edr.hip": ["-ffp-contract=off"],
}
COMMON = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function"]


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(exe).exists():
        raise RuntimeError("hipcc not found; libira cannot be built")
    return exe


def _stale(obj: Path, deps) -> bool:
    if not obj.exists():
        return True
    t = obj.stat().st_mtime
    return any(Path(d).stat().st_mtime > t for d in deps)


def build_tuning(verbose: bool = True) -> Path:
    """The TUNING build: the same sources with -DIRA_TUNING_BUILD, i.e. with the IRA_* environment knobs (ablations, tile
    and radix overrides, A/B kernel selection) compiled in -> csrc/libira_tuning.so.  Never loaded by the product; set
    IRA_TUNING=1 and point IRA_LIBRARY at it to profile (audio_analysis_amd._lib honours the pair for this purpose only and
    checks its ABI version like the product library's)."""
    hipcc = _hipcc()
    objs = []
    out = CSRC / "libira_tuning.so"
    tmp = CSRC / "_tuning"
    tmp.mkdir(exist_ok=True)
    cmds = []
    for name, extra in SOURCES.items():
        obj = tmp / (Path(name).stem + ".o")
        cmds.append([hipcc, *COMMON, "-DIRA_TUNING_BUILD", *extra, "-c", str(CSRC / name), "-o", str(obj)])
        objs.append(obj)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, cmds))
    subprocess.run([hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", *map(str, objs), "-o", str(out)], check=True)
    return out


def build(force: bool = False, verbose: bool = False) -> Path:
    hipcc = _hipcc()
    headers = list(CSRC.glob("*.h")) + [CSRC.parent.parent / "include" / h for h in ("ira.h", "ira_equalise.h", "ira_edr.h")]
    jobs = []
    objs = []
    for name, extra in SOURCES.items():
        src = CSRC / name
        obj = CSRC / (src.stem + ".o")
        objs.append(obj)
        if force or _stale(obj, [src, Path(__file__)] + headers):
            jobs.append([hipcc, *COMMON, *extra, "-c", str(src), "-o", str(obj)])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
        if verbose and r.stderr.strip():
            print(r.stderr, flush=True)

    if jobs:
        with ThreadPoolExecutor(max_workers=min(4, len(jobs))) as ex:
            list(ex.map(run, jobs))
    if jobs or force or _stale(LIB, objs):
        run([hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", *map(str, objs), "-o", str(LIB)])
    return LIB


if __name__ == "__main__":
    if "--tuning" in sys.argv:
        print(build_tuning())
        sys.exit(0)
    p = build(force="--force" in sys.argv, verbose=True)
    print(p)
