#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the device assembly of two checkouts: for a refactor that must not change the kernels.

    python3 tools/isa_compare.py <checkout A> <checkout B> [--tuning] [file.hip ...]      (default: every file of build.SOURCES)

Each file is compiled in both checkouts with the flags build.py uses for it (build.COMMON + build.SOURCES[file], from the
checkout this tool lives in) plus --cuda-device-only -S.  Per kernel: identical or not -- instruction lines only; comment
lines, assembler directives, labels and with them the per-compilation __hip_cuid_* symbol are ignored -- then VGPR, SGPR,
scratch bytes and instruction counts by class, as "A -> B" where they differ.  A kernel that differs but executes the same
number of every opcode is marked "same opcodes": the two differ in instruction order and register numbers only.
A kernel is looked up in A by its symbol among ALL the files given, so one that moved to another file (or to a new one, which
A does not have) is compared with the kernel it was: name both the file it left and the file it went to."""
import collections, re, shutil, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from audio_analysis_amd import build  # noqa: E402

CLASSES = ("VALU", "SALU", "SMEM", "LDS", "VMEM", "s_waitcnt", "s_barrier")


def classify(op):
    if op.startswith("v_"): return "VALU"
    if op.startswith("ds_"): return "LDS"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")): return "VMEM"
    if op.startswith("s_waitcnt"): return "s_waitcnt"
    if op.startswith("s_barrier"): return "s_barrier"
    if op.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime", "s_dcache")): return "SMEM"
    if op.startswith("s_"): return "SALU"
    return "other"


def assembly(root, name, tuning, tmp):
    if not (Path(root) / "audio_analysis_amd" / "csrc" / name).exists():      # a file only the other checkout has
        return ""
    out = Path(tmp) / f"{Path(root).name}_{abs(hash(str(root)))}_{Path(name).stem}.s"
    cmd = [build._hipcc(), *build.COMMON, *(["-DIRA_TUNING_BUILD"] if tuning else []), *build.SOURCES[name],
           "--cuda-device-only", "-S", str(Path(root) / "audio_analysis_amd" / "csrc" / name), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"hipcc failed:\n{' '.join(cmd)}\n{r.stderr}")
    return out.read_text()


def kernels(text):
    """{kernel symbol: (instruction lines, {vgpr, sgpr, scratch})} of one assembly file."""
    found = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M):
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:(.*?)^; Occupancy" % re.escape(name), text, flags=re.S | re.M)
        body, tail = m.group(1), m.group(2)
        ins = []
        for line in body.splitlines():
            line = line.split(";")[0].strip()
            if line and not line.startswith(".") and not line.endswith(":"):
                ins.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(line.split())))   # branch targets carry the function's
                                                                                    # position in its file: not the kernel's own
        res = {key: int(re.search(r";\s*%s:\s*(\d+)" % tag, tail).group(1))
               for key, tag in (("VGPR", "NumVgprs"), ("SGPR", "TotalNumSgprs"), ("scratch", "ScratchSize"))}
        found[name] = (ins, res)
    return found


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not names or not filt:
        return {n: n for n in names}
    out = subprocess.run([filt, *names], capture_output=True, text=True).stdout.split("\n")
    # "void (anonymous namespace)::kern<1, true>(args...)" -> "kern<1, true>"
    short = [re.sub(r"^void ", "", re.sub(r"\((?!anonymous).*$", "", d)).replace("(anonymous namespace)::", "") for d in out]
    return dict(zip(names, short))


def main():
    args = [a for a in sys.argv[1:] if a != "--tuning"]
    tuning = "--tuning" in sys.argv
    if len(args) < 2:
        raise SystemExit(__doc__)
    roots, files = args[:2], args[2:] or list(build.SOURCES)
    same = differ = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=8) as ex:
        texts = list(ex.map(lambda rf: assembly(rf[0], rf[1], tuning, tmp), [(r, f) for f in files for r in roots]))
    print(f"A = {roots[0]}   B = {roots[1]}   flags: {' '.join(build.COMMON)}{' -DIRA_TUNING_BUILD' if tuning else ''} + per file")
    per_file = [(kernels(texts[2 * i]), kernels(texts[2 * i + 1])) for i in range(len(files))]
    in_a = {sym: (f, k) for f, (a, _) in zip(files, per_file) for sym, k in a.items()}      # symbol -> (A's file, kernel)
    in_b = {sym for _, b in per_file for sym in b}
    for f, (a, b) in zip(files, per_file):
        names = demangle(sorted({s for s in a if s not in in_b} | set(b)))
        print(f"== {f}  {' '.join(build.SOURCES[f])}")
        for sym, name in names.items():
            if sym not in in_a or sym not in b:
                print(f"   {name}: only in {'A' if sym in a else 'B'}")
                differ += 1
                continue
            (fa, (ia, ra)), (ib, rb) = in_a[sym], b[sym]
            if fa != f:
                name += f" (A: {fa})"
            ident = ia == ib
            same, differ = same + ident, differ + (not ident)
            ca, cb = (collections.Counter(classify(l.split()[0]) for l in x) for x in (ia, ib))
            cols = [(k, ra[k], rb[k]) for k in ("VGPR", "SGPR", "scratch")] + [("instructions", len(ia), len(ib))]
            cols += [(k, ca[k], cb[k]) for k in CLASSES + (("other",) if ca["other"] or cb["other"] else ())]
            same_opcodes = collections.Counter(l.split()[0] for l in ia) == collections.Counter(l.split()[0] for l in ib)
            print(f"   {name}: {'identical' if ident else 'DIFFERENT (same opcodes)' if same_opcodes else 'DIFFERENT'}")
            print("      " + "  ".join(f"{k} {x}" if x == y else f"{k} {x} -> {y}" for k, x, y in cols))
    print(f"{same} kernels identical, {differ} different")


if __name__ == "__main__":
    main()
