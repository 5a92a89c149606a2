"""Per-kernel comparison of two device assembly listings of one source file (see isa_count.py for
the compile line): which kernels are byte-identical, and the resources of those that are not.

    python benchmarks/isa_diff.py before.s after.s [--fold 'ffm_pipe_kernel<(\\d), true>=ffm_pipe_kernel<\\1>']

A kernel is its code from ``<symbol>:`` to ``.Lfunc_end`` plus its ``.amdhsa_kernel`` block, with the
compiler-numbered local labels normalised (their function index shifts when instantiations go).
Kernels are paired by demangled name; ``--fold 'regex=replacement'`` rewrites the names of the
first listing first (a folded template parameter).  A record for docs/perf_notes.md, not a test."""
import re
import subprocess
import sys

KEYS = ("NumVgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")
SPILLS = ("vgpr_spill_count", "sgpr_spill_count")     # in the kernel's .amdgpu_metadata entry


def kernels(path):
    text = open(path).read()
    syms = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    names = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for sym, name in zip(syms, names):
        body = text[text.index("\n" + sym + ":"):]
        tail = body[body.index(".Lfunc_end"):]
        body = body[:body.index(".Lfunc_end")] + tail[:tail.index("\n")]
        desc = text[text.index(".amdhsa_kernel " + sym):]
        code = (body + desc[:desc.index(".end_amdhsa_kernel")]).replace(sym, "SYM")
        code = re.sub(r"\.(LBB|Lfunc_end|Ltmp)\d+", r".\1", re.sub(r"[ \t]*;.*", "", code))   # comments name BB<n>_ too
        meta = {k: re.search(r"; " + k + r":\s*(\S+)", tail).group(1) for k in KEYS}
        entry = text[:text.index(".symbol:         " + sym + ".kd")].rsplit("\n  - .", 1)[1]
        entry += text[text.index(".symbol:         " + sym + ".kd"):].split("\n  - .", 1)[0]
        meta.update({k: re.search(k + r":\s*(\d+)", entry).group(1) for k in SPILLS})
        meta["insts"] = sum(1 for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith((".", ";")))
        out[name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]] = (code, meta)
    return out


argv = sys.argv[1:]
folds = [argv[i + 1].split("=", 1) for i, a in enumerate(argv) if a == "--fold"]
paths = [a for i, a in enumerate(argv) if a != "--fold" and (i == 0 or argv[i - 1] != "--fold")]
before, after = kernels(paths[0]), kernels(paths[1])
for pat, rep in folds:
    before = {re.sub(pat, rep, k): v for k, v in before.items()}
same = [k for k in after if k in before and before[k][0] == after[k][0]]
print(f"kernels: {len(before)} -> {len(after)}; identical {len(same)}; gone {len(set(before) - set(after))}; "
      f"new {sorted(set(after) - set(before))}")
for k in sorted(after):
    if k in before and k not in same:
        print(k)
        print("  " + "  ".join(f"{key} {before[k][1][key]}->{after[k][1][key]}" for key in KEYS + SPILLS + ("insts",)))
