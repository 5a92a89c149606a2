"""Static instruction counts of one kernel in a device assembly listing
(``hipcc <the flags of hivemall_amd/_build.py> --cuda-device-only -S csrc/kernels/ffm.hip -o ffm.s``):
the whole function, and the span of its backward branches that enclose a barrier (the row loop
of the pipelined FFM kernels, as far as the block layout keeps it contiguous).

    python benchmarks/isa_count.py ffm.s <mangled kernel name> [file to write the loop to]

A record for docs/perf_notes.md (round 7), not a test."""
import re
import sys

path, sym = sys.argv[1], sys.argv[2]
lines = open(path).read().split("\n")
start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
body = lines[start:end + 1]
labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
lo, hi = 1 << 30, 0
# the prologue's first barrier is outside the row loop: a backward branch over it is a cold block
# laid out behind the function that jumps back into the prologue (the side table's gated publish)
first_bar = next((i for i, l in enumerate(body) if "s_barrier" in l), 1 << 30)
for i, l in enumerate(body):
    m = re.search(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", l)
    if m and labels.get(m.group(1), 1 << 30) < i:
        t = labels[m.group(1)]
        if t > first_bar and any("s_barrier" in x for x in body[t:i]):
            lo, hi = min(lo, t), max(hi, i)
loop = body[lo:hi + 1]
if len(sys.argv) > 3:
    open(sys.argv[3], "w").write("\n".join(loop))


def count(seg):
    ins = [l.split()[0] for l in seg if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    c = lambda pred: sum(1 for x in ins if pred(x))
    return {
        "insts": len(ins),
        "v_readlane": c(lambda x: x.startswith("v_readlane")),
        "v_writelane": c(lambda x: x.startswith("v_writelane")),
        "v_readfirstlane": c(lambda x: x.startswith("v_readfirstlane")),
        "s_nop": c(lambda x: x == "s_nop"),
        "v_mul_lo_u32": c(lambda x: x.startswith("v_mul_lo_u32") or x.startswith("v_mad_u64_u32") or x.startswith("v_mul_u32_u24") or x.startswith("v_mad_u32_u24")),
        "valu": c(lambda x: x.startswith("v_")),
        "salu": c(lambda x: x.startswith("s_") and not x.startswith(("s_cbranch", "s_branch", "s_waitcnt", "s_barrier", "s_nop", "s_load", "s_endpgm"))),
        "branch": c(lambda x: x.startswith("s_cbranch")),
        "lds": c(lambda x: x.startswith("ds_")),
        "ds_read_b128": c(lambda x: x.startswith("ds_read_b128")),
        "vmem": c(lambda x: x.startswith(("global_", "buffer_", "flat_"))),
        "scratch": c(lambda x: x.startswith("scratch_")),
        "s_waitcnt": c(lambda x: x == "s_waitcnt"),
        "s_barrier": c(lambda x: x == "s_barrier"),
    }


meta = {}
for l in lines[end:end + 80]:
    for k in ("NumVgprs", "NumSgprs", "Occupancy", "ScratchSize", "sgpr_spill_count", "vgpr_spill_count", "LDSByteSize"):
        m = re.search(r"; " + k + r":\s*(\S+)", l)
        if m and k not in meta:
            meta[k] = m.group(1)
print(sym)
print(" meta", meta)
print(" func", count(body))
print(" loop lines", len(loop), count(loop))
