"""HyperLogLog / Bloom sketches: the fused kernels of ``ops.sketch`` (csrc/kernels/sketch.hip)
against their OpenMP twin, against the per-value Python loop and against a device composition of
parts the tree had before them.

    python benchmarks/sketch_bench.py [--log2n 24] [--reps 7] [--iters 5] [--cpu-threads 16]
                                      [--python-values 16384] [--sweep] [--cpu-only] [--no-cpu]
                                      [--no-python]

Needs a GPU (``--cpu-only`` runs the twin and the Python loop alone).  The workload is ``2^log2n``
values of 8-16 random lowercase bytes, packed once on the host; group ids are uniform random.  One
JSON line per measurement.  A timing is ``--iters`` back-to-back calls between two device
synchronises, divided by ``--iters``; ``--reps`` timings follow one warm-up of the same shape and
the median is reported next to every repeat.  The variants of one row are timed interleaved in the
same loop.  Every call starts from fresh zeroed registers / bits (their allocation and memset are
inside the timing, for every variant): a second update into the same registers would only read.

Rows: ``hll`` = ``hll_registers`` + ``hll_histogram`` at (G, p) = (1, 15), (1024, 15) and
(65536, 12) - the last two take the direct path; ``bloom_bits`` with G = 1 and ``bloom_test`` with
F = 1 at (m, k) = (65536, 4).  Variants:

* ``fused``        the kernels on device-resident buffers, ``check=False`` (as the SQL hooks and
                   the ``misc`` column functions call them after packing the column themselves);
* ``composition``  what the tree offered before: two raw ``hm_mhash`` launches (the two seeds of
                   h64), then torch on the device - index and rho by shifts and an exact
                   ``frexp`` bit length, ``scatter_reduce_(amax)`` into the registers, ``bincount``
                   for the histogram; its registers and histogram are compared with the kernels'.
                   There is none for the Bloom rows: h2 = mm3(s, h1) needs a seed per value, which
                   ``hm_mhash`` does not take;
* ``cpu_twin``     the twin at ``OMP_NUM_THREADS`` threads where the environment sets it, at
                   ``--cpu-threads`` otherwise (the line reports which), compared with the kernels;
* ``python``       ``approx_count_distinct`` / ``bloom`` / ``bloom_contains`` over the first
                   ``--python-values`` values, one run, reported per value and SCALED to the full
                   column (``scaled_seconds``).

``--sweep`` adds the LDS path's grid cap: the (1, 15) and (2, 15) rows at caps 64..4096."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HLL_ROWS = [(1, 15), (1024, 15), (65536, 12)]
M, K = 65536, 4


def workload(n: int, seed: int):
    import numpy as np

    rng = np.random.default_rng(seed)
    lens = rng.integers(8, 17, size=n, dtype=np.int64)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    buf = rng.integers(97, 123, size=int(off[-1]), dtype=np.uint8)
    return buf, off


def report(row, variant, ts, n, **extra):
    med = statistics.median(ts)
    print(json.dumps({"row": row, "variant": variant, "seconds": [round(t, 6) for t in ts],
                      "median_s": round(med, 6), "values": n, "ns_per_value": round(med / max(n, 1) * 1e9, 3),
                      **extra}), flush=True)


def interleaved(fns: dict, reps: int, iters: int, sync) -> dict:
    for fn in fns.values():                                 # warm-up, same shape
        fn()
    sync()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            sync()
            ts[k].append((time.perf_counter() - t0) / iters)
    return ts


def _bit_length(v):
    """Exact bit length of int64 values in 0..2^60 on the device: frexp of a value below 2^30 is
    exact in fp64, so the two halves are taken apart."""
    import torch

    hi = v >> 30
    lo = v & ((1 << 30) - 1)
    e_hi = torch.frexp(hi.double())[1]
    e_lo = torch.frexp(lo.double())[1]
    return torch.where(hi != 0, e_hi + 30, e_lo)


def composition(buf, off, gid64, G, p):
    """(reg uint8 [G, 2^p], hist int32 [G, 66]) from existing parts."""
    import torch

    from hivemall_amd.ops._packed import mhash_packed

    halves = [mhash_packed(buf, off, 0, seed).long() & 0xFFFFFFFF for seed in (0x9747B28C, 0x5BD1E995)]
    h = (halves[0] << 32) | halves[1]                       # int64 bit pattern of h64
    m = 1 << p
    idx = (h >> (64 - p)) & (m - 1)
    low = h & ((1 << (64 - p)) - 1)                         # the 64 - p bits below the index
    rho = (64 - p) - _bit_length(low) + 1                   # clz64(h << p) capped at 64 - p, + 1
    reg = torch.zeros(G * m, dtype=torch.int32, device=buf.device)
    reg.scatter_reduce_(0, gid64 * m + idx, rho.int(), reduce="amax", include_self=True)
    rows = torch.arange(G, dtype=torch.int32, device=buf.device)[:, None] * 66
    hist = torch.bincount((reg.reshape(G, m) + rows).reshape(-1), minlength=G * 66).reshape(G, 66).int()
    return reg.reshape(G, m).to(torch.uint8), hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--python-values", type=int, default=1 << 14)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-python", action="store_true")
    a = ap.parse_args()
    # the twin's OpenMP pool is sized once, when the runtime starts: an ambient OMP_NUM_THREADS
    # is left alone and reported, --cpu-threads applies only where none is set
    os.environ.setdefault("OMP_NUM_THREADS", str(a.cpu_threads))
    threads = int(os.environ["OMP_NUM_THREADS"])
    import numpy as np
    import torch

    from hivemall_amd import misc
    from hivemall_amd.ops import _packed, sketch as sk

    if not a.cpu_only and not torch.cuda.is_available():
        raise SystemExit("sketch_bench: no GPU")
    n = 1 << a.log2n
    buf_h, off_h = (torch.from_numpy(x) for x in workload(n, a.seed))
    rng = np.random.default_rng(a.seed + 1)
    gids_h = {G: torch.from_numpy(rng.integers(0, G, size=n, dtype=np.int32)) for G, _ in HLL_ROWS}
    shape = dict(bytes=int(buf_h.numel()))
    kept = {}

    def hll(buf, off, gid, G, p, **kw):
        reg = sk.hll_registers(buf, off, gid, G, p, check=False, **kw)
        return reg, sk.hll_histogram(reg)

    if not a.cpu_only:
        dev = torch.device("cuda")
        sync = lambda: torch.cuda.synchronize(dev)          # noqa: E731
        buf, off = _packed.pad16(buf_h.to(dev)), off_h.to(dev)
        for G, p in HLL_ROWS:
            gid = gids_h[G].to(dev)
            gid64 = gid.long()
            reg, hist = hll(buf, off, gid, G, p)
            creg, chist = composition(buf, off, gid64, G, p)
            sync()
            same = bool(torch.equal(reg, creg) and torch.equal(hist, chist))
            del creg, chist
            ts = interleaved({"fused": lambda: hll(buf, off, gid, G, p),
                              "composition": lambda: composition(buf, off, gid64, G, p)}, a.reps, a.iters, sync)
            row = f"hll G={G} p={p}"
            report(row, "fused", ts["fused"], n, path="lds" if (G << p) <= sk.LDS_REG_BYTES else "direct", **shape)
            report(row, "composition", ts["composition"], n, equals_fused=same,
                   fused_speedup=round(statistics.median(ts["composition"]) / statistics.median(ts["fused"]), 2))
            kept[row] = (reg.cpu(), hist.cpu())
            del gid, gid64, reg, hist
            torch.cuda.empty_cache()
        gid = torch.zeros(n, dtype=torch.int32, device=dev)
        bits = sk.bloom_bits(buf, off, gid, 1, M, K, check=False)
        ts = interleaved({"add": lambda: sk.bloom_bits(buf, off, gid, 1, M, K, check=False),
                          "test": lambda: sk.bloom_test(bits, gid, buf, off, K, check=False)}, a.reps, a.iters, sync)
        report("bloom_bits G=1", "fused", ts["add"], n, m=M, k=K, composition=None, **shape)
        report("bloom_test F=1", "fused", ts["test"], n, m=M, k=K, composition=None, **shape)
        kept["bloom_bits"] = bits.cpu()
        kept["bloom_test"] = sk.bloom_test(bits, gid, buf, off, K, check=False).cpu()
        if a.sweep:
            for G, p in ((1, 15), (2, 15)):
                g = gids_h[1].to(dev) if G == 1 else (gids_h[1024].to(dev) & 1)
                caps = [64, 128, 256, 512, 1024, 2048, 4096]
                ts = interleaved({c: (lambda c=c: hll(buf, off, g, G, p, _lds_grid=c)) for c in caps},
                                 a.reps, a.iters, sync)
                for c in caps:
                    report(f"hll G={G} p={p}", "lds_grid_sweep", ts[c], n, lds_grid=c)
        del buf, off, gid, bits
        torch.cuda.empty_cache()

    nosync = lambda: None                                   # noqa: E731
    if not a.no_cpu:
        reps = min(a.reps, 3)
        for G, p in HLL_ROWS:
            row = f"hll G={G} p={p}"
            ts = interleaved({"t": lambda: hll(buf_h, off_h, gids_h[G], G, p)}, reps, 1, nosync)["t"]
            reg, hist = hll(buf_h, off_h, gids_h[G], G, p)
            extra = {"equals_kernel": bool(torch.equal(reg, kept[row][0]) and torch.equal(hist, kept[row][1]))} \
                if row in kept else {}
            report(row, "cpu_twin", ts, n, threads=threads, **extra)
        gid = torch.zeros(n, dtype=torch.int32)
        bits = sk.bloom_bits(buf_h, off_h, gid, 1, M, K, check=False)
        ts = interleaved({"add": lambda: sk.bloom_bits(buf_h, off_h, gid, 1, M, K, check=False),
                          "test": lambda: sk.bloom_test(bits, gid, buf_h, off_h, K, check=False)}, reps, 1, nosync)
        ex = {"equals_kernel": bool(torch.equal(bits, kept["bloom_bits"]))} if "bloom_bits" in kept else {}
        report("bloom_bits G=1", "cpu_twin", ts["add"], n, threads=threads, **ex)
        hit = sk.bloom_test(bits, gid, buf_h, off_h, K, check=False)
        ex = {"equals_kernel": bool(torch.equal(hit, kept["bloom_test"]))} if "bloom_test" in kept else {}
        report("bloom_test F=1", "cpu_twin", ts["test"], n, threads=threads, **ex)

    if not a.no_python:
        k = min(a.python_values, n)
        b, o = buf_h.numpy(), off_h.numpy()
        vals = [bytes(b[o[s]:o[s + 1]]).decode() for s in range(k)]
        gid = torch.zeros(k, dtype=torch.int32)
        sub = (buf_h[:int(o[k])], off_h[:k + 1], gid)

        def once(row, fn, equal):
            t0 = time.perf_counter()
            got = fn()
            dt = time.perf_counter() - t0
            report(row, "python", [dt], k, us_per_value=round(dt / k * 1e6, 3), equals_twin=bool(equal(got)),
                   scaled_seconds=round(dt / k * n, 1), scaled_to=n)

        reg = sk.hll_registers(*sub, 1, 15)
        est = sk.hll_estimate(sk.hll_histogram(reg), 15)[0]
        once("hll G=1 p=15", lambda: misc.approx_count_distinct(vals), lambda got: got == est)
        bits = sk.bloom_bits(*sub, 1, M, K)
        flt = misc._bloom_serialize(M, K, bits)[0]
        once("bloom_bits G=1", lambda: misc.bloom(vals), lambda got: got == flt)
        hit = sk.bloom_test(bits, gid, sub[0], sub[1], K).bool().tolist()
        once("bloom_test F=1", lambda: [misc.bloom_contains(flt, v) for v in vals], lambda got: got == hit)


if __name__ == "__main__":
    main()
