"""MinHash signatures: the fused kernel ``ops.minhash.minhash_signatures``
(csrc/kernels/minhash.hip) against its OpenMP twin, against a naive device composition of existing
parts, and against today's per-row ``minhashes`` / ``bbit_minhash``.

    python benchmarks/minhash_bench.py [--rows 1000000] [--fields 39] [--hashes 10 128] [--reps 5]
                                       [--cpu-threads 16] [--per-row-rows 200] [--cpu-only]
                                       [--no-cpu] [--no-per-row]

Needs a GPU (``--cpu-only`` runs the twin and the per-row functions alone).  The workload is
``--rows`` rows of ``--fields`` seeded ``c<field>=<8 hex>`` names, packed once on the host.  One
JSON line per measurement with every repeat, min, median and max and the time per row; every timed
call follows one warm-up call of the same shape and ends in a device synchronise:

* ``fused``        ``minhash_signatures`` on device-resident buffers, with its validation passes
                   over the offsets and name lengths (the call as a user of ``ops`` makes it);
* ``kernel``       the same with ``check=False``: the launch alone, as ``knn.*_batch`` and the
                   SQL functions call it after packing the column themselves;
* ``fused_h2d``    the same plus the host-to-device copy of (buf, off, nlen, rowptr);
* ``composition``  H launches of ``hm_mhash`` (raw hashes, one seed each) and a segmented min in
                   torch (``scatter_reduce_`` ``amin`` over the sign-flipped hashes), timed
                   interleaved with ``fused`` in the same loop; its result is compared with the
                   kernel's;
* ``cpu_twin``     the twin at ``OMP_NUM_THREADS`` threads where the environment sets it, at
                   ``--cpu-threads`` otherwise (the line reports which), compared with the kernel;
* ``per_row``      ``minhashes(row, False, 5, 2)`` (H = 10) or ``bbit_minhash(row)`` (H = 128) on
                   the first ``--per-row-rows`` rows, one run, scaled per row."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def workload(rows: int, fields: int, seed: int):
    """(buf uint8, off int64, nlen int32, rowptr int64) numpy arrays; every row has the same
    layout, so the bytes are filled column-wise."""
    import numpy as np

    rng = np.random.default_rng(seed)
    prefixes = [f"c{f}=".encode() for f in range(fields)]
    lens = np.array([len(p) + 8 for p in prefixes], dtype=np.int64)
    row_bytes = int(lens.sum())
    img = np.empty((rows, row_bytes), dtype=np.uint8)
    hexd = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)
    pos = 0
    for p in prefixes:
        img[:, pos:pos + len(p)] = np.frombuffer(p, dtype=np.uint8)
        pos += len(p)
        v = rng.integers(0, 1 << 32, size=rows, dtype=np.uint64)
        for d in range(8):
            img[:, pos + d] = hexd[((v >> np.uint64(4 * (7 - d))) & np.uint64(15)).astype(np.int64)]
        pos += 8
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    off = np.empty(rows * fields + 1, dtype=np.int64)
    off[:-1] = (np.arange(rows, dtype=np.int64)[:, None] * row_bytes + starts[None, :]).reshape(-1)
    off[-1] = rows * row_bytes
    nlen = np.tile(lens.astype(np.int32), rows)
    rowptr = np.arange(rows + 1, dtype=np.int64) * fields
    return img.reshape(-1), off, nlen, rowptr


def timed(fn, reps, sync):
    fn()                                                    # warm-up, same shape
    sync()
    ts = []
    out = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return ts, out


def report(variant, ts, rows, **extra):
    med = statistics.median(ts)
    print(json.dumps({"variant": variant, "seconds": [round(t, 5) for t in ts],
                      "min_s": round(min(ts), 5), "median_s": round(med, 5), "max_s": round(max(ts), 5),
                      "rows": rows, "us_per_row": round(med / max(rows, 1) * 1e6, 4), **extra}), flush=True)


def composition(buf, off, rowptr, row_of, H):
    """int32 [n_rows, H] from existing parts: hm_mhash per seed, segmented min in torch."""
    import torch

    from hivemall_amd.ops._packed import mhash_packed

    n_rows = rowptr.numel() - 1
    flip = -(1 << 31)                                       # unsigned order as signed order
    out = torch.full((H, n_rows), (1 << 31) - 1, dtype=torch.int32, device=buf.device)
    for h in range(H):
        tmp = mhash_packed(buf, off, 0, h)
        tmp ^= flip
        out[h].scatter_reduce_(0, row_of, tmp, reduce="amin", include_self=True)
    out ^= flip
    out[:, rowptr[1:] == rowptr[:-1]] = 0
    return out.t().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--fields", type=int, default=39)
    ap.add_argument("--hashes", type=int, nargs="+", default=[10, 128])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--per-row-rows", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-per-row", action="store_true")
    a = ap.parse_args()
    # the twin's OpenMP pool is sized once, when the runtime starts: an ambient OMP_NUM_THREADS
    # is left alone and reported, --cpu-threads applies only where none is set
    os.environ.setdefault("OMP_NUM_THREADS", str(a.cpu_threads))
    threads = int(os.environ["OMP_NUM_THREADS"])
    import numpy as np
    import torch

    from hivemall_amd import knn
    from hivemall_amd.ops.minhash import minhash_signatures

    if not a.cpu_only and not torch.cuda.is_available():
        raise SystemExit("minhash_bench: no GPU")
    host = [torch.from_numpy(x) for x in workload(a.rows, a.fields, a.seed)]
    shape = dict(fields=a.fields, nnz=a.rows * a.fields, bytes=int(host[0].numel()))
    nosync = lambda: None                                   # noqa: E731
    kernel_sig = {}

    if not a.cpu_only:
        dev = torch.device("cuda")
        sync = lambda: torch.cuda.synchronize(dev)          # noqa: E731
        on_dev = [t.to(dev) for t in host]
        buf, off, nlen, rowptr = on_dev
        row_of = torch.repeat_interleave(torch.arange(a.rows, device=dev), rowptr[1:] - rowptr[:-1])
        for H in a.hashes:
            fused = lambda: minhash_signatures(buf, off, nlen, rowptr, H)       # noqa: E731
            comp = lambda: composition(buf, off, rowptr, row_of, H)             # noqa: E731
            sig = fused()
            ref = comp()                                    # both warm
            sync()
            same = bool(torch.equal(sig, ref))
            kern = lambda: minhash_signatures(buf, off, nlen, rowptr, H, check=False)   # noqa: E731
            kern()
            tf, tk, tc = [], [], []
            for _ in range(a.reps):                         # interleaved: A B C A B C ...
                for fn, ts in ((fused, tf), (kern, tk), (comp, tc)):
                    sync()
                    t0 = time.perf_counter()
                    fn()
                    sync()
                    ts.append(time.perf_counter() - t0)
            report("fused", tf, a.rows, H=H, **shape)
            report("kernel", tk, a.rows, H=H, **shape)
            report("composition", tc, a.rows, H=H, equals_fused=same, **shape)
            ts, _ = timed(lambda: minhash_signatures(*(t.to(dev) for t in host), H, check=False), a.reps, sync)
            report("fused_h2d", ts, a.rows, H=H, **shape)
            kernel_sig[H] = sig.cpu()
            del sig, ref
        del on_dev, buf, off, nlen, rowptr, row_of
        torch.cuda.empty_cache()

    if not a.no_cpu:
        for H in a.hashes:
            ts, sig = timed(lambda: minhash_signatures(*host, H), a.reps, nosync)
            extra = {"equals_kernel": bool(torch.equal(sig, kernel_sig[H]))} if H in kernel_sig else {}
            report("cpu_twin", ts, a.rows, H=H, threads=threads, **shape, **extra)

    if not a.no_per_row:
        n = min(a.per_row_rows, a.rows)
        b, o = host[0].numpy(), host[1].numpy()
        rows = [[bytes(b[o[s]:o[s + 1]]).decode() for s in range(r * a.fields, (r + 1) * a.fields)]
                for r in range(n)]
        for H in a.hashes:
            if H == 10:
                fn, name = (lambda r: knn.minhashes(r, False, 5, 2)), "minhashes(row, False, 5, 2)"
            else:
                fn, name = (lambda r: knn.bbit_minhash(r, H, 1)), f"bbit_minhash(row, {H}, 1)"
            t0 = time.perf_counter()
            got = [fn(r) for r in rows]
            dt = time.perf_counter() - t0
            batch = knn.minhashes_batch(rows, 5, 2, device="cpu") if H == 10 else \
                knn.bbit_minhash_batch(rows, H, 1, device="cpu")
            report("per_row", [dt], n, H=H, call=name, equals_batch=got == batch,
                   seconds_for_1m_rows=round(dt / n * 1e6, 1))


if __name__ == "__main__":
    main()
