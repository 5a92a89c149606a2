"""``each_top_k`` row selection: the native engine ``ops.each_top_k.segment_topk``
(csrc/kernels/each_top_k.hip) against its OpenMP twin, against what one would write in torch
without the kernel, and against the per-row Python loop ``knn._each_top_k_python``.

    python benchmarks/each_top_k_bench.py [--n 16777216] [--reps 20] [--cpu-threads 16]
                                          [--python-n 262144] [--no-cpu] [--no-python]

Needs a GPU.  Three shapes at ``--n`` rows, scores normal and rounded to four decimals (so ties
are common):

* ``short``  n / 128 groups of 128 rows, k = 10, clustered (the one-wave-per-group kernel);
* ``long``   16 groups of n / 16 rows, k = 100, clustered (the streaming filter, two levels);
* ``zipf``   65,536 groups whose sizes follow 1 / rank, rows in shuffled order, k = 10 (the
             stable sort by group in front of both kernels).

One JSON line per measurement with every repeat, min, median and max and the time per input row;
every timed call follows a warm-up call of the same shape and ends in a device synchronise.  The
kernel and the torch composition alternate, repeat by repeat, in one run.

* ``kernel``    ``segment_topk`` on the GPU (validation, sort where needed, segment bounds, launches);
* ``torch``     on the same device: a stable ``torch.sort`` by score, a stable ``torch.sort`` of
                the reordered codes, group starts by ``searchsorted``, and a cut at rank < k;
* ``cpu_twin``  ``segment_topk`` on the CPU, at ``OMP_NUM_THREADS`` threads where the
                environment sets it, at ``--cpu-threads`` otherwise (the line reports which);
* ``python``    ``_each_top_k_python`` on the first ``--python-n`` rows (one run: it is an
                interpreted loop), and that time SCALED linearly to ``--n`` rows (``scaled_s``).

Every timed output is compared with the twin's for equality (``equals_twin``); the Python loop's
with the twin's on the same prefix."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def shapes(n: int, seed: int):
    """(name, codes int32 [n], G, k) for every shape."""
    import numpy as np

    rng = np.random.default_rng(seed)
    yield "short", np.repeat(np.arange(n // 128, dtype=np.int32), 128), n // 128, 10
    yield "long", np.repeat(np.arange(16, dtype=np.int32), n // 16), 16, 100
    G = 1 << 16
    cdf = np.cumsum(1.0 / np.arange(1, G + 1))
    codes = np.searchsorted(cdf / cdf[-1], rng.random(n)).clip(max=G - 1).astype(np.int32)
    yield "zipf", codes, G, 10


def torch_composition(score, codes, G: int, k: int):
    """The rows ``segment_topk`` returns, from two stable sorts and a rank cut."""
    import torch

    by_score = torch.sort(-score, stable=True).indices
    by_code, o = torch.sort(codes[by_score], stable=True)
    # group starts by binary search in the sorted codes (torch.bincount is far slower on a skewed
    # column: docs/perf_notes.md "each_top_k")
    start = torch.searchsorted(by_code, torch.arange(G, dtype=torch.int32, device=score.device))
    rank = torch.arange(score.numel(), device=score.device) - start[by_code.long()]
    return by_score[o[rank < k]].to(torch.int32)


def report(variant, ts, rows, **extra):
    med = statistics.median(ts)
    print(json.dumps({"variant": variant, "seconds": [round(t, 5) for t in ts],
                      "min_s": round(min(ts), 5), "median_s": round(med, 5), "max_s": round(max(ts), 5),
                      "rows": rows, "ns_per_row": round(med / max(rows, 1) * 1e9, 3), **extra}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--python-n", type=int, default=1 << 18)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-python", action="store_true")
    a = ap.parse_args()
    if a.n % 2048:
        raise SystemExit("each_top_k_bench: --n must be a multiple of 2048")
    # the twin's OpenMP pool is sized once, when the runtime starts: an ambient OMP_NUM_THREADS
    # is left alone and reported, --cpu-threads applies only where none is set
    os.environ.setdefault("OMP_NUM_THREADS", str(a.cpu_threads))
    threads = int(os.environ["OMP_NUM_THREADS"])
    import numpy as np
    import torch

    from hivemall_amd.ops.each_top_k import STATS, segment_topk

    if not torch.cuda.is_available():
        raise SystemExit("each_top_k_bench: no GPU")
    dev = torch.device("cuda")
    sync = lambda: torch.cuda.synchronize(dev)              # noqa: E731

    for name, codes_np, G, k in shapes(a.n, a.seed):
        score_np = np.round(np.random.default_rng(a.seed + 1).normal(size=a.n), 4)
        sc, cc = torch.from_numpy(score_np), torch.from_numpy(codes_np)
        sg, cg = sc.to(dev), cc.to(dev)
        tag = {"shape": name, "n": a.n, "groups": G, "k": k}
        ref = segment_topk(sc, cc, G, k)[0] if not a.no_cpu else None
        same = lambda got: None if ref is None else bool(torch.equal(got.cpu(), ref))   # noqa: E731

        fns = {"kernel": lambda: segment_topk(sg, cg, G, k)[0], "torch": lambda: torch_composition(sg, cg, G, k)}
        times = {v: [] for v in fns}
        outs = {}
        for fn in fns.values():                             # warm-up, same shape
            fn()
        sync()
        for _ in range(a.reps):                             # alternated, repeat by repeat
            for v, fn in fns.items():
                t0 = time.perf_counter()
                outs[v] = fn()
                sync()
                times[v].append(time.perf_counter() - t0)
        segment_topk(sg, cg, G, k)
        report("kernel", times["kernel"], a.n, equals_twin=same(outs["kernel"]), levels=STATS["levels"],
               work_items=STATS["items"], **tag)
        report("torch", times["torch"], a.n, equals_twin=same(outs["torch"]), **tag)
        del sg, cg, outs
        if not a.no_cpu:
            ts = []
            for _ in range(max(1, a.reps // 4)):
                t0 = time.perf_counter()
                out = segment_topk(sc, cc, G, k)[0]
                ts.append(time.perf_counter() - t0)
            report("cpu_twin", ts, a.n, threads=threads, equals_twin=same(out), **tag)
        if not a.no_python:
            from hivemall_amd.knn import _each_top_k_python

            m = min(a.python_n, a.n)
            group, score = codes_np[:m].tolist(), score_np[:m].tolist()
            t0 = time.perf_counter()
            df = _each_top_k_python(k, group, score, list(range(m)))
            dt = time.perf_counter() - t0
            # the loop orders groups by first appearance, the engine by code: compare per group
            twin, optr = segment_topk(sc[:m].contiguous(), cc[:m].contiguous(), G, k)
            twin, optr = twin.numpy(), optr.numpy()
            got = df["c0"].to_numpy()
            first = codes_np[:m][got[df["rank"].to_numpy() == 1]]
            want = np.concatenate([twin[optr[g]:optr[g + 1]] for g in first]) if len(first) else twin[:0]
            report("python", [dt], m, scaled_s=round(dt * (a.n / m), 2), scaled_to={"n": a.n},
                   equals_twin=bool(np.array_equal(got, want)), **{**tag, "n": m, "groups": len(first)})
        del sc, cc


if __name__ == "__main__":
    main()
