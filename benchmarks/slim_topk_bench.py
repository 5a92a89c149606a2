"""SLIM recommendation: the fused kernel ``ops.slim.slim_topk`` (csrc/kernels/slim_topk.hip)
against a torch formulation on the same device and against its OpenMP twin.

    python benchmarks/slim_topk_bench.py [--users 138493] [--items 27278] [--per-user 144]
                                         [--knn 50] [--k 10 100] [--reps 10] [--cpu-threads 16]
                                         [--no-cpu]

Needs a GPU.  The default is the ML-20M shape: users x items with about ``--per-user`` ratings a
user (half-star values, item popularity ~ 1 / rank^0.8, duplicates dropped) and a model of
``--knn`` neighbours per item with weights in (0, 0.1).  Synthetic, seeded.

One JSON line per measurement with every repeat, min, median and max; every timed call follows a
warm-up call of the same shape and ends in a device synchronise; kernel and torch alternate,
repeat by repeat, in one run.

* ``kernel``    ``slim_topk(check=False)`` on the GPU: the transposed model (one sort) and the launch;
* ``torch``     ``models.recommend._slim_topk_torch`` on the same device: sparse ``R @ W^T`` in
                blocks of 4096 users (a dense block of scores and one of term counts), then
                ``torch.topk``;
* ``cpu_twin``  ``slim_topk`` on the CPU at ``OMP_NUM_THREADS`` threads where the environment sets
                it, at ``--cpu-threads`` otherwise (the line reports which).

``equals_twin``: items and score bits equal the twin's.  For torch, whose sums and ties are
ordered differently, ``items_agree`` is the share of equal item slots instead."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make(users: int, items: int, per_user: int, knn: int, seed: int):
    """(R csr, model csr) as NumPy triples."""
    import numpy as np

    rng = np.random.default_rng(seed)
    cdf = np.cumsum(1.0 / np.arange(1, items + 1) ** 0.8)

    def popular(n):
        return np.searchsorted(cdf / cdf[-1], rng.random(n)).clip(max=items - 1)

    def csr(row, col, val, n_rows, drop_diagonal=False):
        keep = row != col if drop_diagonal else np.ones(len(row), dtype=bool)
        key, first = np.unique(row[keep] * items + col[keep], return_index=True)
        ptr = np.zeros(n_rows + 1, dtype=np.int64)
        np.cumsum(np.bincount(key // items, minlength=n_rows), out=ptr[1:])
        return ptr, (key % items).astype(np.int32), val[keep][first]

    n = users * per_user
    R = csr(rng.integers(0, users, n), popular(n), rng.integers(1, 11, n) * 0.5, users)
    m = items * knn
    M = csr(np.repeat(np.arange(items), knn), popular(m), rng.random(m) * 0.1 + 1e-3, items, True)
    return R, M


def report(variant, ts, users, **extra):
    med = statistics.median(ts)
    print(json.dumps({"variant": variant, "seconds": [round(t, 5) for t in ts],
                      "min_s": round(min(ts), 5), "median_s": round(med, 5), "max_s": round(max(ts), 5),
                      "users": users, "us_per_user": round(med / max(users, 1) * 1e6, 3), **extra}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138493)
    ap.add_argument("--items", type=int, default=27278)
    ap.add_argument("--per-user", type=int, default=144)
    ap.add_argument("--knn", type=int, default=50)
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", str(a.cpu_threads))
    threads = int(os.environ["OMP_NUM_THREADS"])
    import torch

    from hivemall_amd.models.recommend import _slim_topk_torch
    from hivemall_amd.ops.slim import slim_topk

    if not torch.cuda.is_available():
        raise SystemExit("slim_topk_bench: no GPU")
    dev = torch.device("cuda")
    sync = lambda: torch.cuda.synchronize(dev)              # noqa: E731
    R, M = make(a.users, a.items, a.per_user, a.knn, a.seed)
    cpu = [torch.from_numpy(x) for x in R + M]
    gpu = [t.to(dev) for t in cpu]
    for k in a.k:
        tag = {"items": a.items, "nnz": int(R[0][-1]), "model_nnz": int(M[0][-1]), "k": k}
        ref, ts = None, []
        if not a.no_cpu:
            for _ in range(max(1, a.reps // 5)):
                t0 = time.perf_counter()
                ref = slim_topk(*cpu, k, check=False)
                ts.append(time.perf_counter() - t0)
        fns = {"kernel": lambda: slim_topk(*gpu, k, check=False),
               "torch": lambda: _slim_topk_torch(*gpu, k, True)}
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
        ki, ks = (t.cpu() for t in outs["kernel"])
        same = None if ref is None else bool(torch.equal(ki, ref[0]) and torch.equal(ks.view(torch.int64),
                                                                                      ref[1].view(torch.int64)))
        report("kernel", times["kernel"], a.users, equals_twin=same, **tag)
        report("torch", times["torch"], a.users,
               items_agree=round(float((outs["torch"][0].cpu() == ki).double().mean()), 6), **tag)
        if ref is not None:
            report("cpu_twin", ts, a.users, threads=threads, **tag)
        del outs


if __name__ == "__main__":
    main()
