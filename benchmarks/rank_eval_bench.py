"""Ranking measures of ``[U, L]`` recommendation lists: the native engine
``ops.rank_eval.rank_measures`` (csrc/kernels/rank_eval.hip) against its OpenMP twin, against the
best formulation in plain torch on the same device, and against the per-row Python loop of
``evaluation.metrics`` that the engine replaces.

    python benchmarks/rank_eval_bench.py [--users 131072,1048576] [--lengths 10,100] [--reps 10]
                                         [--cpu-threads 16] [--python-rows 4096] [--no-cpu] [--no-python]

Needs a GPU.  Every user has a truth set whose size is Zipf-distributed (exponent 1.5, cut at
5000) over ``--items`` items; a rank position is drawn from the user's truth with probability 0.3
and from all items otherwise, so lists carry hits, misses and the odd duplicate.  ``k`` is ``L``.

One JSON line per measurement with every repeat, min, median and max and the time per list
position; every timed call follows a warm-up call of the same shape and ends in a device
synchronise.  The engine and the torch formulation alternate, repeat by repeat, in one run.

* ``kernel``       ``rank_measures`` on the GPU, all seven measures, the truth index built before;
* ``kernel_ndcg``  the same with ``measures = 1 << NDCG`` (one store, one ordered sum);
* ``build_truth``  the truth index itself (two stable sorts, once per data set, not per epoch);
* ``torch``        on the same device: composite keys ``row * items + item``, ``searchsorted`` into
                   the sorted truth keys, ``cumsum`` along the list, row reductions.  Its sums are
                   trees, so it is compared with the engine to a tolerance (``max_abs_diff``), not
                   bit for bit; its sorted truth keys are built before the timed window too;
* ``cpu_twin``     ``rank_measures`` on the CPU at ``OMP_NUM_THREADS`` threads;
* ``python``       the seven ``*_one`` functions on the first ``--python-rows`` rows (one run: it is
                   an interpreted loop), and that time SCALED linearly to ``U`` rows (``scaled_s``);
                   its values are compared with the engine's for equality on those rows."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def corpus(U: int, L: int, n_items: int, seed: int):
    """``(rank int64 [U, L], rowptr int64 [U + 1], items int64 [nnz])`` as numpy arrays."""
    import numpy as np

    rng = np.random.default_rng(seed)
    sizes = np.minimum(rng.zipf(1.5, U), min(5000, n_items)).astype(np.int64)
    rowptr = np.zeros(U + 1, dtype=np.int64)
    np.cumsum(sizes, out=rowptr[1:])
    items = rng.integers(0, n_items, int(rowptr[-1]), dtype=np.int64)       # unsorted, duplicates possible
    rank = rng.integers(0, n_items, (U, L), dtype=np.int64)
    from_truth = rng.random((U, L)) < 0.3
    pick = rowptr[:-1, None] + (rng.random((U, L)) * sizes[:, None]).astype(np.int64)
    rank[from_truth] = items[pick[from_truth]]
    return rank, rowptr, items


def torch_formulation(rank, tkeys, rowptr, n_items: int, log2tab, ideal):
    """fp64 ``[7, U]`` with ``k = L`` from searchsorted on composite keys and cumsum."""
    import torch

    U, L = rank.shape
    dev = rank.device
    rows = torch.arange(U, device=dev).unsqueeze(1)
    keys = (rows * n_items + rank).reshape(-1)
    at = torch.searchsorted(tkeys, keys).clamp_(max=tkeys.numel() - 1)
    hit = (tkeys[at] == keys).reshape(U, L)
    hitf = hit.to(torch.float64)
    upto = torch.cumsum(hitf, 1)
    n_pos = upto[:, -1]
    n_gt = (rowptr[1:] - rowptr[:-1]).to(torch.float64)
    pos1 = torch.arange(1, L + 1, device=dev, dtype=torch.float64)
    out = torch.zeros((7, U), dtype=torch.float64, device=dev)
    out[0] = n_pos / L
    out[1] = torch.where(n_gt > 0, n_pos / n_gt.clamp(min=1), 0.0)
    out[2] = (n_pos > 0).to(torch.float64)
    first = torch.argmax(hit.to(torch.int8), 1).to(torch.float64)
    out[3] = torch.where(n_pos > 0, 1.0 / (first + 1), 0.0)
    out[4] = torch.where(n_gt > 0, (hitf * upto / pos1).sum(1) / n_gt.clamp(min=1, max=L), 0.0)
    m = (rowptr[1:] - rowptr[:-1]).clamp(max=L)
    idcg = ideal[m]
    out[5] = torch.where(idcg > 0, (hitf / log2tab[:L]).sum(1) / idcg.clamp(min=1e-300), 0.0)
    n_neg = L - n_pos
    misses_before = (pos1 - 1) - (upto - hitf)
    correct = (hitf * (n_neg.unsqueeze(1) - misses_before)).sum(1)
    out[6] = torch.where(n_pos == 0, 0.0, torch.where(n_neg == 0, 1.0, correct / (n_pos * n_neg).clamp(min=1)))
    return out


def report(variant, ts, positions, **extra):
    med = statistics.median(ts)
    print(json.dumps({"variant": variant, "seconds": [round(t, 6) for t in ts],
                      "min_s": round(min(ts), 6), "median_s": round(med, 6), "max_s": round(max(ts), 6),
                      "positions": positions, "ns_per_position": round(med / max(positions, 1) * 1e9, 4),
                      **extra}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", default="131072,1048576")
    ap.add_argument("--lengths", default="10,100")
    ap.add_argument("--items", type=int, default=1 << 17)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--python-rows", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-python", action="store_true")
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", str(a.cpu_threads))
    threads = int(os.environ["OMP_NUM_THREADS"])
    import numpy as np
    import torch

    from hivemall_amd.evaluation import metrics as M
    from hivemall_amd.ops import rank_eval as re

    if not torch.cuda.is_available():
        raise SystemExit("rank_eval_bench: no GPU")
    dev = torch.device("cuda")
    sync = lambda: torch.cuda.synchronize(dev)              # noqa: E731
    one = (M.precision_at_one, M.recall_at_one, M.hitrate_one, M.mrr_one, M.average_precision_one, M.ndcg_one,
           M.ranking_auc)

    for U in (int(v) for v in a.users.split(",")):
        for L in (int(v) for v in a.lengths.split(",")):
            rank_np, rowptr_np, items_np = corpus(U, L, a.items, a.seed)
            tag = {"U": U, "L": L, "k": L, "truth_nnz": int(rowptr_np[-1]), "truth_max": int(np.diff(rowptr_np).max())}
            rank_c, rowptr_c, items_c = (torch.from_numpy(x) for x in (rank_np, rowptr_np, items_np))
            rank, rowptr, items = rank_c.to(dev), rowptr_c.to(dev), items_c.to(dev)

            ts = []
            for i in range(4):                              # the first is the warm-up
                sync()
                t0 = time.perf_counter()
                truth = re.build_truth(rowptr, items)
                sync()
                ts.append(time.perf_counter() - t0)
            report("build_truth", ts[1:], int(rowptr_np[-1]), **tag)
            trow = torch.repeat_interleave(torch.arange(U, device=dev), truth.rowptr[1:] - truth.rowptr[:-1])
            tkeys = trow * a.items + truth.items            # sorted: rows ascend, items ascend inside one
            log2tab, ideal = (t.to(dev) for t in map(torch.from_numpy, re.tables(max(L, truth.max_len) + 1)))

            fns = {"kernel": lambda: re.rank_measures(rank, truth, L),
                   "kernel_ndcg": lambda: re.rank_measures(rank, truth, L, measures=1 << re.NDCG),
                   "torch": lambda: torch_formulation(rank, tkeys, truth.rowptr, a.items, log2tab, ideal)}
            times = {v: [] for v in fns}
            outs = {}
            for fn in fns.values():                         # warm-up, same shape
                fn()
            sync()
            for _ in range(a.reps):                         # alternated, repeat by repeat
                for v, fn in fns.items():
                    t0 = time.perf_counter()
                    outs[v] = fn()
                    sync()
                    times[v].append(time.perf_counter() - t0)
            diff = float((outs["torch"] - outs["kernel"]).abs().max())
            same_ndcg = bool(torch.equal(outs["kernel_ndcg"][re.NDCG], outs["kernel"][re.NDCG]))
            report("kernel", times["kernel"], U * L, **tag)
            report("kernel_ndcg", times["kernel_ndcg"], U * L, equals_kernel=same_ndcg, **tag)
            report("torch", times["torch"], U * L, max_abs_diff=diff, **tag)
            got = outs["kernel"].cpu()
            del outs, tkeys, trow

            if not a.no_cpu:
                truth_c = re.build_truth(rowptr_c, items_c)
                re.rank_measures(rank_c, truth_c, L)
                ts = []
                for _ in range(max(2, a.reps // 3)):
                    t0 = time.perf_counter()
                    out = re.rank_measures(rank_c, truth_c, L)
                    ts.append(time.perf_counter() - t0)
                report("cpu_twin", ts, U * L, threads=threads, equals_kernel=bool(torch.equal(out, got)), **tag)
            if not a.no_python:
                m = min(a.python_rows, U)
                ranks = [r.tolist() for r in rank_np[:m]]
                truths = [items_np[rowptr_np[u]:rowptr_np[u + 1]].tolist() for u in range(m)]
                t0 = time.perf_counter()
                vals = [[fn(r, t, L) for r, t in zip(ranks, truths)] for fn in one]
                dt = time.perf_counter() - t0
                equal = bool(np.array_equal(np.asarray(vals).view(np.int64), got[:, :m].numpy().view(np.int64)))
                report("python", [dt], m * L, scaled_s=round(dt * (U / m), 3), scaled_to={"U": U}, rows=m,
                       equals_kernel=equal, **tag)
            del rank, rowptr, items, truth


if __name__ == "__main__":
    main()
