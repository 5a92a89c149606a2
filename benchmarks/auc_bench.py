"""Grouped ROC AUC: the native engine (``ops.auc.auc_groups``, csrc/kernels/auc.hip) and its two
callers against the routes they replace.

    python benchmarks/auc_bench.py [--log2-rows 24] [--shapes small,workgroup,sorted,one] [--reps 7]
                                   [--loop-groups 4096] [--no-sql]

Needs a GPU.  ``2^log2-rows`` rows (fp64 scores rounded to 1e-4, so ties are common; 30 %
positives) in four shapes, one for every kernel class and one for a single group: ``small`` =
groups of 32 rows (sub-wave kernel), ``workgroup`` = groups of 1024 (LDS kernel), ``sorted`` =
groups of 4096 and ``one`` = one group (both the sorted route).  One JSON line per measurement with every repeat, min, median and max; every timed call
follows a warm-up call of the same shape and ends in a device synchronise; where two variants are
compared on the device they alternate repeat by repeat.

* ``auc_groups``    the engine on device tensors, groups contiguous, ``rowptr`` given;
* ``auc_batch``     ``evaluation.auc_batch`` on device tensors with shuffled group codes (adds the
                    sort of the codes and the bincount);
* ``metrics_cuda``  ``metrics.auc`` on the same device tensors (shape ``one`` only): the route a
                    trainer had, compared for equality;
* ``sql_native``    ``evaluation.auc.scalar_grouped`` on pandas columns with a session on the GPU:
                    the column conversion the loop also pays, then the engine;
* ``sql_loop``      what the executor's per-group loop does for ``auc(prob, label) GROUP BY g``:
                    ``metrics.auc`` on the group's Python lists.  Run on the first ``--loop-groups``
                    groups and SCALED linearly to all of them (``scaled_s``) where there are more;
                    compared with the engine for equality on the groups it ran."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GROUP_ROWS = {"small": 32, "workgroup": 1024, "sorted": 4096, "one": None}


def report(variant, ts, **extra):
    print(json.dumps({"variant": variant, "seconds": [round(t, 6) for t in ts], "min_s": round(min(ts), 6),
                      "median_s": round(statistics.median(ts), 6), "max_s": round(max(ts), 6), **extra}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rows", type=int, default=24)
    ap.add_argument("--shapes", default="small,workgroup,sorted,one")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-groups", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-sql", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import pandas as pd
    import torch

    from hivemall_amd import evaluation
    from hivemall_amd.evaluation import auc as route
    from hivemall_amd.evaluation import metrics as M
    from hivemall_amd.ops import auc as engine

    if not torch.cuda.is_available():
        raise SystemExit("auc_bench: no GPU")
    dev = torch.device("cuda")
    sync = lambda: torch.cuda.synchronize(dev)              # noqa: E731

    def timed(fns, reps):
        """``{name: [seconds]}``, ``{name: last result}``: one warm-up each, then alternated."""
        outs = {v: fn() for v, fn in fns.items()}
        sync()
        times = {v: [] for v in fns}
        for _ in range(reps):
            for v, fn in fns.items():
                t0 = time.perf_counter()
                outs[v] = fn()
                sync()
                times[v].append(time.perf_counter() - t0)
        return times, outs

    n = 1 << a.log2_rows
    rng = np.random.default_rng(a.seed)
    s_np = np.round(rng.random(n), 4)
    y_np = (rng.random(n) < 0.3).astype(np.int64)
    s, y = torch.from_numpy(s_np).to(dev), torch.from_numpy(y_np).to(dev)
    for shape in a.shapes.split(","):
        m = GROUP_ROWS[shape] or n
        G = n // m
        tag = {"shape": shape, "rows": n, "groups": G, "rows_per_group": m}
        rowptr = torch.arange(G + 1, dtype=torch.int64, device=dev) * m
        shuffle = torch.from_numpy(rng.permutation(n)).to(dev)
        codes = torch.empty(n, dtype=torch.int64, device=dev)
        codes[shuffle] = torch.arange(n, dtype=torch.int64, device=dev) // m
        s_sh, y_sh = torch.empty_like(s), torch.empty_like(y)
        s_sh[shuffle], y_sh[shuffle] = s, y                 # the same groups, rows in any order
        fns = {"auc_groups": lambda: engine.auc_values(*engine.auc_groups(s, y, rowptr)),
               "auc_batch": lambda: evaluation.auc_batch(s_sh, y_sh, codes)}
        if shape == "one":
            fns["metrics_cuda"] = lambda: torch.tensor([M.auc(s, y)], dtype=torch.float64, device=dev)
        times, outs = timed(fns, a.reps)
        got = outs["auc_groups"].cpu().numpy()
        for v in fns:
            same = bool(np.array_equal(outs[v].cpu().numpy(), got, equal_nan=True))
            report(v, times[v], equals_auc_groups=same, **tag)
        del shuffle, codes, s_sh, y_sh
        if a.no_sql:
            continue
        cols = [pd.Series(s_np), pd.Series(y_np)]
        gcodes = np.arange(n, dtype=np.int64) // m
        session = SimpleNamespace(device=dev)
        ts = []
        for _ in range(3):                                  # the first is the warm-up
            t0 = time.perf_counter()
            vals = route.scalar_grouped(cols, gcodes, G, session=session)
            ts.append(time.perf_counter() - t0)
        report("sql_native", ts[1:], equals_auc_groups=bool(np.array_equal(vals, got, equal_nan=True)), **tag)
        k = min(G, a.loop_groups)
        t0 = time.perf_counter()
        lists = [c.tolist() for c in cols]                  # Session._agg_values: once for the column
        t_lists = time.perf_counter() - t0
        t0 = time.perf_counter()
        loop = [M.auc(lists[0][g * m:(g + 1) * m], lists[1][g * m:(g + 1) * m]) for g in range(k)]
        dt = time.perf_counter() - t0
        report("sql_loop", [t_lists + dt], groups_run=k, tolist_s=round(t_lists, 3),
               scaled_s=round(t_lists + dt * G / k, 3),
               equals_auc_groups=bool(np.array_equal(loop, got[:k], equal_nan=True)), **tag)


if __name__ == "__main__":
    main()
