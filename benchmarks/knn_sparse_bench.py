"""Item-item cosine top-k on an ML-20M-shaped synthetic ratings matrix: ``ops.knn_sparse.knn_cols``
(csrc/kernels/knn_sparse.hip) against the dense device route ``knn.topk_similar`` on the
densified ``[items, users]`` matrix and against the OpenMP twin.

    python benchmarks/knn_sparse_bench.py [--items 27278] [--users 138493] [--nnz 20000000]
                                          [--k 20] [--reps 5] [--cpu-reps 5] [--cpu-threads 16]
                                          [--no-dense] [--no-cpu]

Seeded generator as in ``benchmarks/slim_bench.py``: shifted-Zipf column lengths, user ids
uniform, ratings in 0.5 steps.  One JSON line per measurement, each with every repeat, the median
and the range; every timed call follows a warm-up call of the same shape and ends in a device
synchronise:

* ``knn_cols``       the whole op (validation, transpose, norms, launch order, search);
* ``transpose``      ``csc_transpose`` alone;
* ``rnorm``          ``col_rnorm`` (hm_knn_rnorm) alone;
* ``search``         launch order + hm_knn_cols on prepared inputs;
* ``dense_topk``     ``topk_similar`` on the densified matrix (bf16 GEMM + torch.topk above 256
                     dimensions), the densification not timed; skipped when it does not fit;
                     ``agree_at_1`` is the share of items whose best neighbour is the same;
* ``cpu_twin``       ``knn_cols`` on CPU tensors at ``--cpu-threads`` threads."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hivemall_amd.ops import knn_sparse as K  # noqa: E402


def synth(items: int, users: int, nnz: int, seed: int, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    w = (torch.arange(items, dtype=torch.float64, device=dev) + 31.0) ** -0.9
    lens = torch.clamp((w / w.sum() * nnz).round().long(), 1, users // 2)
    col = torch.repeat_interleave(torch.arange(items, device=dev), lens)
    usr = torch.randint(users, (col.numel(),), generator=g, device=dev)
    key = torch.unique(col * users + usr)                   # sorted: by column, then user
    col, rows = key // users, (key % users).to(torch.int32)
    colptr = torch.zeros(items + 1, dtype=torch.int64, device=dev)
    colptr[1:] = torch.cumsum(torch.bincount(col, minlength=items), 0)
    vals = torch.randint(1, 11, (rows.numel(),), generator=g, device=dev).double() * 0.5
    return colptr, rows, vals


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def timed(fn, reps, dev):
    fn()                                                    # warm-up, same shape
    sync(dev)
    ts = []
    out = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        sync(dev)
        ts.append(time.perf_counter() - t0)
    return ts, out


def report(variant, ts, **extra):
    print(json.dumps({"variant": variant, "seconds": [round(t, 4) for t in ts],
                      "median_s": round(statistics.median(ts), 4), "min_s": round(min(ts), 4),
                      "max_s": round(max(ts), 4), **extra}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=27278)
    ap.add_argument("--users", type=int, default=138493)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    dev = torch.device(a.device)
    if dev.type == "cuda" and not torch.cuda.is_available():
        raise SystemExit("knn_sparse_bench: no GPU; --device cpu times the host twin instead")
    colptr, rows, vals = synth(a.items, a.users, a.nnz, a.seed, dev)
    lens = colptr[1:] - colptr[:-1]
    query = torch.arange(a.items, dtype=torch.int32, device=dev)
    tr = K.csc_transpose(colptr, rows, vals, a.users)
    work = int(K.query_work(colptr, rows, tr[0], query).sum())
    shape = {"items": a.items, "users": a.users, "nnz": int(colptr[-1]), "k": a.k,
             "max_col": int(lens.max()), "max_row": int((tr[0][1:] - tr[0][:-1]).max()),
             "products": work, "device": str(dev)}

    ts, (idx, score) = timed(lambda: K.knn_cols(colptr, rows, vals, a.k, n_rows=a.users), a.reps, dev)
    report("knn_cols", ts, **shape, items_per_s=round(a.items / statistics.median(ts), 1),
           products_per_s=round(work / statistics.median(ts), 1))
    ts_t, _ = timed(lambda: K.csc_transpose(colptr, rows, vals, a.users), a.reps, dev)
    report("transpose", ts_t)
    ts_n, rnorm = timed(lambda: K.col_rnorm(colptr, vals), a.reps, dev)
    report("rnorm", ts_n)
    ts_s, (idx2, score2) = timed(lambda: K.knn_cols_prepared(colptr, rows, vals, tr, rnorm, query, a.k),
                                 a.reps, dev)
    report("search", ts_s, products_per_s=round(work / statistics.median(ts_s), 1),
           rerun_bit_identical=bool(torch.equal(idx, idx2) and torch.equal(score, score2)))

    if dev.type == "cuda" and not a.no_dense:
        from hivemall_amd.knn import topk_similar

        try:
            X = torch.zeros((a.items, a.users), dtype=torch.float32, device=dev)
            col = torch.repeat_interleave(torch.arange(a.items, device=dev), lens)
            X[col, rows.long()] = vals.float()
            ts_d, (_, di) = timed(lambda: topk_similar(X, k=a.k), a.reps, dev)
            agree = float((di[:, 0] == idx[:, 0]).double().mean())
            report("dense_topk", ts_d, dense_gib=round(X.numel() * 4 / 2**30, 2), agree_at_1=round(agree, 4))
            del X, col, di
        except torch.OutOfMemoryError as ex:
            print(json.dumps({"variant": "dense_topk", "skipped": f"out of memory: {ex}"[:200]}), flush=True)
        torch.cuda.empty_cache()

    if not a.no_cpu:
        torch.set_num_threads(a.cpu_threads)
        os.environ["OMP_NUM_THREADS"] = str(a.cpu_threads)
        cpu = torch.device("cpu")
        c_colptr, c_rows, c_vals = colptr.cpu(), rows.cpu(), vals.cpu()
        ts_c, (ci, cs) = timed(lambda: K.knn_cols(c_colptr, c_rows, c_vals, a.k, n_rows=a.users),
                               a.cpu_reps, cpu)
        report("cpu_twin", ts_c, threads=a.cpu_threads,
               idx_equal_to_device=bool(torch.equal(ci, idx.cpu())),
               max_score_diff=float((cs - score.cpu()).abs().max()))


if __name__ == "__main__":
    main()
