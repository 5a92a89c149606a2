"""Pairwise similarity of sparse feature lists: the native engine ``ops.pair_sim``
(csrc/kernels/pair_sim.hip) against a formulation in plain torch on the same device and against
the per-row Python functions of ``hivemall_amd.knn`` that it replaces, and the SQL cross-join query
end to end.

    python benchmarks/pair_sim_bench.py [--shapes criteo,a9a] [--reps 10] [--python-pairs 20000]
                                        [--sql-rows 384] [--no-sql]

Needs a GPU.  Seeded, no files read.  Two cross-form shapes:

* ``criteo``  4096 x 4096 lists of 39 entries: one name per field, the field's value Zipf-distributed
              over 1000 names;
* ``a9a``     1024 x 65536 lists of 14 entries out of 123 names with Zipf popularity.

One JSON line per measurement with every repeat, min, median and max and the time per pair.  Times
are device events around the calls on the current stream; every timed call follows a warm-up call
of the same shape; the engine and the torch formulation alternate, repeat by repeat, in one run.

* ``kernel_<m>``  ``pair_primitives_cross`` with the one plane ``m`` needs (the launch and its output);
* ``engine_<m>``  ``pair_measures_cross``: the kernel plus the finishing on the device;
* ``torch_<m>``   fp64 ``sparse(A) @ dense(B).T`` plus the norms; euclid as ``|a|^2 + |b|^2 - 2 dot``.
                  Its sums are in another order, so it is compared to a tolerance (``max_abs_diff``);
                  its matrices are built before the timed window, as the engine's lists are;
* ``python_<m>``  the per-row function on ``--python-pairs`` pairs (host clock; an interpreted loop),
                  in microseconds per pair, and compared with the engine on those pairs;
* ``sql_<m>``     ``SELECT each_top_k(10, t.id, m(t.features, s.features), t.id, s.id) FROM test t
                  CROSS JOIN train s`` over ``--sql-rows`` x ``--sql-rows`` rows on the native route
                  and with ``HM_SQL_BATCH_UDTF=0`` (host clock), with the share of the native time
                  that the host-side encoding (``encode_columns``) takes."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"criteo": (4096, 4096, 39), "a9a": (1024, 65536, 14)}
MEASURES = ("cosine_similarity", "euclid_distance")


def zipf_ids(rng, n_names: int, size):
    import numpy as np

    p = 1.0 / np.arange(1, n_names + 1)
    return rng.choice(n_names, size=size, p=p / p.sum())


def corpus(shape: str, n: int, seed: int):
    """``n`` feature dicts ``{name: value}`` of the shape."""
    import numpy as np

    rng = np.random.default_rng([seed, n, len(shape)])
    if shape == "criteo":
        ids = zipf_ids(rng, 1000, (n, 39))
        vals = rng.uniform(-3, 3, (n, 39))
        return [{f"c{f}_{i}": v for f, (i, v) in enumerate(zip(ri, rv))} for ri, rv in zip(ids.tolist(), vals.tolist())]
    p = 1.0 / np.arange(1, 124)
    p /= p.sum()
    out = []
    for _ in range(n):
        names = rng.choice(123, size=14, replace=False, p=p)
        out.append({f"f{i}": v for i, v in zip(names.tolist(), rng.uniform(-3, 3, 14).tolist())})
    return out


def as_strings(d: dict) -> list:
    return [f"{k}:{v!r}" for k, v in d.items()]


def report(variant, ts, pairs, **extra):
    med = statistics.median(ts)
    print(json.dumps({"variant": variant, "seconds": [round(t, 6) for t in ts], "min_s": round(min(ts), 6),
                      "median_s": round(med, 6), "max_s": round(max(ts), 6), "pairs": pairs,
                      "ns_per_pair": round(med / max(pairs, 1) * 1e9, 4), **extra}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="criteo,a9a")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--python-pairs", type=int, default=20000)
    ap.add_argument("--sql-rows", type=int, default=384)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-sql", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import pandas as pd
    import torch

    from hivemall_amd import knn
    from hivemall_amd.ops import pair_sim as ps

    if not torch.cuda.is_available():
        raise SystemExit("pair_sim_bench: no GPU")
    dev = torch.device("cuda")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    for shape in a.shapes.split(","):
        N, M, entries = SHAPES[shape]
        dicts = corpus(shape, N, a.seed) + corpus(shape, M, a.seed + 1)
        t0 = time.perf_counter()
        lists = ps.from_dicts(dicts, dev)
        torch.cuda.synchronize(dev)
        tag = {"shape": shape, "N": N, "M": M, "entries": entries, "names": len(lists.names),
               "lanes_per_pair": 8 if lists.max_len <= 8 else 16 if lists.max_len <= 16 else 32 if lists.max_len <= 32 else 64}
        report("from_dicts", [time.perf_counter() - t0], N + M, **tag)
        a_idx = torch.arange(N, dtype=torch.int32, device=dev)
        b_idx = torch.arange(N, N + M, dtype=torch.int32, device=dev)

        fns = {}
        for m in MEASURES:
            fns[f"kernel_{m}"] = lambda m=m: ps.pair_primitives_cross(lists, a_idx, b_idx, ps._MASK[m], check=False)
            fns[f"engine_{m}"] = lambda m=m: ps.pair_measures_cross(lists, a_idx, b_idx, m, check=False)
        try:
            V = len(lists.names)
            lens = lists.lengths()
            rows = torch.repeat_interleave(torch.arange(N + M, device=dev), lens)
            A_rows = rows < N
            A_sp = torch.sparse_coo_tensor(torch.stack([rows[A_rows], lists.ids[A_rows].long()]), lists.vals[A_rows],
                                           (N, V)).coalesce().to_sparse_csr()
            Bt = torch.zeros((V, M), dtype=torch.float64, device=dev)
            Bt[lists.ids[~A_rows].long(), rows[~A_rows] - N] = lists.vals[~A_rows]
            sq_a, sq_b = lists.sq[:N], lists.sq[N:]

            def torch_cosine():
                dot = torch.sparse.mm(A_sp, Bt)
                na, nb = torch.sqrt(sq_a)[:, None], torch.sqrt(sq_b)[None, :]
                return torch.where((na > 0) & (nb > 0), dot / (na * nb), 0.0)

            def torch_euclid():
                dot = torch.sparse.mm(A_sp, Bt)
                return torch.sqrt((sq_a[:, None] + sq_b[None, :] - 2.0 * dot).clamp_(min=0.0))

            torch_cosine()
            torch.cuda.synchronize(dev)
            fns["torch_cosine_similarity"] = torch_cosine
            fns["torch_euclid_distance"] = torch_euclid
        except Exception as ex:                             # noqa: BLE001 - reported, the engine is still timed
            print(json.dumps({"variant": "torch", "error": f"{type(ex).__name__}: {ex}"[:300], **tag}), flush=True)

        times = {v: [] for v in fns}
        outs = {}
        for fn in fns.values():                             # warm-up, same shape
            fn()
        torch.cuda.synchronize(dev)
        for _ in range(a.reps):                             # alternated, repeat by repeat
            for v, fn in fns.items():
                dt, out = timed(fn)
                times[v].append(dt)
                outs[v] = out if v.startswith(("engine", "torch")) else None
        for m in MEASURES:
            report(f"kernel_{m}", times[f"kernel_{m}"], N * M, **tag)
            report(f"engine_{m}", times[f"engine_{m}"], N * M, **tag)
            if f"torch_{m}" in fns:
                diff = float((outs[f"torch_{m}"] - outs[f"engine_{m}"]).abs().max())
                ratio = statistics.median(times[f"torch_{m}"]) / statistics.median(times[f"engine_{m}"])
                report(f"torch_{m}", times[f"torch_{m}"], N * M, max_abs_diff=diff,
                       torch_over_engine=round(ratio, 3), **tag)

        # the per-row functions on a sample of the same pairs
        rng = np.random.default_rng(a.seed + 2)
        n_py = min(a.python_pairs, N * M)
        pi, pj = rng.integers(0, N, n_py), rng.integers(0, M, n_py)
        strs = {}
        for i in set(pi.tolist()) | {N + j for j in set(pj.tolist())}:
            strs[i] = as_strings(dicts[i])
        for m in MEASURES:
            fn = getattr(knn, m)
            t0 = time.perf_counter()
            vals = [fn(strs[i], strs[N + j]) for i, j in zip(pi.tolist(), pj.tolist())]
            dt = time.perf_counter() - t0
            got = outs[f"engine_{m}"][torch.from_numpy(pi).to(dev), torch.from_numpy(pj).to(dev)].cpu().numpy()
            vals = np.asarray(vals)
            equal = float((vals.view(np.int64) == got.view(np.int64)).mean())
            rel = float(np.max(np.abs(vals - got) / np.maximum(np.abs(vals), 1e-300)))
            kern_us = statistics.median(times[f"engine_{m}"]) / (N * M) * 1e6
            report(f"python_{m}", [dt], n_py, us_per_pair=round(dt / n_py * 1e6, 3), engine_us_per_pair=round(kern_us, 6),
                   bit_equal_share=round(equal, 4), max_rel_diff=rel, **tag)
        del outs, lists, fns

        if not a.no_sql:
            from hivemall_amd.sql import Session

            R = a.sql_rows
            test = pd.DataFrame({"id": range(R), "features": pd.Series([as_strings(d) for d in dicts[:R]], dtype=object)})
            train = pd.DataFrame({"id": range(R), "features": pd.Series([as_strings(d) for d in dicts[N:N + R]], dtype=object)})
            s = Session(device="cuda")
            s.register("test", test)
            s.register("train", train)
            real = ps.encode_columns
            spent = [0.0]

            def clocked(*args, **kw):
                t0 = time.perf_counter()
                try:
                    return real(*args, **kw)
                finally:
                    spent[0] += time.perf_counter() - t0

            for m in MEASURES:
                q = f"SELECT each_top_k(10, t.id, {m}(t.features, s.features), t.id, s.id) FROM test t CROSS JOIN train s"
                os.environ.pop("HM_SQL_BATCH_UDTF", None)
                s.sql(q)                                    # warm-up
                ps.encode_columns = clocked
                try:
                    native = []
                    spent[0] = 0.0
                    for _ in range(3):
                        t0 = time.perf_counter()
                        got = s.sql(q)
                        native.append(time.perf_counter() - t0)
                    share = spent[0] / sum(native)
                finally:
                    ps.encode_columns = real
                os.environ["HM_SQL_BATCH_UDTF"] = "0"
                try:
                    t0 = time.perf_counter()
                    want = s.sql(q)
                    loop = time.perf_counter() - t0
                finally:
                    os.environ.pop("HM_SQL_BATCH_UDTF", None)
                same_rows = bool(got["c0"].tolist() == want["c0"].tolist() and got["c1"].tolist() == want["c1"].tolist())
                report(f"sql_{m}", native, R * R, per_row_s=round(loop, 4),
                       per_row_over_native=round(loop / statistics.median(native), 2),
                       encode_share=round(share, 3), same_rows=same_rows, shape=shape, rows=R, entries=entries)


if __name__ == "__main__":
    main()
