"""train_kpa: the native engine ``ops.kpa`` (csrc/kernels/kpa.hip), kernel by kernel, against the
per-row Python learner it replaces.

    python benchmarks/kpa_bench.py [--shapes criteo,short] [--reps 5] [--python-rows 2000]

Needs a GPU.  Seeded, no files read.  Two shapes:

* ``criteo``  65,536 rows of 39 entries, one name per field, the field's value Zipf-distributed over
              2^20 names in all (741 pairs a row);
* ``short``   262,144 rows of 8 entries out of 4,096 names with Zipf popularity (28 pairs a row).

One JSON line per measurement with every repeat, min, median and max and rows/s.  Kernel times are
device events around synchronised work on the current stream, each after a warm-up call of the
same shape:

* ``encode``  the host-side parse and CSR build (host clock; one run);
* ``table``   kernel A and the rank by first occurrence (``build_table``);
* ``train``   kernel B, one epoch (``train``);
* ``score``   kernel C over the encoded training rows (the launch only);
* ``python``  ``KPA('-engine python')`` on the first ``--python-rows`` rows (host clock), with the
              largest deviation of the native weights from it on that prefix."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"criteo": (65536, 39, 1 << 20), "short": (262144, 8, 4096)}


def corpus(shape: str, n: int, seed: int):
    """``(features, labels)``: ``n`` rows of ``name:value`` strings, distinct names inside a row."""
    import numpy as np

    _, entries, names = SHAPES[shape]
    rng = np.random.default_rng([seed, entries])
    vals = rng.uniform(-1, 1, (n, entries)).round(6)
    if shape == "criteo":
        per = names // entries
        p = 1.0 / np.arange(1, per + 1)
        ids = rng.choice(per, size=(n, entries), p=p / p.sum())
        feats = [[f"c{f}_{i}:{v}" for f, (i, v) in enumerate(zip(ri, rv))] for ri, rv in zip(ids.tolist(), vals.tolist())]
    else:
        p = 1.0 / np.arange(1, names + 1)
        p /= p.sum()
        ids = rng.choice(names, size=(n, entries), p=p)
        # distinct names inside a row: a repeated draw is dropped, so a few rows run short
        feats = [[f"f{i}:{v}" for i, v in zip(dict.fromkeys(ri), rv)] for ri, rv in zip(ids.tolist(), vals.tolist())]
    return feats, rng.integers(0, 2, n).tolist()


def report(variant, ts, rows, **extra):
    med = statistics.median(ts)
    print(json.dumps({"variant": variant, "seconds": [round(t, 6) for t in ts], "min_s": round(min(ts), 6),
                      "median_s": round(med, 6), "max_s": round(max(ts), 6), "rows": rows,
                      "rows_per_s": round(rows / max(med, 1e-12), 1), **extra}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="criteo,short")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--python-rows", type=int, default=2000)
    ap.add_argument("--rows", type=int, default=0, help="rows of every shape (0 = the shape's own)")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch

    from hivemall_amd import _native
    from hivemall_amd.models.recommend import KPA
    from hivemall_amd.ops import kpa as K

    if not torch.cuda.is_available():
        raise SystemExit("kpa_bench: no GPU")
    dev = torch.device("cuda")

    def timed(fn):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    def repeat(fn):
        fn()                                                # warm-up, same shape
        runs = [timed(fn) for _ in range(a.reps)]
        return [t for t, _ in runs], runs[-1][1]

    c, pkc = 1.0, 1.0
    for shape in a.shapes.split(","):
        n = a.rows or SHAPES[shape][0]
        feats, y = corpus(shape, n, a.seed)
        vocab: dict = {}
        t0 = time.perf_counter()
        rows = K.encode(feats, y, vocab, device=dev)
        torch.cuda.synchronize(dev)
        tag = {"shape": shape, "entries": SHAPES[shape][1], "names": len(vocab), "pair_occurrences": rows.n_occ}
        report("encode", [time.perf_counter() - t0], n, **tag)

        ts, table = repeat(lambda: K.build_table(rows))
        tag["slots"] = table.slots
        report("table", ts, n, capacity=table.keys.numel(), chunks=table.chunks, **tag)
        ts, (w0, w1, w2, w3) = repeat(lambda: K.train(rows, table, len(vocab), iters=1, c=c, pkc=pkc))
        report("train", ts, n, us_per_row=round(statistics.median(ts) / n * 1e6, 3), **tag)
        out = torch.zeros(n, dtype=torch.float64, device=dev)
        p = _native.ptr
        ts, _ = repeat(lambda: _native.call_hip(
            "hm_kpa_score", dev, p(rows.ptr), p(rows.ids), p(rows.vals), n, p(table.keys), p(table.remap),
            table.cap_mask, p(w0), p(w1), p(w2), p(w3), pkc, math.sqrt(2 * pkc), math.sqrt(2), p(out)))
        report("score", ts, n, **tag)

        k = min(a.python_rows, n)
        t0 = time.perf_counter()
        ref = KPA(f"-engine python -c {c} -pkc {pkc}", device="cpu").fit(feats[:k], y[:k])
        dt = time.perf_counter() - t0
        m = K.fit(feats[:k], y[:k], iters=1, c=c, pkc=pkc, device=dev)
        d1, d2, d3 = m.dicts()
        dev_max = max(max((abs(g[key] - want[key]) / max(1.0, abs(want[key])) for key in want), default=0.0)
                      for g, want in ((d1, ref.w1), (d2, ref.w2), (d3, ref.w3)))
        same_keys = list(d3) == list(ref.w3) and list(d1) == list(ref.w1)
        report("python", [dt], k, us_per_row=round(dt / k * 1e6, 1), max_weight_deviation=dev_max,
               same_keys=same_keys, **{kk: v for kk, v in tag.items() if kk in ("shape", "entries")})
        del rows, table, w0, w1, w2, w3, out


if __name__ == "__main__":
    main()
