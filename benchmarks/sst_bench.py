"""``sst`` change-point scores: the native engine ``ops.sst.sst_scores`` (csrc/kernels/sst.hip)
against its OpenMP twin and against the per-point NumPy / LAPACK loop of ``sst -engine numpy``.

    python benchmarks/sst_bench.py [--n 1048576] [--batch 1024 4096] [--w 30] [--reps 5]
                                   [--cpu-n 65536] [--cpu-threads 16] [--numpy-n 8192]
                                   [--no-cpu] [--no-numpy]

Needs a GPU.  The series are seeded noisy sines with a frequency change every 1000 samples.  One
JSON line per measurement with every repeat, min, median and max, and the time per scored point;
every timed call follows a warm-up call of the same shape and ends in a device synchronise:

* ``series``    one series of ``--n`` samples on the GPU (validation, launch, sweep-cap check);
* ``batch``     ``S x N`` series in one launch;
* ``cpu_twin``  the twin on one series of ``--cpu-n`` samples, with its largest difference from
                the kernel on the same samples; at ``OMP_NUM_THREADS`` threads where the
                environment sets it, at ``--cpu-threads`` otherwise (the line reports which);
* ``numpy``     ``sst(x, "-engine numpy")`` on ``--numpy-n`` samples (one run: it is a Python
                loop of three LAPACK calls per point)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def series(S: int, N: int, seed: int):
    import numpy as np

    rng = np.random.default_rng(seed)
    t = np.arange(N)
    freq = rng.uniform(1.0, 6.0, size=(S, N // 1000 + 1))[:, t // 1000]
    return np.sin(t / freq) + rng.normal(0, 0.1, size=(S, N))


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


def report(variant, ts, points, **extra):
    med = statistics.median(ts)
    print(json.dumps({"variant": variant, "seconds": [round(t, 4) for t in ts],
                      "min_s": round(min(ts), 4), "median_s": round(med, 4), "max_s": round(max(ts), 4),
                      "scored_points": points, "us_per_point": round(med / max(points, 1) * 1e6, 4),
                      **extra}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, nargs=2, default=[1024, 4096], metavar=("S", "N"))
    ap.add_argument("--w", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-n", type=int, default=1 << 16)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--numpy-n", type=int, default=1 << 13)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    # the twin's OpenMP pool is sized once, when the runtime starts: an ambient OMP_NUM_THREADS
    # is left alone and reported, --cpu-threads applies only where none is set
    os.environ.setdefault("OMP_NUM_THREADS", str(a.cpu_threads))
    threads = int(os.environ["OMP_NUM_THREADS"])
    import torch

    from hivemall_amd.ops.sst import sst_scores

    if not torch.cuda.is_available():
        raise SystemExit("sst_bench: no GPU")
    dev = torch.device("cuda")
    need = 4 * a.w
    sync = lambda: torch.cuda.synchronize(dev)              # noqa: E731

    x1 = torch.from_numpy(series(1, a.n, a.seed)[0]).to(dev)
    ts, (score1, sw) = timed(lambda: sst_scores(x1, a.w, return_sweeps=True), a.reps, sync)
    report("series", ts, a.n - need + 1, N=a.n, w=a.w, max_sweeps=int(sw.max()))
    S, N = a.batch
    xb = torch.from_numpy(series(S, N, a.seed + 1)).to(dev)
    ts, (_, sw) = timed(lambda: sst_scores(xb, a.w, return_sweeps=True), a.reps, sync)
    report("batch", ts, S * (N - need + 1), S=S, N=N, w=a.w, max_sweeps=int(sw.max()))
    del xb

    if not a.no_cpu:
        xc = x1[:a.cpu_n].cpu()
        ts, score_c = timed(lambda: sst_scores(xc, a.w), a.reps, lambda: None)
        report("cpu_twin", ts, a.cpu_n - need + 1, N=a.cpu_n, w=a.w, threads=threads,
               max_diff_to_kernel=float((score_c - score1[:a.cpu_n].cpu()).abs().max()))
    if not a.no_numpy:
        from hivemall_amd.anomaly import sst

        xn = x1[:a.numpy_n].cpu().numpy()
        t0 = time.perf_counter()
        rows = sst(xn, f"-w {a.w} -engine numpy")
        dt = time.perf_counter() - t0
        diff = max(abs(row[0] - v) for row, v in zip(rows, score1[:a.numpy_n].cpu().tolist()))
        report("numpy", [dt], a.numpy_n - need + 1, N=a.numpy_n, w=a.w, max_diff_to_kernel=diff)


if __name__ == "__main__":
    main()
