"""``changefinder`` scores: the native engine ``ops.changefinder.changefinder_scores``
(csrc/kernels/changefinder.hip) against its OpenMP twin and against the per-point Python loop of
``changefinder -engine python``.

    python benchmarks/changefinder_bench.py [--n 1048576] [--reps 5] [--cpu-threads 16]
                                            [--python-n 16384] [--no-cpu] [--no-python]

Needs a GPU.  The series are seeded noisy sines with a frequency change every 1000 samples.  The
cases are ``(S, D, k)`` = (1, 1, 7), (64, 1, 7), (1, 8, 7) and (1, 1, 32), every other option at
its default.  One JSON line per measurement with every repeat, min, median and max, and the time
per point (a point is one sample of one series, whatever D); every timed call follows a warm-up
call of the same shape and ends in a device synchronise:

* ``kernel``    the case on the GPU (validation, transposition, table upload, launches);
* ``cpu_twin``  the same tensor on the CPU, with its largest difference from the kernel in units
                of ``eps * max(1, |twin|)``; at ``OMP_NUM_THREADS`` threads where the environment
                sets it, at ``--cpu-threads`` otherwise (the line reports which).  The twin is
                sequential in time and parallel over rows, so for S * D = 1 it is one thread;
* ``python``    ``changefinder(x, "-engine python")`` on the first ``--python-n`` samples of
                series 0 (one run: it is an interpreted loop), and that time SCALED to ``--n``
                samples and S series (``scaled_s``; the loop is linear in both)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(1, 1, 7), (64, 1, 7), (1, 8, 7), (1, 1, 32)]


def series(S: int, N: int, D: int, seed: int):
    import numpy as np

    rng = np.random.default_rng(seed)
    t = np.arange(N)
    freq = rng.uniform(1.0, 6.0, size=(S, N // 1000 + 1, D))[:, t // 1000]
    return np.sin(t[None, :, None] / freq) + rng.normal(0, 0.1, size=(S, N, D))


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
    print(json.dumps({"variant": variant, "seconds": [round(t, 5) for t in ts],
                      "min_s": round(min(ts), 5), "median_s": round(med, 5), "max_s": round(max(ts), 5),
                      "points": points, "us_per_point": round(med / max(points, 1) * 1e6, 5),
                      **extra}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--python-n", type=int, default=1 << 14)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-python", action="store_true")
    a = ap.parse_args()
    # the twin's OpenMP pool is sized once, when the runtime starts: an ambient OMP_NUM_THREADS
    # is left alone and reported, --cpu-threads applies only where none is set
    os.environ.setdefault("OMP_NUM_THREADS", str(a.cpu_threads))
    threads = int(os.environ["OMP_NUM_THREADS"])
    import numpy as np
    import torch

    from hivemall_amd.ops.changefinder import changefinder_scores

    if not torch.cuda.is_available():
        raise SystemExit("changefinder_bench: no GPU")
    dev = torch.device("cuda")
    sync = lambda: torch.cuda.synchronize(dev)              # noqa: E731
    eps = float(np.finfo(np.float64).eps)

    for S, D, k in CASES:
        xc = torch.from_numpy(series(S, a.n, D, a.seed))
        xg = xc.to(dev)
        tag = {"S": S, "D": D, "N": a.n, "k": k}
        ts, (og, cg) = timed(lambda: changefinder_scores(xg, k), a.reps, sync)
        report("kernel", ts, S * a.n, **tag)
        og, cg = og.cpu(), cg.cpu()
        del xg
        if not a.no_cpu:
            ts, (oc, cc) = timed(lambda: changefinder_scores(xc, k), max(1, a.reps // 2), lambda: None)
            unit = lambda got, ref: float(((got - ref).abs()                    # noqa: E731
                                           / (eps * ref.abs().clamp(min=1.0))).max())
            report("cpu_twin", ts, S * a.n, threads=threads, rows=S * D,
                   max_units_to_kernel=[unit(og, oc), unit(cg, cc)], **tag)
        if not a.no_python:
            from hivemall_amd.anomaly import changefinder

            n = min(a.python_n, a.n)
            xs = xc[0, :n].numpy()
            xs = list(xs[:, 0]) if D == 1 else list(xs)
            t0 = time.perf_counter()
            rows = np.array(changefinder(xs, f"-k {k} -engine python"))
            dt = time.perf_counter() - t0
            got = np.stack([og[0, :n].numpy(), cg[0, :n].numpy()], 1)
            diff = float((np.abs(got - rows) / (eps * np.maximum(1.0, np.abs(rows)))).max())
            report("python", [dt], n, scaled_s=round(dt * (a.n / n) * S, 2),
                   scaled_to={"N": a.n, "S": S}, max_units_to_kernel=diff, **{**tag, "N": n, "S": 1})
        del xc, og, cg


if __name__ == "__main__":
    main()
