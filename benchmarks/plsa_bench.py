"""train_plsa epoch time: ``-engine native`` (ops/plsa.py: the per-document EM kernel and the
deterministic P(w|z) update kernels of csrc/kernels/plsa.hip) against ``-engine torch`` (tensor
ops with one host-synchronised EM loop per mini-batch) in one process on the same device.

    python benchmarks/plsa_bench.py [--docs 20000] [--vocab 50000] [--topics 64] [--words 100]
                                    [--batch 128] [--reps 5] [--epochs 1 21] [--device cuda]
                                    [--engines native torch]

Seeded corpus: every topic owns a random set of ``4 * vocab / topics`` words; a document draws
``words`` distinct words from the sets of three topics, with counts 1 + Poisson(1).  Documents are
``{word: count}`` maps, as ``train_plsa`` receives them.

``PLSA.fit`` also encodes the vocabulary on the host, the same work in both engines, so an epoch is
timed as the difference between two fits: ``(t(fit, e2 epochs) - t(fit, e1 epochs)) / (e2 - e1)``
with ``-delta`` and ``-max_inner_iters`` at their defaults.  The host part of a fit varies by about
0.1 s between calls, hence twenty epochs between the two.  A warm-up fit of every shape comes
first, the engines alternate inside every repeat, every timed fit ends in a device synchronise.
One JSON line per engine (epoch seconds of every repeat, their median and spread, whole-fit
seconds) and a last line with the ratio of the medians and the shape the run actually had."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hivemall_amd.models.topicmodel import PLSA  # noqa: E402


def corpus(docs: int, vocab: int, topics: int, words: int, seed: int):
    rng = np.random.default_rng(seed)
    own = max(words, 4 * vocab // topics)
    sets = [rng.choice(vocab, size=own, replace=False) for _ in range(topics)]
    names = [f"w{i}" for i in range(vocab)]
    out = []
    for _ in range(docs):
        pool = np.unique(np.concatenate([sets[k] for k in rng.choice(topics, size=3, replace=False)]))
        ids = rng.choice(pool, size=min(words, len(pool)), replace=False)
        cnt = 1.0 + rng.poisson(1.0, size=len(ids))
        out.append({names[i]: float(c) for i, c in zip(ids, cnt)})
    return out


def timed_fit(engine: str, epochs: int, docs, a, dev):
    m = PLSA(f"-topics {a.topics} -iters {epochs} -mini_batch_size {a.batch} -seed 1 -engine {engine}", device=dev)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    m.fit(docs)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=20000)
    ap.add_argument("--vocab", type=int, default=50000)
    ap.add_argument("--topics", type=int, default=64)
    ap.add_argument("--words", type=int, default=100)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epochs", type=int, nargs=2, default=[1, 21])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--engines", nargs="+", default=["native", "torch"], choices=["native", "torch"],
                    help="one engine alone is for a profiler run: no ratio line")
    a = ap.parse_args()
    dev = torch.device(a.device)
    if dev.type == "cuda" and not torch.cuda.is_available():
        raise SystemExit("plsa_bench: no GPU; --device cpu times the host twins instead")
    e1, e2 = a.epochs
    if not 0 < e1 < e2:
        raise SystemExit("plsa_bench: --epochs needs 0 < e1 < e2")
    docs = corpus(a.docs, a.vocab, a.topics, a.words, a.seed)
    engines = tuple(dict.fromkeys(a.engines))
    for eng in engines:                                     # warm-up: code load, allocator, all shapes
        timed_fit(eng, 1, docs, a, dev)
    epoch = {e: [] for e in engines}
    whole = {e: [] for e in engines}
    model = {}
    for _ in range(a.reps):
        for eng in engines:
            t1, _ = timed_fit(eng, e1, docs, a, dev)
            t2, model[eng] = timed_fit(eng, e2, docs, a, dev)
            epoch[eng].append((t2 - t1) / (e2 - e1))
            whole[eng].append(t2)
    shape = {"docs": len(docs), "vocab_seen": int(model[engines[0]].pwz.shape[1]), "topics": a.topics,
             "nnz": int(sum(len(d) for d in docs)), "mean_words": round(sum(len(d) for d in docs) / len(docs), 1),
             "batch": a.batch, "device": str(dev)}
    med = {}
    for eng in engines:
        ts = epoch[eng]
        med[eng] = statistics.median(ts)
        print(json.dumps({"engine": eng, "epoch_s": [round(t, 4) for t in ts], "epoch_s_median": round(med[eng], 4),
                          "epoch_s_min": round(min(ts), 4), "epoch_s_max": round(max(ts), 4),
                          f"fit_{e2}_epochs_s": [round(t, 3) for t in whole[eng]],
                          "docs_per_s": round(len(docs) / med[eng])}), flush=True)
    if len(engines) < 2:
        print(json.dumps(shape), flush=True)
        return
    diff = float((model["native"].pwz - model["torch"].pwz).abs().max())
    print(json.dumps({"native_over_torch_epoch": round(med["torch"] / med["native"], 2), **shape,
                      "epochs_differenced": [e1, e2], "reps": a.reps,
                      "max_abs_pwz_diff_between_engines": diff}), flush=True)


if __name__ == "__main__":
    main()
