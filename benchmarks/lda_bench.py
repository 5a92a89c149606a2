"""train_lda fit time on one GPU, three routes in one process:

    kernel   -engine torch: the fused E-step kernel (csrc/kernels/lda.hip) inside torch ops on the
             whole [K, V] table (the default route)
    torch    the same with the E-step as torch ops too (HM_LDA_TORCH=1)
    native   -engine native: batch-sparse E[log beta], E-step with the bound and the fused M-step
             (ops/lda.py), three launches per mini-batch

    python benchmarks/lda_bench.py [--engine kernel torch native] [--docs 4000] [--vocab 20000]
                                   [--topics 100] [--reps 3]

Synthetic corpus: D docs of ~L words drawn from K planted topics over a V-word vocabulary
(20-Newsgroups-like scale).  After a warm-up fit of every route the routes alternate inside every
repeat and every timed fit (5 epochs, -eps 0) ends in a device synchronise: one JSON line per
route.  Then one line per route (``kernel``, ``native``) with the parts of one mini-batch step timed one
by one (device events, median of 50 runs each): the torch route's table passes and E-step call,
the native route's three launches."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hivemall_amd.models.topicmodel import LDA, _csr  # noqa: E402


def corpus(D=20000, V=20000, K=100, L=150, seed=0):
    rng = np.random.default_rng(seed)
    beta = rng.dirichlet(np.full(V, 0.05), size=K)
    words = [f"w{i}" for i in range(V)]
    docs = []
    for _ in range(D):
        th = rng.dirichlet(np.full(K, 0.1))
        z = rng.choice(K, size=L, p=th)
        cnt = np.bincount(z, minlength=K)
        toks = []
        for k in np.nonzero(cnt)[0]:
            toks += [words[i] for i in rng.choice(V, size=cnt[k], p=beta[k])]
        docs.append(toks)
    return docs


def fit(route, docs, K, iters, eps=""):
    os.environ["HM_LDA_TORCH"] = "1" if route == "torch" else "0"
    engine = "native" if route == "native" else "torch"
    m = LDA(f"-topics {K} -iters {iters} {eps} -mini_batch_size 256 -seed 1 -engine {engine}", device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.fit(docs)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, m


def _median_us(step, reps):
    us = []
    for i in range(reps + 5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        if i >= 5:
            us.append(a.elapsed_time(b) * 1e3)
    return round(statistics.median(us), 1)


def torch_breakdown(m, docs, K, bs=256, reps=50):
    """Median device time of each part of a mini-batch step of ``LDA.fit``'s torch route (the
    lines of that loop, one by one; ``e_step_call`` is ``LDA.e_step``: the host draw and upload of
    gamma, the offsets, a transpose copy of its own and ``hm_lda_estep``) on the first mini-batch."""
    from hivemall_amd.models.topicmodel import _flatten

    os.environ["HM_LDA_TORCH"] = "0"
    rows = m.vocab.encode(docs[:bs], add=False)
    doc, w, cnt = _flatten(rows, m.device)
    lam, B = m.lam, len(rows)
    Eb = torch.exp(m._elog(lam, 1))
    gamma, contrib = m.e_step(doc, w, cnt, B, Eb)
    sstats = torch.zeros_like(lam).index_add_(1, w, contrib.T)
    steps = {"exp_elog_table": lambda: torch.exp(m._elog(lam, 1)),
             "transpose_copy": lambda: Eb.T.contiguous(),
             "e_step_call": lambda: m.e_step(doc, w, cnt, B, Eb),
             "sstats_zeros_index_add": lambda: torch.zeros_like(lam).index_add_(1, w, contrib.T),
             "blend": lambda: (1 - 0.05) * lam + 0.05 * (m.eta + 10.0 * sstats),
             "bound_pass": lambda: (cnt * torch.log((torch.exp(m._elog(gamma, 1))[doc] * Eb[:, w].T).sum(1)
                                                    + 1e-100)).sum().double()}
    out = {"route": "kernel", "batch_docs": B, "nnz": int(w.numel()), "vocab": int(lam.shape[1])}
    out.update({name + "_us": _median_us(step, reps) for name, step in steps.items()})
    return out


def launch_breakdown(m, docs, K, bs=256, reps=50):
    """Median device time of each native launch on the first mini-batch of ``docs``."""
    from hivemall_amd.ops import lda as L

    dev = m.device
    rows = m.vocab.encode(docs[:bs], add=False)
    ptr, wid, cnt = _csr(rows, dev)
    doc_off = torch.from_numpy(ptr.astype(np.int32)).to(dev)
    perm, word_off, uniq = L.batch_index(wid, op="lda")
    wpos = L.word_positions(wid, uniq)
    lamT = m.lam.T.contiguous()
    V = lamT.shape[0]
    T = lamT.sum(0, dtype=torch.float64).float()
    scratch = L.mstep_scratch(uniq.numel(), V, K, dev)
    gamma0 = torch.full((len(rows), K), 1.0, device=dev)
    EbU = L.lda_batch_eb(uniq, lamT, T)
    contrib = L.lda_doc_estep(doc_off, wpos, cnt, EbU, gamma0.clone(), 1.0 / K, 1e-3, 100)[1]
    steps = {"lda_batch_eb": lambda: L.lda_batch_eb(uniq, lamT, T, check=False),
             "lda_doc_estep": lambda: L.lda_doc_estep(doc_off, wpos, cnt, EbU, gamma0.clone(), 1.0 / K, 1e-3, 100,
                                                      check=False),
             # rho = 0: the table keeps its values over the repeats (every row is still read and written)
             "lda_mstep": lambda: L.lda_mstep(word_off, perm, uniq, contrib, 0.0, 1.0 / K, 1.0, lamT, T, scratch,
                                              check=False)}
    out = {"route": "native", "batch_docs": len(rows), "nnz": int(wid.numel()), "batch_words": int(uniq.numel()),
           "vocab": V}
    out.update({name + "_us": _median_us(step, reps) for name, step in steps.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--engine", nargs="+", default=["kernel", "torch"], choices=["kernel", "torch", "native"])
    ap.add_argument("--docs", type=int, default=int(os.environ.get("D", 4000)))
    ap.add_argument("--topics", type=int, default=int(os.environ.get("K", 100)))
    ap.add_argument("--vocab", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lda_bench: no GPU")
    docs = corpus(D=a.docs, V=a.vocab, K=a.topics)
    routes = tuple(dict.fromkeys(a.engine))
    for r in routes:
        fit(r, docs, a.topics, 1)                               # warm-up: code load, every shape
    secs = {r: [] for r in routes}
    model = {}
    for _ in range(a.reps):
        for r in routes:
            dt, model[r] = fit(r, docs, a.topics, 5, "-eps 0")
            secs[r].append(dt)
    for r in routes:
        med = statistics.median(secs[r])
        print(json.dumps({"estep": r, "docs": a.docs, "topics": a.topics, "vocab_seen": int(model[r].lam.shape[1]),
                          "fit_5_epochs_s": [round(t, 3) for t in secs[r]], "fit_5_epochs_s_median": round(med, 3),
                          "docs_epochs_per_s": round(5 * a.docs / med),
                          "perplexity": round(float(model[r].perplexity or 0), 3)}), flush=True)
    if "kernel" in routes:
        print(json.dumps(torch_breakdown(model["kernel"], docs, a.topics)), flush=True)
    if "native" in routes:
        print(json.dumps(launch_breakdown(model["native"], docs, a.topics)), flush=True)


if __name__ == "__main__":
    main()
