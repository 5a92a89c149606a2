"""Top-k recommendation for every user (MovieLens-20M shape) — fused MFMA kernel vs
GEMM + torch.topk.

    python benchmarks/mips_bench.py [--users 138493] [--items 27278] [--dim 64] [--k 10]
                                    [--precision bf16|fp32]

Prints one JSON line per variant: ms per full sweep, effective TFLOP/s of the score GEMM,
and agreement of the fused result with the unfused one (fraction of identical top-k sets).
Synthetic random-init factors (bf16 operands, fp32 accumulation in both variants).

``--precision fp32`` builds fp32 operands and times four variants, alternating them over
``--repeats`` rounds in this one process: the fused fp32 MFMA kernel, a chunked fp32 ``matmul``
+ ``torch.topk`` (the route the fp32 kernel replaces, and its yardstick), the fused bf16
kernel on the same tables and the chunked bf16 ``matmul`` + ``torch.topk``.  Each line carries
the median, the fastest and the slowest round.  ``--k`` up to 256: above 64 the fused variants
are the kernels of ``csrc/kernels/topk_mips_wide.hip``."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hivemall_amd.ops.topk_mips import mips_topk  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out


def main_fp32(a):
    """Fused fp32 kernel against fp32 GEMM + topk and the fused bf16 kernel, alternating."""
    import statistics

    dev = torch.device("cuda")
    torch.backends.cuda.matmul.allow_tf32 = False
    g = torch.Generator(device=dev).manual_seed(0)
    U = torch.randn(a.users, a.dim, device=dev, generator=g) * 0.3
    V = torch.randn(a.items, a.dim, device=dev, generator=g) * 0.3
    bias = torch.randn(a.items, device=dev, generator=g) * 0.05
    flop = 2.0 * a.users * a.items * a.dim

    def unfused():
        outs_i, outs_s = [], []
        for r0 in range(0, a.users, a.chunk):
            t = torch.topk(U[r0:r0 + a.chunk] @ V.T + bias[None, :], a.k, dim=1)
            outs_i.append(t.indices)
            outs_s.append(t.values)
        return torch.cat(outs_i), torch.cat(outs_s)

    Ub, Vb = U.bfloat16(), V.bfloat16()

    def unfused_bf16():                      # BPRMF.recommend_topk's route above topk_mips.KMAX
        outs_i, outs_s = [], []
        for r0 in range(0, a.users, a.chunk):
            t = torch.topk((Ub[r0:r0 + a.chunk] @ Vb.T).float() + bias[None, :], a.k, dim=1)
            outs_i.append(t.indices)
            outs_s.append(t.values)
        return torch.cat(outs_i), torch.cat(outs_s)

    variants = {
        "fused_fp32_mfma_topk": lambda: mips_topk(U, V, a.k, item_bias=bias, precision="fp32"),
        "gemm_fp32+torch.topk": unfused,
        "fused_bf16_mfma_topk": lambda: mips_topk(U, V, a.k, item_bias=bias, precision="bf16"),
        "gemm_bf16+torch.topk": unfused_bf16,
    }
    ms = {n: [] for n in variants}
    out = {}
    for _ in range(a.repeats):
        for n, fn in variants.items():       # timed() warms each variant before its window
            t, out[n] = timed(fn, a.reps)
            ms[n].append(t)
    fi, fs = out["fused_fp32_mfma_topk"]
    ui, us = out["gemm_fp32+torch.topk"]
    same = (torch.sort(fi, 1).values == torch.sort(ui, 1).values).all(1).float().mean().item()
    med = {n: statistics.median(v) for n, v in ms.items()}
    for n, v in ms.items():
        rec = {"variant": n, "ms": round(med[n], 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3),
               "tflops": round(flop / med[n] / 1e9, 1), "users": a.users, "items": a.items, "dim": a.dim,
               "k": a.k, "repeats": a.repeats, "reps": a.reps}
        if n == "gemm_fp32+torch.topk":
            rec.update(speedup_fused_fp32=round(med[n] / med["fused_fp32_mfma_topk"], 2),
                       same_topk_set_frac=round(same, 4), max_score_diff=(fs - us).abs().max().item())
        if n == "gemm_bf16+torch.topk":
            rec.update(speedup_fused_bf16=round(med[n] / med["fused_bf16_mfma_topk"], 2))
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138493)
    ap.add_argument("--items", type=int, default=27278)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=32768, help="user rows per GEMM+topk chunk")
    ap.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--repeats", type=int, default=5, help="alternating rounds (--precision fp32)")
    a = ap.parse_args()
    if a.precision == "fp32":
        return main_fp32(a)
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    U = (torch.randn(a.users, a.dim, device=dev, generator=g) * 0.3).bfloat16()
    V = (torch.randn(a.items, a.dim, device=dev, generator=g) * 0.3).bfloat16()
    bias = torch.randn(a.items, device=dev, generator=g) * 0.05
    flop = 2.0 * a.users * a.items * a.dim

    ms, (fi, fs) = timed(lambda: mips_topk(U, V, a.k, item_bias=bias), a.reps)
    print(json.dumps({"variant": "fused_mfma_topk", "ms": round(ms, 3), "tflops": round(flop / ms / 1e9, 1),
                      "users": a.users, "items": a.items, "dim": a.dim, "k": a.k}), flush=True)

    def unfused():
        outs_i, outs_s = [], []
        for r0 in range(0, a.users, a.chunk):
            S = (U[r0:r0 + a.chunk] @ V.T).float() + bias[None, :]
            t = torch.topk(S, a.k, dim=1)
            outs_i.append(t.indices)
            outs_s.append(t.values)
        return torch.cat(outs_i), torch.cat(outs_s)

    ms2, (ui, us) = timed(unfused, a.reps)
    same = (torch.sort(fi, 1).values == torch.sort(ui, 1).values).all(1).float().mean().item()
    err = (fs - us).abs().max().item()
    print(json.dumps({"variant": "gemm_bf16+torch.topk", "ms": round(ms2, 3), "tflops": round(flop / ms2 / 1e9, 1),
                      "speedup_fused": round(ms2 / ms, 2), "same_topk_set_frac": round(same, 4),
                      "max_score_diff": err}), flush=True)


if __name__ == "__main__":
    main()
