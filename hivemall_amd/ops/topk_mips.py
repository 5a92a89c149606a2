"""Fused top-k maximum inner product search (``csrc/kernels/topk_mips.hip``; ``k`` up to 256).

``mips_topk(Q, I, k)`` returns, for every query row, the ``k`` items with the largest
``<Q[q], I[n]> + item_bias[n]`` (+ ``row_bias[q]`` on the returned scores), best first,
optionally excluding a per-query sorted item list (already-seen items, Hivemall's
``populate_not_in``) and/or the query's own index (item-item kNN).

On ``cuda`` tensors this is one gfx950 kernel: bf16 MFMA score tiles filtered against a
running per-row top-k in LDS — the M x N score matrix never reaches HBM.  CPU tensors use a
blocked fp32 ``matmul`` + ``topk`` with the same contract (and tie order: higher score first,
then lower item index).

``precision="bf16"`` (the default) rounds both operand tables to bf16 before the sweep: scores
carry about 2^-9 relative error per product and the ranking is the ranking of those scores.
``precision="fp32"`` runs the fp32 MFMA kernels of ``csrc/kernels/topk_mips_f32.hip`` on the
tables as they are: fp32 products, fp32 accumulation, the ranking of the fp32 scores.

``k <= 64`` runs the kernels of those two files; ``k`` in 65..256 runs
``csrc/kernels/topk_mips_wide.hip`` (the same score tiles, a per-row buffer of 64-bit keys in LDS
compacted by a bitonic sort), for either precision and with the same contract.

This is the fused form of the reference's recommendation query
``each_top_k(k, user, mf_predict(...) / bprmf_predict(...), item)`` over the user x item
join (core/src/main/java/hivemall/tools/EachTopKUDTF.java, mf/MFPredictionUDF.java,
mf/BPRMFPredictionUDF.java; SURVEY.md §2.3.5 kernel K8) and of cosine-similarity kNN
(knn/similarity/CosineSimilarityUDF.java).
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _native

_P = C.c_void_p
_native.register_hip("hm_mips_topk", [C.c_int] * 7 + [_P] * 7 + [_P])
_native.register_hip("hm_mips_topk_f32", [C.c_int] * 7 + [_P] * 7 + [_P])
_native.register_hip("hm_mips_topk_wide", [C.c_int] * 7 + [_P] * 7 + [_P])
_native.register_hip("hm_mips_topk_wide_f32", [C.c_int] * 7 + [_P] * 7 + [_P])

KMAX = 256
_K_NARROW = 64              # up to here the register / 96-slot kernels; above, topk_mips_wide.hip
_KD = (32, 64, 128, 256)
_KD_F32 = (16, 32, 64, 128, 256)
PRECISIONS = ("bf16", "fp32")


def _pad_bf16(x: torch.Tensor, kd: int) -> torch.Tensor:
    out = torch.zeros(x.shape[0], kd, dtype=torch.bfloat16, device=x.device)
    out[:, : x.shape[1]] = x.to(torch.bfloat16)
    return out.contiguous()


def _pad_f32(x: torch.Tensor, kd: int) -> torch.Tensor:
    if x.shape[1] == kd and x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 16 == 0:
        return x                                         # the kernel reads rows as 16-B chunks
    out = torch.zeros(x.shape[0], kd, dtype=torch.float32, device=x.device)
    out[:, : x.shape[1]] = x
    return out


def exclusion_csr(rows, items, n_rows: int, device=None):
    """(query row, item) pairs -> (ptr int64 [n_rows+1], items sorted per row int32)."""
    r = torch.as_tensor(rows, device=device).long()
    i = torch.as_tensor(items, device=device).long()
    key = torch.unique(r * (1 << 32) + i)
    rr = key >> 32
    ii = (key & 0xFFFFFFFF).to(torch.int32)
    ptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=r.device)
    ptr[1:] = torch.cumsum(torch.bincount(rr, minlength=n_rows), 0)
    return ptr.contiguous(), ii.contiguous()


def _splits_for(M: int, N: int, sms: int) -> int:
    blocks = (M + 63) // 64
    s = 1
    # at least ~4 blocks per CU, each split still sweeping >= 8 tiles of 64 items
    while blocks * s < 4 * sms and N // (64 * s * 2) >= 8:
        s *= 2
    return s


def _splits_for_wide(M: int, N: int, k: int, sms: int) -> int:
    """Splits of the wide kernels (k > 64): one block a CU (64 rows, 32 above k = 128), and a
    split is worth merging only while it sweeps at least 4 k (and 512) items."""
    blocks = (M + 63) // 64 if k <= 128 else (M + 31) // 32
    s = 1
    while blocks * s < 2 * sms and N // (s * 2) >= max(512, 4 * k):
        s *= 2
    return s


def _merge(idx: torch.Tensor, sc: torch.Tensor, k: int):
    """[S, M, k] partial results -> [M, k] (score desc, index asc)."""
    S, M, _ = idx.shape
    idx = idx.permute(1, 0, 2).reshape(M, S * k)
    sc = sc.permute(1, 0, 2).reshape(M, S * k)
    # lexicographic (score desc, idx asc): sort by idx first, then stable sort by score
    big = torch.where(idx < 0, torch.full_like(idx, 2**31 - 1), idx)
    o = torch.argsort(big, dim=1, stable=True)
    idx, sc = idx.gather(1, o), sc.gather(1, o)
    o = torch.argsort(sc, dim=1, descending=True, stable=True)[:, :k]
    return idx.gather(1, o), sc.gather(1, o)


def mips_topk(Q: torch.Tensor, I: torch.Tensor, k: int, item_bias: torch.Tensor | None = None,
              row_bias: torch.Tensor | None = None, exclude: tuple | None = None,
              exclude_self_offset: int | None = None, splits: int | None = None,
              precision: str = "bf16"):
    """Top-``k`` items per query row; returns (indices int64 [M,k], scores fp32 [M,k]).
    Missing entries (fewer than k admissible items) are index -1 / score -inf.

    precision: operand type of the GPU kernel, ``"bf16"`` or ``"fp32"`` (CPU tensors always
    run in fp32).

    exclude: (ptr int64 [M+1], items int32 sorted per row) from ``exclusion_csr``.
    exclude_self_offset: drop item ``q + offset`` for query ``q`` (0 for Q is I)."""
    M, d = Q.shape
    N, d2 = I.shape
    if d != d2:
        raise ValueError(f"mips_topk: dimension mismatch {d} vs {d2}")
    if not 0 < k <= KMAX:
        raise ValueError(f"mips_topk: k must be in 1..{KMAX}")
    if precision not in PRECISIONS:
        raise ValueError(f"mips_topk: precision must be one of {PRECISIONS}, got {precision!r}")
    if Q.is_cuda:
        return _mips_gpu(Q, I, k, item_bias, row_bias, exclude, exclude_self_offset, splits, precision)
    return _mips_cpu(Q, I, k, item_bias, row_bias, exclude, exclude_self_offset)


def _mips_gpu(Q, I, k, item_bias, row_bias, exclude, self_off, splits, precision="bf16"):
    dev = Q.device
    M, d = Q.shape
    N = I.shape[0]
    kds = _KD_F32 if precision == "fp32" else _KD
    kd = next((x for x in kds if x >= d), None)
    if kd is None:
        raise ValueError(f"mips_topk: dimension {d} > {kds[-1]}")
    wide = k > _K_NARROW
    if precision == "fp32":
        entry = "hm_mips_topk_wide_f32" if wide else "hm_mips_topk_f32"
        Qb, Ib = _pad_f32(Q, kd), _pad_f32(I.to(dev), kd)
    else:
        entry = "hm_mips_topk_wide" if wide else "hm_mips_topk"
        Qb, Ib = _pad_bf16(Q, kd), _pad_bf16(I.to(dev), kd)
    bias = item_bias.to(device=dev, dtype=torch.float32).contiguous() if item_bias is not None else None
    if splits is None:
        sms = torch.cuda.get_device_properties(dev).multi_processor_count
        splits = _splits_for_wide(M, N, k, sms) if wide else _splits_for(M, N, sms)
    ex_ptr = ex_idx = None
    if exclude is not None:
        ex_ptr, ex_idx = (t.to(dev).contiguous() for t in exclude)
        if ex_ptr.dtype != torch.int64 or ex_idx.dtype != torch.int32 or ex_ptr.numel() != M + 1:
            raise ValueError("mips_topk: exclude must be (int64 ptr [M+1], int32 items)")
    oi = torch.empty(splits, M, k, dtype=torch.int32, device=dev)
    os_ = torch.empty(splits, M, k, dtype=torch.float32, device=dev)
    p = _native.ptr
    rc = getattr(_native.hip(), entry)(M, N, kd, k, splits, int(self_off is not None), int(self_off or 0),
                                       p(Qb), p(Ib), p(bias), p(ex_ptr), p(ex_idx), p(oi), p(os_),
                                       _native.stream_of(dev))
    _native.check(rc, entry)
    if splits > 1:
        idx, sc = _merge(oi, os_, k)
    else:
        idx, sc = oi[0], os_[0]
    idx = idx.long()
    if row_bias is not None and row_bias.dtype == torch.float64:
        # an fp64 row bias is added in fp64 and rounded once (the fp32 callers pass mu + b_u so)
        sc = torch.where(idx >= 0, (sc.double() + row_bias.to(dev)[:, None]).float(), sc)
    elif row_bias is not None:
        sc = torch.where(idx >= 0, sc + row_bias.to(dev, torch.float32)[:, None], sc)
    return idx, sc


def _mips_cpu(Q, I, k, item_bias, row_bias, exclude, self_off, block: int = 4096):
    M = Q.shape[0]
    N = I.shape[0]
    Qf, If = Q.float(), I.float()
    out_i = torch.full((M, k), -1, dtype=torch.int64)
    out_s = torch.full((M, k), -float("inf"))
    for r0 in range(0, M, block):
        r1 = min(M, r0 + block)
        S = Qf[r0:r1] @ If.T
        if item_bias is not None:
            S += item_bias.float()[None, :]
        if self_off is not None:
            cols = torch.arange(r0, r1) + self_off
            ok = (cols >= 0) & (cols < N)
            S[torch.nonzero(ok).flatten(), cols[ok]] = -float("inf")
        if exclude is not None:
            ptr, ex = exclude
            ptr = ptr.cpu()
            lo, hi = int(ptr[r0]), int(ptr[r1])
            rows = torch.repeat_interleave(torch.arange(r1 - r0), (ptr[r0 + 1: r1 + 1] - ptr[r0:r1]))
            S[rows, ex.cpu()[lo:hi].long()] = -float("inf")
        # (score desc, index asc): topk over a stably index-ordered matrix
        kk = min(k, N)
        o = torch.argsort(S, dim=1, descending=True, stable=True)[:, :kk]
        sc = S.gather(1, o)
        o = torch.where(torch.isinf(sc) & (sc < 0), torch.full_like(o, -1), o)
        out_i[r0:r1, :kk] = o
        out_s[r0:r1, :kk] = sc
    if row_bias is not None:
        out_s = torch.where(out_i >= 0, out_s + row_bias.float()[:, None], out_s)
    return out_i, out_s
