"""Segmented top-k (``csrc/kernels/each_top_k.hip``, ``csrc/host/each_top_k_cpu.cpp``): the engine
behind ``knn.each_top_k`` / ``knn.each_top_k_batch``.

Contract (``docs/compat.md`` "each_top_k engine"; ``knn._each_top_k_python`` is the definition).

* A group is every row with the same code, adjacent or not; groups come out by code.
* Inside a group the rows are ordered by the pair (score in the chosen direction, input position):
  ``largest`` puts the highest score first, otherwise the lowest; equal scores keep input order
  either way; ``-0.0`` and ``0.0`` are equal; the infinities are ordinary values.  NaN is refused.
* The first ``min(k, group size)`` rows of every group are kept.

No two rows share a pair, so the result is one integer array, the same from the kernels, the twin
and ``np.lexsort((arange(n), -score if largest else score, codes))`` cut at rank ``< k``.

``cuda`` tensors run the gfx950 kernels on the current stream: groups of up to ``WAVE_SEG_MAX``
rows one wave each, longer ones cut into work items of ``chunk`` rows whose best ``k`` are
selected again, level after level, until one item holds the group.  CPU tensors run the OpenMP
twin in one pass; with an explicit ``chunk`` they run the same levels through the twin's work-item
form, so the level plan is checked where there is no GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _native
from . import _args

_P = C.c_void_p
_I64 = _native.c_i64
_native.register_hip("hm_each_top_k", [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P])
_native.register_hip("hm_each_top_k_items", [_P] * 8 + [_I64, C.c_int, C.c_int, _P, _P, _P, _P])
_native.register_host("hm_each_top_k_cpu", [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _I64, _P])
_native.register_host("hm_each_top_k_items_cpu", [_P] * 8 + [_I64, C.c_int, C.c_int, _P, _P, _P])

K_MAX = 128                 # ETK_KMAX
WAVE_SEG_MAX = 256          # ETK_WAVE_SEG_MAX: up to here a group is one wave's
# A level turns L rows into at most (L / chunk + 1) * k candidates: with chunk >= 16 * K_MAX it
# shrinks a group at least 16-fold (beyond 2 * chunk rows), so 2^31 rows are 4 levels at the
# default and at most 8 at the minimum.
CHUNK_MIN = 16 * K_MAX
CHUNK_MAX = 1 << 24
CHUNK_DEFAULT = 16384       # 16 rounds of the kernel's 1024 rows per work item
N_MAX = 2**31 - 1

# what the last calls did (the tests assert the path taken, not its timing)
STATS = {"calls": 0, "perm": 0, "no_perm": 0, "levels": 0, "items": 0}


def supports(k) -> bool:
    """Whether ``|k|`` is in the engine's range."""
    try:
        return not isinstance(k, bool) and 1 <= abs(int(k)) <= K_MAX
    except (TypeError, ValueError):
        return False


def _plan_level(begin, length, dst_final, k: int, chunk: int):
    """One level over the open groups (numpy int64 arrays: first position, length, output
    offset).  Returns the work items ``[4, W]`` (begin, end, dst, final), the size of the
    candidate buffer they fill, and the groups still open afterwards."""
    nch = -(-length // chunk)
    first = np.cumsum(nch) - nch
    seg = np.repeat(np.arange(len(nch), dtype=np.int64), nch)
    idx = np.arange(int(nch.sum()), dtype=np.int64) - first[seg]
    ib = begin[seg] + idx * chunk
    ie = np.minimum(ib + chunk, (begin + length)[seg])
    final = nch[seg] == 1
    cnt = np.where(final, 0, np.minimum(ie - ib, k))
    coff = np.cumsum(cnt) - cnt
    items = np.stack([ib, ie, np.where(final, dst_final[seg], coff), final.astype(np.int64)])
    keep = nch > 1
    nxt_len = np.bincount(seg, weights=cnt, minlength=len(nch)).astype(np.int64)
    return np.ascontiguousarray(items), int(cnt.sum()), (coff[first[keep]], nxt_len[keep], dst_final[keep])


def segment_topk(score: torch.Tensor, codes: torch.Tensor, n_groups: int, k: int, *,
                 largest: bool = True, chunk: int | None = None):
    """``(rows int32 [M], outptr int64 [G + 1])``: the input row of every output row, group after
    group by code and best first inside one; group ``g`` owns ``rows[outptr[g]:outptr[g + 1]]``,
    ``min(k, its size)`` rows.  ``score`` fp64 ``[n]`` without NaN, ``codes`` int32 ``[n]`` in
    ``0..n_groups-1`` in any order, on one device.  ``chunk`` (``CHUNK_MIN..CHUNK_MAX``) sets how
    many levels a long group takes and never the result."""
    _args.want("each_top_k", score, "score", torch.float64, 1)
    _args.want("each_top_k", codes, "codes", torch.int32, 1)
    _args.same_device("each_top_k", (score, codes), ("score", "codes"))
    G = _args.int_in("each_top_k", n_groups, "n_groups", 0, N_MAX)
    k = _args.int_in("each_top_k", k, "k", 1, K_MAX)
    explicit = chunk is not None
    chunk = _args.int_in("each_top_k", chunk, "chunk", CHUNK_MIN, CHUNK_MAX) if explicit else CHUNK_DEFAULT
    n = score.numel()
    if codes.numel() != n:
        raise ValueError(f"each_top_k: codes must hold {n} codes, got {codes.numel()}")
    if n > N_MAX:
        raise ValueError(f"each_top_k: {n} rows, at most 2^31 - 1")
    dev = score.device
    bad = torch.isnan(score)
    if bool(bad.any()):
        raise ValueError(f"each_top_k: score[{int(torch.nonzero(bad)[0])}] is NaN")
    if n and (int(codes.min()) < 0 or int(codes.max()) >= G):
        raise ValueError(f"each_top_k: codes must be in 0..{G - 1}")
    score, codes = score.contiguous(), codes.contiguous()

    STATS["calls"] += 1
    STATS["levels"] = STATS["items"] = 0
    perm, by_code = None, codes
    if n and bool((codes[1:] < codes[:-1]).any()):
        by_code, perm = torch.sort(codes, stable=True)
        perm = perm.to(torch.int32)
        STATS["perm"] += 1
    elif n:
        STATS["no_perm"] += 1
    # the segment bounds by binary search in the sorted codes: torch.bincount's atomics pile up on
    # a large group (docs/perf_notes.md "each_top_k")
    segptr = torch.searchsorted(by_code, torch.arange(G + 1, dtype=torch.int32, device=dev))
    lens = segptr[1:] - segptr[:-1]
    outptr = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens.clamp(max=k), 0, out=outptr[1:])
    rows = torch.empty(int(outptr[-1]), dtype=torch.int32, device=dev)
    if n == 0:
        return rows, outptr

    ptr = _native.ptr
    big = 1 if largest else 0
    if not score.is_cuda and not explicit:
        _native.call_host("hm_each_top_k", ptr(score), ptr(perm), ptr(segptr), ptr(outptr), G, k, big, 0,
                          ptr(rows))
        return rows, outptr
    if score.is_cuda:
        _native.call_hip("hm_each_top_k", dev, ptr(score), ptr(perm), ptr(segptr), ptr(outptr), G, k, big,
                         ptr(rows))
    else:
        _native.call_host("hm_each_top_k", ptr(score), ptr(perm), ptr(segptr), ptr(outptr), G, k, big,
                          WAVE_SEG_MAX, ptr(rows))
    long_ids = torch.nonzero(lens > WAVE_SEG_MAX).reshape(-1)
    if long_ids.numel() == 0:
        return rows, outptr
    open_ = (segptr[long_ids].cpu().numpy(), lens[long_ids].cpu().numpy(), outptr[long_ids].cpu().numpy())
    ckey = cpos = None
    while len(open_[0]):
        items, n_cand, open_ = _plan_level(*open_, k, chunk)
        W = items.shape[1]
        it = torch.from_numpy(items).to(dev)
        okey = torch.empty(max(n_cand, 1), dtype=torch.int64, device=dev)
        opos = torch.empty(max(n_cand, 1), dtype=torch.int32, device=dev)
        args = (ptr(score), ptr(perm), ptr(ckey), ptr(cpos), ptr(it[0]), ptr(it[1]), ptr(it[2]), ptr(it[3]),
                W, k, big, ptr(okey), ptr(opos), ptr(rows))
        if score.is_cuda:
            _native.call_hip("hm_each_top_k_items", dev, *args)
        else:
            _native.call_host("hm_each_top_k_items", *args)
        ckey, cpos = okey, opos                    # the level read the previous pair; it may go now
        STATS["levels"] += 1
        STATS["items"] += W
    return rows, outptr
