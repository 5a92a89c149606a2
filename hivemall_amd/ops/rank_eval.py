"""Per-row ranking measures (``csrc/kernels/rank_eval.hip``, ``csrc/host/rank_eval_cpu.cpp``): the
engine behind ``evaluation.ranking_measures_batch`` and the grouped forms of the rank UDAFs.

Contract (``docs/compat.md`` "Ranking-measures engine"; ``evaluation.metrics``'s ``*_one`` functions
and ``ranking_auc`` are the definition).

* Row ``u`` is a rank list (item ids, best first, duplicates allowed) and a truth set; ``k`` is
  ``None``, ``0`` or a positive int and cuts the list as ``rank[:k or None]`` does.
* The seven outputs are fp64 and equal the Python functions bit for bit: every one is a quotient of
  two integers, or a sum in list order of such quotients (``average_precision``), or a sum in list
  order of ``gain / log2(i + 2)`` (``ndcg``).
* ``log2(i + 2)`` and the binary ideal DCG are host tables built with ``math.log2`` and sequential
  adds (``tables``); neither the kernel nor the twin computes a logarithm.

``cuda`` tensors run the gfx950 kernel on the current stream; CPU tensors run the OpenMP twin.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from .. import _native
from . import _args

_P = C.c_void_p
_I64 = _native.c_i64
_native.register_hip("hm_rank_eval", [_P] * 8 + [_I64, _I64, C.c_int, C.c_int, C.c_int, _P, _P])
_native.register_hip("hm_rank_eval_idcg", [_P, _P, _P, _I64, _I64, _P, _P])
_native.register_host("hm_rank_eval_cpu", [_P] * 8 + [_I64, _I64, C.c_int, C.c_int, C.c_int, _P])
_native.register_host("hm_rank_eval_idcg_cpu", [_P, _P, _P, _I64, _I64, _P])

L_MAX = 1024                # RE_LMAX
K_MAX = 2**31 - 1
REL_MAX = 62                # 2 ** rel - 1 of an int64 grade, computed as ldexp(1.0, rel) - 1
PRECISION, RECALL, HITRATE, MRR, AP, NDCG, AUC = range(7)
NAMES = ("precision_at", "recall_at", "hitrate", "mrr", "average_precision", "ndcg", "auc")
ALL = (1 << 7) - 1

# what the calls did (the tests assert the path taken, not its timing)
STATS = {"calls": 0, "hip": 0, "host": 0, "idcg": 0, "table_builds": 0}

_OP = "rank_eval"
_GAIN = np.ldexp(1.0, np.arange(REL_MAX + 1)) - 1.0    # gain of grade g, exact
_tab = {"log2": np.zeros(0), "ideal": np.zeros(0), "dev": {}}


def tables(n: int):
    """``(log2tab, ideal)`` fp64 ``[>= n]`` numpy arrays: ``log2tab[i] = math.log2(i + 2)`` and
    ``ideal[m]`` = the sequential sum of ``1 / log2tab[i]`` over ``i < m`` (the ideal DCG of ``m``
    items of relevance 1).  ``np.log2`` differs from ``math.log2`` on integers, hence the loop;
    ``np.cumsum`` adds in order.  Cached and grown on demand."""
    have = len(_tab["log2"])
    if n > have:
        n = max(n, 2 * have, 2048)
        log2 = np.empty(n, dtype=np.float64)
        log2[:have] = _tab["log2"]
        log2[have:] = [math.log2(i + 2) for i in range(have, n)]
        ideal = np.zeros(n, dtype=np.float64)
        np.cumsum(1.0 / log2[:-1], out=ideal[1:])
        _tab.update(log2=log2, ideal=ideal, dev={})
        STATS["table_builds"] += 1
    return _tab["log2"], _tab["ideal"]


def _tables_on(device, n: int):
    log2, ideal = tables(n)
    key = str(device)
    if key not in _tab["dev"]:
        _tab["dev"][key] = (torch.from_numpy(log2).to(device), torch.from_numpy(ideal).to(device))
    return _tab["dev"][key]


@dataclass
class TruthIndex:
    """The truth side of ``rank_measures``, prepared once (``build_truth``) and reused every epoch:
    ``items`` int64 sorted ascending and distinct inside each row of ``rowptr`` int64 ``[U + 1]``;
    for graded truth ``gain`` fp64 aligned with ``items`` and ``idcg`` fp64 ``[nnz]`` with
    ``idcg[rowptr[u] + m - 1]`` = the ideal DCG of the row's ``m`` largest gains."""
    rowptr: torch.Tensor
    items: torch.Tensor
    gain: torch.Tensor | None
    idcg: torch.Tensor | None
    max_len: int

    @property
    def n_rows(self) -> int:
        return self.rowptr.numel() - 1

    @property
    def device(self):
        return self.items.device


def _call(name: str, dev, *args) -> None:
    if dev.type == "cuda":
        _native.call_hip(name, dev, *args)
        STATS["hip"] += 1
    else:
        _native.call_host(name, *args)
        STATS["host"] += 1


def build_truth(rowptr: torch.Tensor, items: torch.Tensor, rel: torch.Tensor | None = None) -> TruthIndex:
    """The index of a CSR truth: row ``u`` holds ``items[rowptr[u]:rowptr[u + 1]]`` in any order,
    duplicates allowed.  ``rel`` (int64, aligned with ``items``, grades ``0..62``) makes the truth
    graded with gain ``2 ** rel - 1``; of a duplicated item the last grade counts, as in a dict."""
    _args.want(_OP, rowptr, "rowptr", torch.int64, 1)
    _args.want(_OP, items, "items", torch.int64, 1)
    _args.same_device(_OP, (items, rowptr), ("items", "rowptr"))
    if rowptr.numel() < 1:
        raise ValueError(f"{_OP}: rowptr must hold at least one entry")
    nnz, U, dev = items.numel(), rowptr.numel() - 1, items.device
    if int(rowptr[0]) != 0 or int(rowptr[-1]) != nnz or bool((rowptr[1:] < rowptr[:-1]).any()):
        raise ValueError(f"{_OP}: rowptr must rise from 0 to len(items) = {nnz}")
    if rel is not None:
        _args.want(_OP, rel, "rel", torch.int64, 1)
        _args.same_device(_OP, (items, rel), ("items", "rel"))
        if rel.numel() != nnz:
            raise ValueError(f"{_OP}: rel must hold {nnz} grades, got {rel.numel()}")
        if nnz and (int(rel.min()) < 0 or int(rel.max()) > REL_MAX):
            raise ValueError(f"{_OP}: grades must be in 0..{REL_MAX}")
    rows = torch.repeat_interleave(torch.arange(U, dtype=torch.int64, device=dev), rowptr[1:] - rowptr[:-1])
    # sorted by (row, item), equal pairs in input order: two stable sorts, since an int64 item
    # leaves no room for the row in one key
    o1 = torch.sort(items, stable=True).indices
    order = o1[torch.sort(rows[o1], stable=True).indices]
    r_s, i_s = rows[order], items[order]
    last = torch.ones(nnz, dtype=torch.bool, device=dev)           # the last of every run of one pair
    if nnz > 1:
        last[:-1] = (r_s[1:] != r_s[:-1]) | (i_s[1:] != i_s[:-1])
    r_u, i_u = r_s[last], i_s[last].contiguous()
    ptr = torch.searchsorted(r_u, torch.arange(U + 1, dtype=torch.int64, device=dev)).contiguous()
    max_len = int((ptr[1:] - ptr[:-1]).max()) if U else 0
    gain = idcg = None
    if rel is not None:
        gain = torch.from_numpy(_GAIN).to(dev)[rel[order][last]].contiguous()
        # every row's gains, largest first
        g1 = torch.sort(gain, descending=True, stable=True)
        desc = g1.values[torch.sort(r_u[g1.indices], stable=True).indices].contiguous()
        idcg = torch.empty_like(gain)
        log2tab, _ = _tables_on(dev, max_len + 1)
        _call("hm_rank_eval_idcg", dev, _native.ptr(ptr), _native.ptr(desc), _native.ptr(log2tab),
              log2tab.numel(), U, _native.ptr(idcg))
        STATS["idcg"] += 1
    return TruthIndex(ptr, i_u, gain, idcg, max_len)


def check_k(k) -> int:
    """``k`` as the engine takes it: ``None`` and ``0`` are no cut."""
    return 0 if k is None else _args.int_in(_OP, k, "k", 0, K_MAX)


def rank_measures(rank: torch.Tensor, truth: TruthIndex, k=None, *, lengths: torch.Tensor | None = None,
                  measures: int = ALL, out: torch.Tensor | None = None) -> torch.Tensor:
    """fp64 ``[7, U]``: rows ``PRECISION, RECALL, HITRATE, MRR, AP, NDCG, AUC`` of every rank list.
    ``rank`` int64 ``[U, L]`` with ``1 <= L <= L_MAX`` (what ``recommend_topk`` returns); ``lengths``
    int32 ``[U]`` for ragged lists padded to ``L``; ``k`` is ``None``, ``0`` or ``1..2^31-1``.
    ``measures`` is a bit mask (``1 << NDCG | 1 << AUC``): rows it leaves out are not computed and
    keep the values of ``out`` (zeros when ``out`` is not given)."""
    _args.want(_OP, rank, "rank", torch.int64, 2)
    if not isinstance(truth, TruthIndex):
        raise ValueError(f"{_OP}: truth must be a TruthIndex (build_truth), got {type(truth).__name__}")
    U, L = rank.shape
    dev = rank.device
    if truth.device != dev:
        raise ValueError(f"{_OP}: truth is on {truth.device}, rank on {dev}")
    if truth.n_rows != U:
        raise ValueError(f"{_OP}: truth holds {truth.n_rows} rows, rank {U}")
    if not 1 <= L <= L_MAX:
        raise ValueError(f"{_OP}: rank lists must hold 1..{L_MAX} positions, got {L}")
    k = check_k(k)
    measures = _args.int_in(_OP, measures, "measures", 0, ALL)
    if lengths is not None:
        _args.want(_OP, lengths, "lengths", torch.int32, 1)
        _args.same_device(_OP, (rank, lengths), ("rank", "lengths"))
        if lengths.numel() != U:
            raise ValueError(f"{_OP}: lengths must hold {U} entries, got {lengths.numel()}")
        lengths = lengths.contiguous()
    if out is None:
        out = torch.zeros((7, U), dtype=torch.float64, device=dev)
    else:
        _args.want(_OP, out, "out", torch.float64, 2)
        _args.same_device(_OP, (rank, out), ("rank", "out"))
        if tuple(out.shape) != (7, U) or not out.is_contiguous():
            raise ValueError(f"{_OP}: out must be a contiguous [7, {U}] tensor, got shape {tuple(out.shape)}")
    STATS["calls"] += 1
    if U == 0 or measures == 0:
        return out
    rank = rank.contiguous()
    log2tab, ideal = _tables_on(dev, max(L, truth.max_len) + 1)
    ptr = _native.ptr
    _call("hm_rank_eval", dev, ptr(rank), ptr(lengths), ptr(truth.rowptr), ptr(truth.items), ptr(truth.gain),
          ptr(truth.idcg), ptr(log2tab), ptr(ideal), log2tab.numel(), U, L, k, measures, ptr(out))
    return out
