"""Cosine k-nearest neighbours over the sparse columns of a CSC matrix
(``csrc/kernels/knn_sparse.hip``, ``csrc/host/knn_sparse_cpu.cpp``): the item-item similarity +
``each_top_k`` step of Hivemall's SLIM recipe, in front of ``ops.slim``.

The input is the CSC triple ``ops.slim.check_csc`` validates (columns = the vectors to compare,
e.g. items; rows = the dimensions, e.g. users) plus ``n_rows``.  For a query column ``i`` and any
other column ``j``: ``dot(i, j)`` over the common rows, ``rnorm(c) = 1 / sqrt(sum v^2)`` (0 for
an empty column), ``score(i, j) = (dot * rnorm(i)) * rnorm(j)``.  The candidates of ``i`` are the
columns ``j != i`` with ``dot(i, j) != 0``; the result holds the ``k`` best under "score
descending, then column id ascending", padded with ``-1`` / ``0.0``.

``knn_cols`` builds the transpose (``csc_transpose``: a stable sort on the tensors' device) and
the norms (``col_rnorm``), then runs one workgroup per query with the dots of a tile of ``tile``
candidate columns in LDS.  The result does not depend on ``tile``.  Everything is fp64.  ``cuda``
tensors run the gfx950 kernels on the current stream, CPU tensors the OpenMP twin.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _native
from . import _args
from .slim import KMAX, check_csc

_P = C.c_void_p
_I64 = _native.c_i64
_native.register_hip("hm_knn_rnorm", [_P, _P, C.c_int, _P, _P])
_native.register_hip("hm_knn_cols", [_P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _I64, C.c_int,
                                     C.c_int, _P, _P, _P])
_native.register_host("hm_knn_rnorm_cpu", [_P, _P, C.c_int, _P])
_native.register_host("hm_knn_cols_cpu", [_P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _I64, C.c_int,
                                          C.c_int, _P, _P])

TILE_MAX = 16384    # candidate columns per pass: 128 KiB of fp64 accumulators in one CU's LDS


def _check_rows(rows: torch.Tensor, n_rows) -> int:
    """``n_rows`` validated against the row ids (default: the largest id + 1)."""
    nnz = rows.numel()
    lo, hi = (int(rows.min()), int(rows.max())) if nnz else (0, -1)
    if n_rows is None:
        n_rows = hi + 1
    n_rows = int(n_rows)
    if n_rows < 0 or n_rows > 2**31 - 1:
        raise ValueError(f"knn: n_rows must be in 0..2^31 - 1, got {n_rows}")
    if nnz and (lo < 0 or hi >= n_rows):
        raise ValueError(f"knn: rows must hold ids in 0..{n_rows - 1} (n_rows = {n_rows}), "
                         f"found {lo}..{hi}")
    return n_rows


def csc_transpose(colptr: torch.Tensor, rows: torch.Tensor, vals: torch.Tensor, n_rows: int):
    """(rowptr int64 [n_rows + 1], cols int32 ascending inside a row, rvals fp64): the same
    matrix by rows, from a stable sort of the row ids on the tensors' device."""
    n_cols = colptr.numel() - 1
    col_of = torch.repeat_interleave(torch.arange(n_cols, dtype=torch.int32, device=rows.device),
                                     colptr[1:] - colptr[:-1])
    perm = torch.sort(rows, stable=True).indices
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=rows.device)
    if rows.numel():
        torch.cumsum(torch.bincount(rows.long(), minlength=n_rows), 0, out=rowptr[1:])
    return rowptr, col_of[perm].contiguous(), vals[perm].contiguous()


def col_rnorm(colptr: torch.Tensor, vals: torch.Tensor) -> torch.Tensor:
    """fp64 [C]: ``1 / sqrt(sum v^2)`` of every column, 0 for an empty one.  The summation order
    is fixed, so identical columns get bit-identical norms."""
    _args.want("knn", colptr, "colptr", torch.int64, 1)
    _args.want("knn", vals, "vals", torch.float64, 1)
    _args.same_device("knn", (colptr, vals), ("colptr", "vals"))
    n_cols = colptr.numel() - 1
    out = torch.empty(max(n_cols, 0), dtype=torch.float64, device=vals.device)
    if n_cols <= 0:
        return out
    colptr, vals = colptr.contiguous(), vals.contiguous()
    args = (_native.ptr(colptr), _native.ptr(vals), n_cols, _native.ptr(out))
    if vals.is_cuda:
        _native.call_hip("hm_knn_rnorm", vals.device, *args)
    else:
        _native.call_host("hm_knn_rnorm", *args)
    return out


def query_work(colptr: torch.Tensor, rows: torch.Tensor, rowptr: torch.Tensor,
               query: torch.Tensor) -> torch.Tensor:
    """int64 [n]: the products a query accumulates, ``sum over rows u of column i of len(row u)``."""
    row_len = rowptr[1:] - rowptr[:-1]
    cs = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=rows.device)
    torch.cumsum(row_len[rows.long()], 0, out=cs[1:])
    q = query.long()
    return cs[colptr[q + 1]] - cs[colptr[q]]


def knn_cols(colptr: torch.Tensor, rows: torch.Tensor, vals: torch.Tensor, k: int,
             query: torch.Tensor | None = None, *, n_rows: int | None = None,
             tile: int | None = None, check: bool = True):
    """(idx int32 [n, k], score fp64 [n, k]): the ``k`` nearest columns of every ``query`` column
    (int32 [n]; default: every column) by cosine, ``-1`` / ``0.0`` where a query has fewer than
    ``k`` candidates.  Rows come back in the order of ``query``.

    ``tile`` (1..``TILE_MAX``, default ``TILE_MAX``) is the number of candidate columns a pass
    holds; it changes the number of passes, never the result.  ``check=False`` skips the
    validation of the CSC triple and of the row ids for a caller that has done it."""
    if check:
        n_cols = check_csc(colptr, rows, vals)
        n_rows = _check_rows(rows, n_rows)
    else:
        n_cols = colptr.numel() - 1
        n_rows = (int(rows.max()) + 1 if rows.numel() else 0) if n_rows is None else int(n_rows)
    k = _args.int_in("knn", k, "k", 1, KMAX)
    tile = TILE_MAX if tile is None else _args.int_in("knn", tile, "tile", 1, TILE_MAX)
    dev = colptr.device
    if query is None:
        query = torch.arange(n_cols, dtype=torch.int32, device=dev)
    _args.want("knn", query, "query", torch.int32, 1)
    _args.same_device("knn", (colptr, query), ("colptr", "query"))
    n = query.numel()
    if n and (int(query.min()) < 0 or int(query.max()) >= n_cols):
        raise ValueError(f"knn: query column ids must be in 0..{n_cols - 1}")
    if n == 0:
        return (torch.empty((0, k), dtype=torch.int32, device=dev),
                torch.empty((0, k), dtype=torch.float64, device=dev))
    colptr, rows, vals, query = (t.contiguous() for t in (colptr, rows, vals, query))
    return knn_cols_prepared(colptr, rows, vals, csc_transpose(colptr, rows, vals, n_rows),
                             col_rnorm(colptr, vals), query, k, tile)


def knn_cols_prepared(colptr, rows, vals, transposed, rnorm, query, k: int, tile: int = TILE_MAX):
    """The search itself, for validated contiguous arguments: ``transposed`` from
    ``csc_transpose``, ``rnorm`` from ``col_rnorm``."""
    rowptr, cols, rvals = transposed
    dev = colptr.device
    n_cols, n = colptr.numel() - 1, query.numel()
    idx = torch.empty((n, k), dtype=torch.int32, device=dev)
    score = torch.empty((n, k), dtype=torch.float64, device=dev)
    p = _native.ptr
    if colptr.is_cuda:
        # heaviest queries first, so that the long workgroups start early
        work = query_work(colptr, rows, rowptr, query)
        order = torch.sort(work, descending=True, stable=True).indices.to(torch.int32)
        _native.call_hip("hm_knn_cols", dev, p(colptr), p(rows), p(vals), n_cols, p(rowptr), p(cols), p(rvals),
                         p(rnorm), p(query), p(order), n, k, tile, p(idx), p(score))
    else:
        _native.call_host("hm_knn_cols", p(colptr), p(rows), p(vals), n_cols, p(rowptr), p(cols), p(rvals),
                          p(rnorm), p(query), n, k, tile, p(idx), p(score))
    return idx, score
