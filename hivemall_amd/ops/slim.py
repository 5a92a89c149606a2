"""SLIM's two native steps (``csrc/kernels/slim.hip``, ``csrc/host/slim_cpu.cpp``).

``slim_gram(colptr, rows, vals, target, nbr)`` builds, for every item, the Gram matrix of its
neighbours' rating vectors and their products with the item's own vector, straight from a CSC
ratings matrix (columns = rating vectors): ``G[t, a, c] = <col nbr[t, a], col nbr[t, c]>``,
``b[t, a] = <col nbr[t, a], col target[t]>``.  No dense ``users x K`` matrix is formed.

``slim_cd(G, b, l1, l2, iters, eps)`` runs the non-negative elastic-net coordinate descent of
``models.recommend._slim_cd_chunk`` on them: coordinates in index order,
``w_k = max(0, b_k - sum_{m != k} G_km w_m - l1) / (G_kk + l2)``, coordinates with
``G_kk <= 0`` skipped, an item stops after the sweep whose largest change is below ``eps``.

Everything is fp64.  ``cuda`` tensors run the gfx950 kernels (one workgroup per item for the
Gram build; one wave per item with its Gram matrix in LDS for the descent, hence at most
``KMAX`` neighbours), CPU tensors the OpenMP twins with the same contracts.

``slim_topk(rowptr, cols, vals, mptr, mnn, mw, k)`` serves the model: for every user (a row of a
CSR ratings matrix) the ``k`` best items under ``score(u, i) = sum of mw * r[u, nn]`` over the
neighbours ``nn`` of model row ``i`` that the user has rated, added in ascending ``nn`` order,
every product rounded before its add, so that kernel (``csrc/kernels/slim_topk.hip``), twin and a
Python loop give the same bits (``docs/compat.md``, SLIM recommendation).  Limits: ``k <= KTOP``,
fewer than 2^31 users and items.  Inside them nothing is declined (``supports``): more items than
one LDS bitmap window (``BITMAP_ITEMS``) are served window by window, a user with more than
``STAGED_RATINGS`` ratings is looked up in global memory instead of LDS.

Reference: core/src/main/java/hivemall/recommend/SlimUDTF.java.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _native
from . import _args

_P = C.c_void_p
_I64 = _native.c_i64
_F64 = C.c_double
_native.register_hip("hm_slim_gram", [_P, _P, _P, C.c_int, _P, _P, _I64, C.c_int, _P, _P, _P])
_native.register_hip("hm_slim_cd", [_P, _P, _I64, C.c_int, _F64, _F64, C.c_int, _F64, _P, _P])
_native.register_host("hm_slim_gram_cpu", [_P, _P, _P, C.c_int, _P, _P, _I64, C.c_int, _P, _P])
_native.register_host("hm_slim_cd_cpu", [_P, _P, _I64, C.c_int, _F64, _F64, C.c_int, _F64, _P])

_native.register_hip("hm_slim_topk", [_P, _P, _P, _I64, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P])
_native.register_host("hm_slim_topk_cpu", [_P, _P, _P, _I64, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P])

KMAX = 128          # neighbours per item of slim_cd (an fp64 K x K Gram matrix in one CU's LDS)
KTOP = 256          # slim_topk's largest k (the best-k list of a workgroup in LDS)
BITMAP_ITEMS = 16384 * 32   # items per candidate-bitmap window of slim_topk (64 KiB of LDS)
STAGED_RATINGS = 1024       # a user's ratings held in LDS by slim_topk; longer rows stay in memory


def check_csc(colptr: torch.Tensor, rows: torch.Tensor, vals: torch.Tensor) -> int:
    """Validate a CSC triple (dtypes, shapes, offsets, row ids strictly increasing inside every
    column); returns the number of columns."""
    _args.want("slim", colptr, "colptr", torch.int64, 1)
    _args.want("slim", rows, "rows", torch.int32, 1)
    _args.want("slim", vals, "vals", torch.float64, 1)
    _args.same_device("slim", (colptr, rows, vals), ("colptr", "rows", "vals"))
    nnz = rows.numel()
    if colptr.numel() < 1 or vals.numel() != nnz:
        raise ValueError("slim: colptr must have C + 1 entries and rows / vals the same length")
    if int(colptr[0]) != 0 or int(colptr[-1]) != nnz or bool((colptr[1:] < colptr[:-1]).any()):
        raise ValueError("slim: colptr must rise from 0 to len(rows)")
    if nnz > 1:
        bad = rows[1:] <= rows[:-1]
        starts = colptr[1:-1]
        starts = starts[(starts > 0) & (starts < nnz)]
        bad[starts - 1] = False                       # a new column may start anywhere
        if bool(bad.any()):
            raise ValueError("slim: rows must be strictly increasing inside every column")
    return colptr.numel() - 1


def slim_gram(colptr: torch.Tensor, rows: torch.Tensor, vals: torch.Tensor,
              target: torch.Tensor, nbr: torch.Tensor, *, check: bool = True):
    """(G fp64 [n, K, K], b fp64 [n, K]) for ``target`` int32 [n] and ``nbr`` int32 [n, K]
    (column ids, ``-1`` = padding: its rows and columns of G and entries of b are zero).

    ``check=False`` skips the validation of the CSC triple (``check_csc``) for a caller that
    has validated it once and launches many chunks."""
    _args.want("slim", target, "target", torch.int32, 1)
    _args.want("slim", nbr, "nbr", torch.int32, 2)
    if check:
        n_cols = check_csc(colptr, rows, vals)
    else:
        n_cols = colptr.numel() - 1
    _args.same_device("slim", (colptr, target, nbr), ("colptr", "target", "nbr"))
    n, K = nbr.shape
    if target.numel() != n:
        raise ValueError(f"slim: target has {target.numel()} entries, nbr {n} rows")
    if n and (int(target.min()) < 0 or int(target.max()) >= n_cols):
        raise ValueError(f"slim: target column ids must be in 0..{n_cols - 1}")
    if n and K and (int(nbr.min()) < -1 or int(nbr.max()) >= n_cols):
        raise ValueError(f"slim: nbr column ids must be -1 or in 0..{n_cols - 1}")
    dev = colptr.device
    G = torch.empty((n, K, K), dtype=torch.float64, device=dev)
    b = torch.empty((n, K), dtype=torch.float64, device=dev)
    if n == 0 or K == 0:
        return G, b
    colptr, rows, vals, target, nbr = (t.contiguous() for t in (colptr, rows, vals, target, nbr))
    p = _native.ptr
    args = (p(colptr), p(rows), p(vals), n_cols, p(target), p(nbr), n, K, p(G), p(b))
    if colptr.is_cuda:
        _native.call_hip("hm_slim_gram", dev, *args)
    else:
        _native.call_host("hm_slim_gram", *args)
    return G, b


def slim_cd(G: torch.Tensor, b: torch.Tensor, l1: float, l2: float, iters: int,
            eps: float) -> torch.Tensor:
    """W fp64 [n, K] from G fp64 [n, K, K] and b fp64 [n, K]; K <= ``KMAX``."""
    _args.want("slim", G, "G", torch.float64, 3)
    _args.want("slim", b, "b", torch.float64, 2)
    _args.same_device("slim", (G, b), ("G", "b"))
    n, K = b.shape
    if tuple(G.shape) != (n, K, K):
        raise ValueError(f"slim: G must be [n, K, K] for b [n, K], got {tuple(G.shape)} and {tuple(b.shape)}")
    if K > KMAX:
        raise ValueError(f"slim_cd: {K} neighbours per item, the native descent holds at most {KMAX}")
    if iters < 0:
        raise ValueError("slim_cd: iters must be >= 0")
    W = torch.zeros((n, K), dtype=torch.float64, device=G.device)
    if n == 0 or K == 0 or iters == 0:
        return W
    G, b = G.contiguous(), b.contiguous()
    p = _native.ptr
    args = (p(G), p(b), n, K, float(l1), float(l2), int(iters), float(eps), p(W))
    if G.is_cuda:
        _native.call_hip("hm_slim_cd", G.device, *args)
    else:
        _native.call_host("hm_slim_cd", *args)
    return W


def check_csr(ptr: torch.Tensor, idx: torch.Tensor, vals: torch.Tensor,
              names=("rowptr", "cols", "vals")) -> int:
    """``check_csc`` for a row-major triple under the given argument names (the ratings of
    ``slim_topk``, its model): dtypes, offsets, indices >= 0 and strictly increasing inside every
    row, finite values; returns the number of rows."""
    _args.want("slim", ptr, names[0], torch.int64, 1)
    _args.want("slim", idx, names[1], torch.int32, 1)
    _args.want("slim", vals, names[2], torch.float64, 1)
    _args.same_device("slim", (ptr, idx, vals), names)
    nnz = idx.numel()
    if ptr.numel() < 1 or vals.numel() != nnz:
        raise ValueError(f"slim: {names[0]} must have n + 1 entries and {names[1]} / {names[2]} the same length")
    if int(ptr[0]) != 0 or int(ptr[-1]) != nnz or bool((ptr[1:] < ptr[:-1]).any()):
        raise ValueError(f"slim: {names[0]} must rise from 0 to len({names[1]})")
    if nnz and int(idx.min()) < 0:
        raise ValueError(f"slim: {names[1]} must be >= 0")
    if nnz > 1:
        bad = idx[1:] <= idx[:-1]
        starts = ptr[1:-1]
        starts = starts[(starts > 0) & (starts < nnz)]
        bad[starts - 1] = False                       # a new row may start anywhere
        if bool(bad.any()):
            raise ValueError(f"slim: {names[1]} must be strictly increasing inside every row")
    if not bool(torch.isfinite(vals).all()):
        raise ValueError(f"slim: {names[2]} must be finite")
    return ptr.numel() - 1


def supports(n_users: int, n_items: int, k: int) -> bool:
    """Whether ``slim_topk`` serves this shape.  Row lengths and item counts never decline: a
    long row is searched in memory, many items are walked one bitmap window at a time."""
    return 1 <= k <= KTOP and 0 <= n_users < 2**31 and 0 <= n_items < 2**31


def transpose_model(mptr: torch.Tensor, mnn: torch.Tensor):
    """(tptr int64 [I + 1], ti int32): for every neighbour ``nn`` the target items whose model
    row holds it, ascending.  One stable sort."""
    n_items = mptr.numel() - 1
    tgt = torch.repeat_interleave(torch.arange(n_items, dtype=torch.int32, device=mptr.device),
                                  mptr[1:] - mptr[:-1])
    order = torch.sort(mnn, stable=True)[1]
    tptr = torch.zeros(n_items + 1, dtype=torch.int64, device=mptr.device)
    tptr[1:] = torch.cumsum(torch.bincount(mnn, minlength=n_items), 0)
    return tptr, tgt[order].contiguous()


def check_topk(rowptr, cols, vals, mptr, mnn, mw, k) -> tuple[int, int, int]:
    """The argument contract of ``slim_topk``, for every engine that serves it (the kernel, the
    twin, the torch path of ``SLIM.recommend_topk``): ``(n_users, n_items, k)`` or ``ValueError``."""
    k = _args.int_in("slim_topk", k, "k", 1, KTOP)
    n_users = check_csr(rowptr, cols, vals)
    n_items = check_csr(mptr, mnn, mw, ("mptr", "mnn", "mw"))
    _args.same_device("slim", (rowptr, mptr), ("rowptr", "mptr"))
    for name, t in (("cols", cols), ("mnn", mnn)):
        if t.numel() and int(t.max()) >= n_items:
            raise ValueError(f"slim: {name} must be item indices in 0..{n_items - 1}")
    if mnn.numel():
        own = torch.repeat_interleave(torch.arange(n_items, dtype=torch.int32, device=mnn.device),
                                      mptr[1:] - mptr[:-1])
        if bool((own == mnn).any()):
            raise ValueError("slim: an item must not be its own neighbour (mnn != i)")
    return n_users, n_items, k


def slim_topk(rowptr: torch.Tensor, cols: torch.Tensor, vals: torch.Tensor, mptr: torch.Tensor,
              mnn: torch.Tensor, mw: torch.Tensor, k: int, exclude_seen: bool = True,
              check: bool = True):
    """(items int32 [U, k], scores fp64 [U, k]), best first, padded with ``-1`` / ``-inf``.

    ``(rowptr, cols, vals)`` is the user-major CSR of the ratings, ``(mptr, mnn, mw)`` the model
    as a CSR over the ``I`` target items (row ``i``: its neighbours and weights); both with
    strictly ascending indices inside a row, item indices in ``0..I-1``, ``mnn != i``, finite
    values.  Item ``i`` is a candidate of user ``u`` when ``u`` rated one of row ``i``'s
    neighbours (and, with ``exclude_seen``, not ``i`` itself); the order is score descending,
    then item ascending.  ``check=False`` skips the validation of the two triples."""
    if check:
        n_users, n_items, k = check_topk(rowptr, cols, vals, mptr, mnn, mw, k)
    else:
        k = _args.int_in("slim_topk", k, "k", 1, KTOP)
        n_users, n_items = rowptr.numel() - 1, mptr.numel() - 1
    if not supports(n_users, n_items, k):
        raise ValueError(f"slim_topk: {n_users} users x {n_items} items is outside the engine (< 2^31 each)")
    dev = rowptr.device
    items = torch.empty((n_users, k), dtype=torch.int32, device=dev)
    scores = torch.empty((n_users, k), dtype=torch.float64, device=dev)
    if n_users == 0:
        return items, scores
    rowptr, cols, vals, mptr, mnn, mw = (t.contiguous() for t in (rowptr, cols, vals, mptr, mnn, mw))
    tptr, ti = transpose_model(mptr, mnn)
    p = _native.ptr
    args = (p(rowptr), p(cols), p(vals), n_users, p(mptr), p(mnn), p(mw), p(tptr), p(ti), n_items,
            k, int(bool(exclude_seen)), p(items), p(scores))
    if rowptr.is_cuda:
        _native.call_hip("hm_slim_topk", dev, *args)
    else:
        _native.call_host("hm_slim_topk", *args)
    return items, scores
