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

KMAX = 128          # neighbours per item of slim_cd (an fp64 K x K Gram matrix in one CU's LDS)


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
