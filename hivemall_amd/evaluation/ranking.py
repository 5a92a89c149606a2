"""Whole-column ranking measures on the native engine (``ops/rank_eval.py``).

* ``ranking_measures_batch``: the seven per-row measures of ``[U, L]`` rank lists against a CSR
  truth, for callers that hold tensors (a trainer validating after every epoch).
* ``grouped_form``: the column-at-once form of one rank UDAF for the SQL executor
  (``registry``): per-row values from the engine, then the loop's own mean per group.  It is taken
  only where the result provably equals the loop's and declines (None) anything else.
"""
from __future__ import annotations

import itertools
import os

import numpy as np
import torch

RANK_EVAL_CALLS = {"native": 0, "python": 0}       # how the calls were served (tests assert the route)

# ndcg_one adds its terms with sum(): left to right up to Python 3.11, compensated from 3.12.  The
# engine adds left to right, so ndcg is native only where sum() does too.
SUM_IS_SEQUENTIAL = sum([0.1] * 10) == 0.9999999999999999


def _as_tensor(x, dtype, device, name):
    if isinstance(x, torch.Tensor):
        t = x
    else:
        x = np.asarray(x)
        t = torch.from_numpy(np.ascontiguousarray(x) if x.flags.writeable else x.copy())
    if t.dtype != dtype:
        if t.dtype.is_floating_point or t.dtype == torch.bool or dtype.is_floating_point:
            raise ValueError(f"rank_eval: {name} must be {dtype}, got {t.dtype}")
        t = t.to(dtype)
    return t.to(device)


def ranking_measures_batch(rank, truth, k=None, device=None) -> dict:
    """The seven ranking measures of every row and their means.

    ``rank`` is an int64 ``[U, L]`` tensor or array (``recommend_topk``'s item tensor goes in as it
    is, without a host copy), or a numpy CSR pair ``(rowptr, items)`` of ragged lists.  ``truth``
    is an ``ops.rank_eval.TruthIndex`` (built once, reused every epoch) or a CSR pair
    ``(rowptr, items)`` / triple ``(rowptr, items, rel)`` of tensors or arrays; items need not be
    sorted or distinct.  ``device`` defaults to ``rank``'s when it is a tensor, else to the GPU
    when there is one.

    Returns ``{name: fp64 [U] tensor}`` for ``ops.rank_eval.NAMES`` plus ``"mean"``, a dict of
    0-dim tensors.  The per-row values equal ``metrics.*_one`` bit for bit; the means are
    ``torch.mean`` and equal ``np.mean`` to within rounding."""
    from ..models.base import resolve_device
    from ..ops import rank_eval as re

    if device is None and isinstance(rank, torch.Tensor):
        dev = rank.device
    else:
        dev = resolve_device(device)
    lengths = None
    if isinstance(rank, tuple) and len(rank) == 2:
        rank, lengths = _pad_csr(np.asarray(rank[0]), np.asarray(rank[1]))
        lengths = torch.from_numpy(lengths).to(dev)
    rank = _as_tensor(rank, torch.int64, dev, "rank")
    if not isinstance(truth, re.TruthIndex):
        if not isinstance(truth, (tuple, list)) or len(truth) not in (2, 3):
            raise ValueError("rank_eval: truth must be a TruthIndex or (rowptr, items[, rel])")
        parts = [_as_tensor(t, torch.int64, dev, n) for t, n in zip(truth, ("rowptr", "items", "rel"))]
        truth = re.build_truth(*parts)
    vals = re.rank_measures(rank, truth, k, lengths=lengths)
    out = {name: vals[m] for m, name in enumerate(re.NAMES)}
    out["mean"] = {name: (vals[m].mean() if vals.shape[1] else vals.new_tensor(float("nan")))
                   for m, name in enumerate(re.NAMES)}
    return out


def _pad_csr(rowptr: np.ndarray, items: np.ndarray):
    """``(rank int64 [U, max(L, 1)], lengths int32 [U])`` of ragged lists."""
    from ..ops import rank_eval as re

    if rowptr.ndim != 1 or len(rowptr) < 1 or rowptr.dtype.kind not in "iu" or items.dtype.kind not in "iu":
        raise ValueError("rank_eval: a CSR rank is (rowptr, items) of integers")
    lens = np.diff(rowptr.astype(np.int64))
    if int(rowptr[0]) != 0 or int(rowptr[-1]) != len(items) or (lens < 0).any():
        raise ValueError(f"rank_eval: rowptr must rise from 0 to len(items) = {len(items)}")
    L = max(int(lens.max()) if len(lens) else 0, 1)
    if L > re.L_MAX:
        raise ValueError(f"rank_eval: rank lists must hold at most {re.L_MAX} positions, got {L}")
    mat = np.zeros((len(lens), L), dtype=np.int64)
    mat[np.arange(L) < lens[:, None]] = items
    return mat, lens.astype(np.int32)


# ------------------------------------------------------------------ the SQL route
_NP_INTS = (np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32)


def _plain_ints(row) -> bool:
    """Whether every element is a plain ``int`` or a NumPy integer inside int64: in a set
    ``1.0 == 1 == True``, so anything else could hit where an int64 compare would not."""
    if isinstance(row, np.ndarray):
        return row.ndim == 1 and row.dtype.type in _NP_INTS
    return all(t is int or t in _NP_INTS for t in set(map(type, row)))


def _flatten(rows):
    """``(flat int64, lens int64)`` of a column of integer lists, or None when one is not a list,
    tuple or 1-d array of plain ints inside int64."""
    for r in rows:
        if not isinstance(r, (list, tuple, np.ndarray)) or not _plain_ints(r):
            return None
    lens = np.fromiter(map(len, rows), dtype=np.int64, count=len(rows))
    try:
        flat = np.fromiter(itertools.chain.from_iterable(rows), dtype=np.int64, count=int(lens.sum()))
    except (OverflowError, TypeError, ValueError):
        return None
    return flat, lens


def _is_graded(t) -> bool:
    """ndcg_one's own test for a graded truth."""
    if isinstance(t, dict):
        return True
    if isinstance(t, (list, tuple)) and len(t):
        first = next((v for v in t if v is not None), None)
        return isinstance(first, (tuple, list))
    return False


def _graded(truth):
    """``(items, lens, grades int64)`` of a truth column with dict or ``(item, rel)`` rows (plain
    rows count as grade 1, which is what ndcg_one gives them), or None."""
    from ..ops import rank_eval as re

    keys, grades = [], []
    for t in truth:
        if isinstance(t, dict):
            ks, vs = list(t.keys()), list(t.values())
        elif _is_graded(t):
            if not all(isinstance(p, (tuple, list)) and len(p) == 2 for p in t):
                return None
            ks, vs = [p[0] for p in t], [p[1] for p in t]
        elif isinstance(t, (list, tuple, np.ndarray)) and _plain_ints(t):
            # ndcg_one: rel = {t: 1.0 for t in _as_set(truth)}
            ks, vs = list(t), [1] * len(t)
        else:
            return None
        for v in vs:
            if type(v) not in (int, float) or not 0 <= v <= re.REL_MAX or v != int(v):
                return None
        keys.append(ks)
        grades.append([int(v) for v in vs])
    flat = _flatten(keys)
    if flat is None:
        return None
    rel = np.fromiter(itertools.chain.from_iterable(grades), dtype=np.int64, count=len(flat[0]))
    return flat[0], flat[1], rel


def _constant_k(kcol):
    """``(True, k)`` when the column is one plain int in the engine's range (None: no column),
    else ``(False, None)``."""
    from ..ops import rank_eval as re

    if kcol is None:
        return True, None
    vals = kcol.tolist() if hasattr(kcol, "tolist") else list(kcol)
    if not vals:
        return True, None
    k = vals[0]
    if type(k) is not int and type(k) not in _NP_INTS:
        return False, None
    if any(type(v) is not type(k) or v != k for v in vals):
        return False, None
    k = int(k)
    return (True, k) if 0 <= k <= re.K_MAX else (False, None)


def _per_row_values(measure: int, rank_rows, truth_rows, k, device):
    """fp64 numpy ``[U]`` of one measure from the engine, or None where the input is not proven."""
    from ..models.base import resolve_device
    from ..ops import rank_eval as re

    if measure == re.NDCG and not SUM_IS_SEQUENTIAL:
        return None
    rk = _flatten(rank_rows)
    if rk is None:
        return None
    flat, lens = rk
    L = max(int(lens.max()), 1)
    if L > re.L_MAX:
        return None
    rel = None
    if measure == re.NDCG and any(_is_graded(t) for t in truth_rows):
        tr = _graded(truth_rows)
        if tr is None:
            return None
        titems, tlens, rel = tr
    else:
        tr = _flatten(truth_rows)
        if tr is None:
            return None
        titems, tlens = tr
    dev = resolve_device(device)
    try:
        from .. import _native

        _native.hip() if dev.type == "cuda" else _native.host()
    except (RuntimeError, OSError):
        return None                                 # no native library: the loop serves
    U = len(lens)
    mat = np.zeros((U, L), dtype=np.int64)
    mat[np.arange(L) < lens[:, None]] = flat
    rowptr = np.zeros(U + 1, dtype=np.int64)
    np.cumsum(tlens, out=rowptr[1:])
    to = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    truth = re.build_truth(to(rowptr), to(titems), None if rel is None else to(rel))
    vals = re.rank_measures(to(mat), truth, k, lengths=to(lens.astype(np.int32)), measures=1 << measure)
    return np.ascontiguousarray(vals[measure].cpu().numpy())


def grouped_form(measure: int, array_form_only: bool = False):
    """The ``grouped`` form (``registry``) of the rank UDAF that reports ``measure``: one value per
    group, ``float(np.mean(...))`` of the group's per-row values in row order, which is
    ``metrics._mean``'s own arithmetic; ``nan`` for a group without rows.  None declines."""
    def grouped(arg_series, codes, n_groups, session=None):
        if len(arg_series) not in (2, 3) or os.environ.get("HM_SQL_BATCH_UDTF", "1") == "0":
            return None
        rank_rows, truth_rows = arg_series[0].tolist(), arg_series[1].tolist()
        if array_form_only and not rank_rows:
            return None                             # auc cannot tell its two forms without a row
        ok, k = _constant_k(arg_series[2] if len(arg_series) == 3 else None)
        if not ok:
            return None
        codes = np.asarray(codes)
        if rank_rows:
            vals = _per_row_values(measure, rank_rows, truth_rows, k, None if session is None else session.device)
            if vals is None:
                return None
        else:
            vals = np.zeros(0, dtype=np.float64)
        RANK_EVAL_CALLS["native"] += 1
        order = np.argsort(codes, kind="stable")
        bounds = np.searchsorted(codes[order], np.arange(n_groups + 1))
        return [float(np.mean(vals[order[bounds[g]:bounds[g + 1]]])) if bounds[g + 1] > bounds[g] else float("nan")
                for g in range(n_groups)]
    return grouped
