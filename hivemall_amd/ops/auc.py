"""Grouped ROC AUC in integers (``csrc/kernels/auc.hip``, ``csrc/host/auc_cpu.cpp``): the engine
behind ``evaluation.auc_batch`` and the ``(score, label)`` form of SQL's ``auc``.

Contract (``docs/compat.md`` "AUC engine"; ``evaluation.metrics.auc`` is the definition).

* ``auc_groups(scores, labels, rowptr, order=None)`` returns ``(two_u, n_pos, n_neg)``, int64
  ``[G]`` each.  Group ``g`` is the rows ``order[rowptr[g]:rowptr[g + 1]]``, contiguous rows
  without ``order``.  ``two_u[g]`` is the sum over the group's positive rows ``p`` and negative
  rows ``n`` of ``2 * [p > n] + [p == n]``; a group where nothing counts gets zeros.
* A row with a NaN score or a NaN label is absent, and so is an ``order`` entry outside the rows.
  A label ``> 0`` is positive.  Scores compare as fp64 values (fp32 is widened, which is exact):
  ``-0.0 == 0.0`` and ``+-inf`` are ordinary values.
* ``auc_values`` turns the counts into ``(two_u / 2) / (n_pos * n_neg)`` in fp64: ``nan`` for a
  group without a positive or without a negative.  While a group holds fewer than ``2^26`` rows
  this is ``metrics.auc`` of the group bit for bit, since every intermediate of its rank-sum
  formula is then a half-integer below ``2^52``; a larger group raises ``ValueError``, and so do
  ``2^31`` rows or more.

``cuda`` tensors run the gfx950 kernels on the current stream, CPU tensors the OpenMP twin.  The
kernels come in three classes of group size, binned on the host from ``rowptr`` (read once): up to
``SMALL_MAX`` rows in a sub-wave, up to ``MEDIUM_MAX`` in a workgroup, and longer groups through
``torch.sort`` and three kernels over tiles of ``TILE`` sorted rows.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _native
from . import _args

_P = C.c_void_p
_I64 = _native.c_i64
_native.register_hip("hm_auc_prepare", [_P, C.c_int, _P, C.c_int, _I64, _P, _I64, _P, _P, _P])
_native.register_hip("hm_auc_small", [_P, _P, _P, _P, _I64, C.c_int, _P, _P, _P, _P])
_native.register_hip("hm_auc_medium", [_P, _P, _P, _P, _I64, _P, _P, _P, _P])
_native.register_hip("hm_auc_long_count", [_P, _I64, _P, _P])
_native.register_hip("hm_auc_long_scan", [_P, _I64, _P, _P, _P])
_native.register_hip("hm_auc_long_sum", [_P] * 6 + [_I64, _P, _P, _P, _P])
_native.register_host("hm_auc_groups_cpu", [_P, C.c_int, _P, C.c_int, _I64, _P, _I64, _P, _I64, _P, _P, _P])

SMALL_MAX = 64              # one sub-wave of 8, 16, 32 or 64 lanes
MEDIUM_MAX = 2048           # AUC_MEDIUM_MAX: one workgroup, 16 KB of LDS keys
TILE = 2048                 # AUC_TILE
GROUP_ROWS_MAX = 2**26 - 1  # where the exactness argument ends
ROWS_MAX = 2**31 - 1

# what the calls did (the tests assert the path taken, not its timing)
STATS = {"calls": 0, "hip": 0, "host": 0}

_OP = "auc"
_KIND = {torch.float64: 0, torch.float32: 1, torch.int64: 2, torch.int32: 3}    # AUC_F64 .. AUC_I32
_NARROW = (torch.int8, torch.int16, torch.uint8, torch.bool)
_LANES = (8, 16, 32, SMALL_MAX)


def _column(t, name: str, kinds) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{_OP}: {name} must be a torch tensor, got {type(t).__name__}")
    if t.dim() != 1:
        raise ValueError(f"{_OP}: {name} must have 1 dimension(s), got shape {tuple(t.shape)}")
    if t.dtype in _NARROW and torch.int32 in kinds:
        t = t.to(torch.int32)
    if t.dtype not in kinds:
        raise ValueError(f"{_OP}: {name} must be one of {', '.join(map(str, kinds))}, got {t.dtype}")
    return t


def auc_groups(scores: torch.Tensor, labels: torch.Tensor, rowptr: torch.Tensor,
               order: torch.Tensor | None = None):
    """``(two_u, n_pos, n_neg)`` int64 ``[G]`` of the groups ``order[rowptr[g]:rowptr[g + 1]]``
    (module docstring).  ``scores`` fp64 or fp32 ``[n]``, ``labels`` fp64, fp32 or an integer type
    ``[n]``, ``rowptr`` int64 ``[G + 1]`` rising from 0 to the number of grouped rows, ``order``
    int64 row numbers."""
    scores = _column(scores, "scores", (torch.float64, torch.float32))
    labels = _column(labels, "labels", tuple(_KIND))
    _args.want(_OP, rowptr, "rowptr", torch.int64, 1)
    names, ts = ["scores", "labels", "rowptr"], [scores, labels, rowptr]
    if order is not None:
        _args.want(_OP, order, "order", torch.int64, 1)
        order = order.contiguous()
        names.append("order")
        ts.append(order)
    _args.same_device(_OP, ts, names)
    n = scores.numel()
    if labels.numel() != n:
        raise ValueError(f"{_OP}: labels must hold {n} rows, got {labels.numel()}")
    N = n if order is None else order.numel()
    if max(n, N) > ROWS_MAX:
        raise ValueError(f"{_OP}: at most {ROWS_MAX} rows, got {max(n, N)}")
    if rowptr.numel() < 1:
        raise ValueError(f"{_OP}: rowptr must hold at least one entry")
    rp = rowptr.cpu().numpy()                      # the one host read: the size binning needs it
    sizes = np.diff(rp)
    if int(rp[0]) != 0 or int(rp[-1]) != N or (sizes < 0).any():
        raise ValueError(f"{_OP}: rowptr must rise from 0 to the {N} grouped rows")
    G = len(sizes)
    if G and int(sizes.max()) > GROUP_ROWS_MAX:
        raise ValueError(f"{_OP}: a group holds {int(sizes.max())} rows, the limit is {GROUP_ROWS_MAX}")
    dev = scores.device
    STATS["calls"] += 1
    out = torch.zeros((3, G), dtype=torch.int64, device=dev)
    if G == 0:
        return out[0], out[1], out[2]
    ptr = _native.ptr
    scores, labels, rowptr = scores.contiguous(), labels.contiguous(), rowptr.contiguous()
    columns = (ptr(scores), _KIND[scores.dtype], ptr(labels), _KIND[labels.dtype], n, ptr(order), N)
    if dev.type != "cuda":
        _native.call_host("hm_auc_groups", *columns, ptr(rowptr), G, ptr(out[0]), ptr(out[1]), ptr(out[2]))
        STATS["host"] += 1
        return out[0], out[1], out[2]

    outs = (ptr(out[0]), ptr(out[1]), ptr(out[2]))
    keys = torch.empty(N, dtype=torch.int64, device=dev)
    cls = torch.empty(N, dtype=torch.uint8, device=dev)
    _native.call_hip("hm_auc_prepare", dev, *columns, ptr(keys), ptr(cls))
    # size classes: four sub-wave widths, the workgroup, the sorted route
    klass = np.searchsorted(np.asarray(_LANES + (MEDIUM_MAX,)), sizes, side="left")
    by_class = np.argsort(klass, kind="stable")
    counts = np.bincount(klass, minlength=6)
    ids = torch.from_numpy(by_class).to(dev)
    at = 0
    for k, cnt in enumerate(counts.tolist()):
        part = ids[at:at + cnt]
        if cnt and k < 4:
            _native.call_hip("hm_auc_small", dev, ptr(keys), ptr(cls), ptr(rowptr), ptr(part), cnt, _LANES[k], *outs)
        elif cnt and k == 4:
            _native.call_hip("hm_auc_medium", dev, ptr(keys), ptr(cls), ptr(rowptr), ptr(part), cnt, *outs)
        elif cnt:
            _long_groups(keys, cls, rp[by_class[at:]], sizes[by_class[at:]], part, outs)
        at += cnt
    STATS["hip"] += 1
    return out[0], out[1], out[2]


def _long_groups(keys, cls, starts: np.ndarray, lens: np.ndarray, ids: torch.Tensor, outs) -> None:
    """The groups longer than ``MEDIUM_MAX``: their rows sorted by (group, key) with ``torch.sort``,
    then negatives per tile, the exclusive negative prefix and the two searches per positive."""
    dev, ptr = keys.device, _native.ptr
    GL = len(lens)
    seg = np.zeros(GL + 1, dtype=np.int64)
    np.cumsum(lens, out=seg[1:])
    NL = int(seg[-1])
    segptr = torch.from_numpy(seg).to(dev)
    gid = None
    if GL == 1:
        k, c = keys[int(starts[0]):int(starts[0]) + NL], cls[int(starts[0]):int(starts[0]) + NL]
        s = torch.sort(k)
        k, c = s.values, c[s.indices]
    else:
        gid = torch.repeat_interleave(torch.from_numpy(lens).to(dev), output_size=NL)
        src = torch.arange(NL, dtype=torch.int64, device=dev) + (torch.from_numpy(starts).to(dev) - segptr[:-1])[gid]
        k, c = keys[src], cls[src]
        # by key, then stably by group: an int64 key leaves no room for the group in one sort
        o1 = torch.sort(k).indices
        perm = o1[torch.sort(gid[o1], stable=True).indices]
        k, c, gid = k[perm], c[perm], gid.to(torch.int32)
    k, c = k.contiguous(), c.contiguous()
    tiles = torch.empty((NL + TILE - 1) // TILE, dtype=torch.int64, device=dev)
    _native.call_hip("hm_auc_long_count", dev, ptr(c), NL, ptr(tiles))
    inc = torch.cumsum(tiles, 0)
    negpre = torch.empty(NL + 1, dtype=torch.int32, device=dev)
    _native.call_hip("hm_auc_long_scan", dev, ptr(c), NL, ptr(inc), ptr(negpre))
    _native.call_hip("hm_auc_long_sum", dev, ptr(k), ptr(c), ptr(negpre), ptr(gid), ptr(segptr), ptr(ids), NL, *outs)


def auc_values(two_u: torch.Tensor, n_pos: torch.Tensor, n_neg: torch.Tensor) -> torch.Tensor:
    """fp64 ``(two_u / 2) / (n_pos * n_neg)``; ``0 / 0 = nan`` where a class is empty."""
    return (two_u.to(torch.float64) / 2) / (n_pos.to(torch.float64) * n_neg.to(torch.float64))
