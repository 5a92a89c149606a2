"""Binary-classification ROC AUC of whole columns on the native engine (``ops/auc.py``).

* ``auc_batch``: the AUC of every group of a prediction table, for callers that hold tensors (a
  trainer scoring a validation set after every epoch, per-user "GAUC").
* ``scalar_grouped``: the column-at-once form of ``auc(score, label)`` for the SQL executor
  (``registry``).  Its values equal ``metrics.auc`` of every group bit for bit; it declines (None)
  what it cannot serve, and the executor's loop then answers with its results and its exceptions.
"""
from __future__ import annotations

import os

import numpy as np
import torch

AUC_CALLS = {"native": 0, "python": 0}         # how auc(score, label) columns were served


def _as_column(x, device, floating: bool) -> torch.Tensor:
    """A score column (fp32 stays, anything else becomes fp64) or a label column (floats and
    integers stay as they are) on ``device``."""
    if not isinstance(x, torch.Tensor):
        x = np.asarray(x)
        if x.dtype.kind not in "fiub":
            raise ValueError(f"auc: a column must hold numbers, got dtype {x.dtype}")
        if x.dtype.kind == "u" or x.dtype == np.float16:
            x = x.astype(np.float64 if floating else np.int64)
        x = torch.from_numpy(np.ascontiguousarray(x) if x.flags.writeable else x.copy())
    if floating and x.dtype != torch.float32:
        x = x.to(torch.float64)
    elif x.dtype in (torch.float16, torch.bfloat16):
        x = x.to(torch.float32)
    return x.reshape(-1).to(device)


def auc_batch(scores, labels, groups=None, device=None) -> torch.Tensor:
    """fp64 ``[G]``: the ROC AUC (ties averaged) of every group, ``metrics.auc`` of the group's rows
    bit for bit; ``nan`` for a group without a positive, without a negative or without a row.

    ``scores`` and ``labels`` are tensors or arrays of ``n`` rows (a label ``> 0`` is positive, a
    row with a NaN score or label is left out).  ``groups`` holds the group code ``0..G-1`` of
    every row, in any row order, as an int tensor or array; ``None`` is one group.  Tensors that
    are on the device already go in without a host copy; ``device`` defaults to the device of
    ``scores`` when it is a tensor, else to the GPU when there is one."""
    from ..models.base import resolve_device
    from ..ops import auc as engine

    dev = scores.device if device is None and isinstance(scores, torch.Tensor) else resolve_device(device)
    s = _as_column(scores, dev, floating=True)
    y = _as_column(labels, dev, floating=False)
    n = s.numel()
    if groups is None:
        rowptr, order = torch.tensor([0, n], dtype=torch.int64, device=dev), None
    else:
        codes = groups if isinstance(groups, torch.Tensor) else torch.from_numpy(np.asarray(groups))
        if codes.dtype.is_floating_point or codes.dtype == torch.bool or codes.dim() != 1 or codes.numel() != n:
            raise ValueError(f"auc: groups must be {n} integer codes")
        codes = codes.to(dev, torch.int64)
        if n and int(codes.min()) < 0:
            raise ValueError("auc: group codes must not be negative")
        G = int(codes.max()) + 1 if n else 0
        order = torch.sort(codes, stable=True).indices
        rowptr = torch.zeros(G + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(codes, minlength=G), 0, out=rowptr[1:])
    return engine.auc_values(*engine.auc_groups(s, y, rowptr, order))


def scalar_grouped(arg_series, codes, n_groups, session=None):
    """One ``metrics.auc`` value per group of the ``(score, label)`` columns, or None to decline:
    no session (the device is the session's), ``HM_SQL_BATCH_UDTF=0``, no row, columns that
    ``np.asarray(col.tolist(), dtype=np.float64)`` (the loop's own conversion: None becomes NaN, an
    absent row) refuses or does not make 1-d, a row or group count beyond the engine's limits, or
    no native library."""
    from ..models.base import resolve_device
    from ..ops import auc as engine

    def decline():
        AUC_CALLS["python"] += 1
        return None

    if session is None or len(arg_series) != 2 or os.environ.get("HM_SQL_BATCH_UDTF", "1") == "0":
        return decline()
    try:
        s = np.asarray(arg_series[0].tolist(), dtype=np.float64)
        y = np.asarray(arg_series[1].tolist(), dtype=np.float64)
    except (TypeError, ValueError):
        return decline()
    codes = np.asarray(codes)
    n = len(codes)
    if n == 0 or s.shape != (n,) or y.shape != (n,) or n > engine.ROWS_MAX:
        return decline()
    order = np.argsort(codes, kind="stable")
    rowptr = np.searchsorted(codes[order], np.arange(n_groups + 1)).astype(np.int64)
    if int(np.diff(rowptr).max()) > engine.GROUP_ROWS_MAX:
        return decline()
    dev = resolve_device(session.device)
    try:
        from .. import _native

        _native.hip() if dev.type == "cuda" else _native.host()
    except (RuntimeError, OSError):
        return decline()
    to = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    vals = engine.auc_values(*engine.auc_groups(to(s), to(y), to(rowptr), to(order.astype(np.int64))))
    AUC_CALLS["native"] += 1
    return vals.cpu().tolist()
