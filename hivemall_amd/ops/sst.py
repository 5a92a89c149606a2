"""Singular spectrum transformation scores (``csrc/kernels/sst.hip``, ``csrc/host/sst_cpu.cpp``):
the native engine behind ``sst -engine native``.

For a series ``x[0..N)``, window ``w``, ``n`` past and ``m`` current columns, offset ``g`` and
ranks ``r`` / ``k``: with ``need = w + n + max(0, -g) + m`` a point ``t`` with ``t + 1 < need``
scores exactly 0; otherwise, with ``end = t + 1``, the past matrix is
``P[l, i] = x[end + g - m - n + i - w + 1 + l]`` (``w x n``), the current one
``Q0[l, i] = x[end - m + i - w + 1 + l]`` (``w x m``), ``U`` / ``Q`` are their leading
``min(r, w, n)`` / ``min(k, w, m)`` left singular vectors and the score is
``1 - sigma_max(U^T Q)^2``, clamped to [0, 1].  A singular vector with
``sigma_i <= max(rows, cols) * eps * sigma_1`` is in no subspace; two empty subspaces score 0,
exactly one scores 1 (docs/compat.md has the whole contract).

Every SVD is a cyclic one-sided Jacobi with a cap of 30 sweeps, on the matrix scaled by a power
of two (the score does not depend on the scale), so samples of any finite magnitude are fine.
Everything is fp64.  ``cuda`` tensors run the gfx950 kernel on the current stream, CPU tensors
the OpenMP twin.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _native
from . import _args

_P = C.c_void_p
_I64 = _native.c_i64
_native.register_hip("hm_sst_scores", [_P, _I64, _I64] + [C.c_int] * 6 + [_P, _P, _P])
_native.register_host("hm_sst_scores_cpu", [_P, _I64, _I64] + [C.c_int] * 6 + [_P, _P])

DIM_MAX = 64        # rows = one wave; three 64 x 64 fp64 matrices are 96 KiB of LDS
SWEEP_CAP = 30


def supports(w: int, n: int, m: int, g: int, r: int, k: int) -> bool:
    """Whether the shape is inside the engine's limits (``sst -engine auto`` asks before it
    chooses this engine): ``2 <= w <= 64``, ``1 <= n, m <= 64``, ``r, k >= 1``, ``g <= m``."""
    return (2 <= w <= DIM_MAX and 1 <= n <= DIM_MAX and 1 <= m <= DIM_MAX and 1 <= r < 2**31
            and 1 <= k < 2**31 and -(2**31) < g <= m)


def sst_scores(x: torch.Tensor, w: int = 30, n: int | None = None, m: int | None = None,
               g: int | None = None, r: int = 3, k: int = 5, *, return_sweeps: bool = False):
    """fp64 scores with the shape and device of ``x`` (fp64 ``[N]`` or ``[S, N]``, every row its
    own series).  ``n`` and ``m`` default to ``w``, ``g`` to ``-w``.  With ``return_sweeps`` also
    the int32 tensor of the largest sweep count of each point's three Jacobi runs (0 in the
    unscored prefix).  Raises ``RuntimeError`` if a point did not converge in 30 sweeps."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"sst: x must be a torch tensor, got {type(x).__name__}")
    if x.dtype != torch.float64:
        raise ValueError(f"sst: x must be {torch.float64}, got {x.dtype}")
    if x.dim() not in (1, 2):
        raise ValueError(f"sst: x must be [N] or [S, N], got shape {tuple(x.shape)}")
    w = _args.int_in("sst", w, "w", 2, DIM_MAX)
    n = w if n is None else _args.int_in("sst", n, "n", 1, DIM_MAX)
    m = w if m is None else _args.int_in("sst", m, "m", 1, DIM_MAX)
    g = -w if g is None else _args.int_in("sst", g, "g", -(2**31 - 1))
    r = _args.int_in("sst", r, "r", 1)
    k = _args.int_in("sst", k, "k", 1)
    if g > m:
        raise ValueError(f"sst: g must be <= m = {m} (the past windows would reach beyond t), got {g}")
    xs = (x if x.dim() == 2 else x[None]).contiguous()
    S, N = xs.shape
    where = (lambda at: at) if x.dim() == 1 else (lambda at: (at // N, at % N))
    _args.all_finite("sst", xs, where)
    need = w + n + max(0, -g) + m
    out = torch.zeros((S, N), dtype=torch.float64, device=x.device)
    sweeps = torch.zeros((S, N), dtype=torch.int32, device=x.device)
    if S and N >= need:
        args = (_native.ptr(xs), S, N, w, n, m, g, r, k, _native.ptr(out), _native.ptr(sweeps))
        if x.is_cuda:
            _native.call_hip("hm_sst_scores", x.device, *args)
        else:
            _native.call_host("hm_sst_scores", *args)
        capped = sweeps > SWEEP_CAP
        if bool(capped.any()):
            at = int(torch.nonzero(capped.reshape(-1))[0])
            raise RuntimeError(f"sst: the Jacobi SVD of point {where(at)} did not converge in "
                               f"{SWEEP_CAP} sweeps")
    out, sweeps = out.reshape(x.shape), sweeps.reshape(x.shape)
    return (out, sweeps) if return_sweeps else out
