"""ChangeFinder scores (``csrc/kernels/changefinder.hip``, ``csrc/host/changefinder_cpu.cpp``):
the native engine behind ``changefinder -engine native``.

One series ``x[0..N)`` of ``D``-vectors runs through two stages of the sequentially discounting AR
model of order ``k`` (``anomaly.SDAR1D``): stage 1 scores every dimension with rate ``r1`` and
``loss1`` and adds the ``D`` scores to the outlier score ``o_t``; ``y_t`` is the mean of ``o`` over
the last ``min(T1, t + 1)`` points; stage 2 scores ``y`` with ``r2`` and ``loss2``; the
change-point score is the mean of that over the last ``min(T2, t + 1)`` points.  docs/compat.md
("changefinder -engine") has the recurrences.

Every piece of SDAR state is an exponentially weighted sum with the decay ``1 - r``, so the kernel
runs a series as three linear scans per stage, parallel over time in chunks of ``CHUNK`` points;
the OpenMP twin is sequential in time, in the Python path's operation order.  Everything is fp64.
``cuda`` tensors run the gfx950 kernels on the current stream, CPU tensors the twin.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _native
from . import _args

_P = C.c_void_p
_I64 = _native.c_i64
_SIG = ([_P, _I64, _I64, _I64, C.c_int, C.c_double, C.c_double] + [C.c_int] * 4 + [_P] * 11)
_native.register_hip("hm_changefinder", _SIG + [_P])
_native.register_host("hm_changefinder_cpu", _SIG)

CHUNK = 256         # points per workgroup, one lane each
K_MAX = 32          # the covariance sums and Levinson coefficients of a point stay in registers
T_MAX = 1024
LOSSES = ("hellinger", "logloss")


def _rate(v, name: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(f"changefinder: {name} must be a float in (0, 1), got {v!r}")
    v = float(v)
    if not 0.0 < v < 1.0:
        raise ValueError(f"changefinder: {name} must be in (0, 1), got {v}")
    return v


def _loss(v, name: str) -> int:
    if v not in LOSSES:
        raise ValueError(f"changefinder: {name} must be hellinger or logloss, got {v!r}")
    return LOSSES.index(v)


def supports(k, r1, r2, T1, T2, loss1, loss2) -> bool:
    """Whether the options are inside the engine's limits (``changefinder -engine auto`` asks
    before it chooses this engine): ``1 <= k <= 32``, ``0 < r1, r2 < 1``, ``1 <= T1, T2 <= 1024``,
    losses hellinger or logloss."""
    try:
        _args.int_in("changefinder", k, "k", 1, K_MAX)
        _rate(r1, "r1")
        _rate(r2, "r2")
        _args.int_in("changefinder", T1, "T1", 1, T_MAX)
        _args.int_in("changefinder", T2, "T2", 1, T_MAX)
        _loss(loss1, "loss1")
        _loss(loss2, "loss2")
    except ValueError:
        return False
    return True


def changefinder_scores(x: torch.Tensor, k: int = 7, r1: float = 0.02, r2: float = 0.02,
                        T1: int = 7, T2: int = 7, loss1: str = "hellinger",
                        loss2: str = "hellinger"):
    """``(outlier, changepoint)``, both fp64 on the device of ``x`` and of shape ``[N]`` or
    ``[S, N]``, for ``x`` fp64 ``[N]``, ``[S, N]`` (scalar series) or ``[S, N, D]`` (series of
    ``D``-vectors); every ``s`` is its own series."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"changefinder: x must be a torch tensor, got {type(x).__name__}")
    if x.dtype != torch.float64:
        raise ValueError(f"changefinder: x must be {torch.float64}, got {x.dtype}")
    if x.dim() not in (1, 2, 3):
        raise ValueError(f"changefinder: x must be [N], [S, N] or [S, N, D], got shape {tuple(x.shape)}")
    k = _args.int_in("changefinder", k, "k", 1, K_MAX)
    r1, r2 = _rate(r1, "r1"), _rate(r2, "r2")
    T1 = _args.int_in("changefinder", T1, "T1", 1, T_MAX)
    T2 = _args.int_in("changefinder", T2, "T2", 1, T_MAX)
    l1, l2 = _loss(loss1, "loss1"), _loss(loss2, "loss2")
    x3 = x.reshape(1, -1, 1) if x.dim() == 1 else x[:, :, None] if x.dim() == 2 else x
    S, N, D = x3.shape

    def where(at):
        index = (at // (N * D), at // D % N, at % D)
        return index[1] if x.dim() == 1 else index[:x.dim()]

    _args.all_finite("changefinder", x3, where)
    out_shape = tuple(x.shape[:2]) if x.dim() == 3 else tuple(x.shape)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=x.device)   # noqa: E731
    outlier, changepoint = new(S, N), new(S, N)
    if S * N * D == 0:
        return outlier.zero_().reshape(out_shape), changepoint.zero_().reshape(out_shape)
    rows = x3.permute(0, 2, 1).contiguous()                 # [S, D, N]: a row is contiguous in t
    score, y = new(S * D, N), new(S, N)
    p = _native.ptr
    if x.is_cuda:
        nch = -(-N // CHUNK)
        if S * D * nch * (k + 1) > 2**31 - 1:
            raise ValueError(f"changefinder: x of shape {tuple(x.shape)} needs more than 2^31 - 1 "
                             "chunk sums; split the batch")
        # the scan factors: a^(i+1) inside a chunk, (a^CHUNK)^(i+1) over the chunk sums
        steps = torch.arange(1, CHUNK + 1, dtype=torch.float64)
        steps = torch.cat([steps, CHUNK * steps])
        pw1 = torch.pow(torch.tensor(1.0 - r1, dtype=torch.float64), steps).to(x.device)
        pw2 = torch.pow(torch.tensor(1.0 - r2, dtype=torch.float64), steps).to(x.device)
        agg1, car1 = new(S * D * nch), new(S * D * nch)
        aggc, carc = new(S * D * nch * (k + 1)), new(S * D * nch * (k + 1))
        e2 = new(S * D, N)
        _native.call_hip(
            "hm_changefinder", x.device, p(rows), S, D, N, k, r1, r2, T1, T2, l1, l2, p(pw1), p(pw2),
            p(agg1), p(car1), p(aggc), p(carc), p(e2), p(score), p(y), p(outlier), p(changepoint))
    else:
        _native.call_host(
            "hm_changefinder", p(rows), S, D, N, k, r1, r2, T1, T2, l1, l2, *([0] * 7), p(score), p(y),
            p(outlier), p(changepoint))
    return outlier.reshape(out_shape), changepoint.reshape(out_shape)
