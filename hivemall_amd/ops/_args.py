"""The argument checks the native engines share.  Every function takes the engine's message prefix
(``"slim"``, ``"knn"``, ...) first; all raise ``ValueError``."""
from __future__ import annotations

import operator

import torch


def want(op: str, t, name: str, dtype, ndim: int) -> None:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{op}: {name} must be a torch tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{op}: {name} must be {dtype}, got {t.dtype}")
    if t.dim() != ndim:
        raise ValueError(f"{op}: {name} must have {ndim} dimension(s), got shape {tuple(t.shape)}")


def same_device(op: str, ts, names) -> None:
    """Every tensor of ``ts`` is on the device of the first."""
    for t, nm in zip(ts[1:], names[1:]):
        if t.device != ts[0].device:
            raise ValueError(f"{op}: {nm} is on {t.device}, {names[0]} on {ts[0].device}")


def int_in(op: str, v, name: str, lo: int, hi: int | None = None) -> int:
    """``v`` as an int in ``lo..hi``; no ``hi`` means any int32 from ``lo`` up.  Bools and floats
    are refused."""
    rng = f"{lo}..{hi}" if hi is not None else f">= {lo}"
    try:
        if isinstance(v, bool):
            raise TypeError
        v = operator.index(v)
    except TypeError:
        raise ValueError(f"{op}: {name} must be an int in {rng}, got {v!r}") from None
    if not lo <= v <= (2**31 - 1 if hi is None else hi):
        raise ValueError(f"{op}: {name} must be in {rng}, got {v}")
    return v


def all_finite(op: str, x: torch.Tensor, where) -> None:
    """Refuses a floating tensor with a NaN or an infinity; ``where(at)`` turns the flat index of
    the first one (in the contiguous order of ``x``) into the index the message shows."""
    bad = ~torch.isfinite(x)
    if bool(bad.any()):
        at = int(torch.nonzero(bad.reshape(-1))[0])
        raise ValueError(f"{op}: x[{where(at)}] is not finite ({float(x.reshape(-1)[at])})")
