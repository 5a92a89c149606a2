"""The host side of a packed string column: ``buf`` (uint8 bytes) + ``off`` (int64 [n + 1] offsets,
string ``s`` = ``buf[off[s]:off[s + 1]]``), as the string kernels of ``csrc/kernels/strspan.h`` and
their OpenMP twins take it.  Shared by ``ops.minhash``, ``ops.sketch`` and ``utils.hashing``."""
from __future__ import annotations

import ctypes as C

import torch

from .. import _native
from . import _args

_native.register_hip("hm_mhash", [_native.c_p, _native.c_p, _native.c_i64, C.c_uint32, C.c_int32,
                                  _native.c_p, _native.c_p])


def check_offsets(op: str, off: torch.Tensor, name: str, buf: torch.Tensor | None = None) -> None:
    """``off`` starts at 0, is non-decreasing and (with ``buf``) ends inside ``buf``."""
    if off.numel() < 1:
        raise ValueError(f"{op}: {name} must hold at least one offset")
    if int(off[0]) != 0:
        raise ValueError(f"{op}: {name} must start at 0, got {int(off[0])}")
    if off.numel() > 1 and bool((off[1:] < off[:-1]).any()):
        raise ValueError(f"{op}: {name} must be non-decreasing")
    if buf is not None and int(off[-1]) > buf.numel():
        raise ValueError(f"{op}: {name} ends at {int(off[-1])}, buf holds {buf.numel()} bytes")


def pad16(buf: torch.Tensor) -> torch.Tensor:
    """The string kernels stage bytes in whole aligned 16-B chunks: a base that is 16-B aligned and
    a length that is a multiple of 16 keep every such chunk inside the allocation."""
    n = buf.numel()
    if n and n % 16 == 0 and buf.data_ptr() % 16 == 0:
        return buf
    out = torch.zeros(max(16, (n + 15) // 16 * 16), dtype=torch.uint8, device=buf.device)
    out[:n] = buf
    return out


def launch(name: str, buf: torch.Tensor, *rest) -> None:
    """Runs string engine ``name`` on ``(buf, *rest)``: the gfx950 launcher on the current stream
    for a ``cuda`` buffer (padded as the kernels need it), the OpenMP twin ``<name>_cpu`` otherwise
    (which wants a buffer it can take the address of)."""
    buf = buf.contiguous()
    if buf.is_cuda:
        buf = pad16(buf)
        _native.call_hip(name, buf.device, _native.ptr(buf), *rest)
    else:
        if buf.numel() == 0:
            buf = torch.zeros(1, dtype=torch.uint8)
        _native.call_host(name, _native.ptr(buf), *rest)


def mhash_packed(buf: torch.Tensor, off: torch.Tensor, num_features: int, seed: int) -> torch.Tensor:
    """int32 ``[n]``: ``mhash`` of every string of a ``cuda`` column (``csrc/kernels/hashing.hip``),
    in ``1..num_features``; ``num_features <= 0`` gives the raw signed 32-bit MurmurHash3."""
    _args.want("mhash", buf, "buf", torch.uint8, 1)
    _args.want("mhash", off, "off", torch.int64, 1)
    _args.same_device("mhash", (buf, off), ("buf", "off"))
    if not buf.is_cuda:
        raise ValueError(f"mhash: buf must be on a cuda device, got {buf.device}")
    if off.numel() < 1:
        raise ValueError("mhash: off must hold at least one offset")
    num_features = _args.int_in("mhash", num_features, "num_features", -2**31, 2**31 - 1)
    seed = _args.int_in("mhash", seed, "seed", 0, 2**32 - 1)
    n = off.numel() - 1
    out = torch.empty(n, dtype=torch.int32, device=buf.device)
    if n:
        off = off.contiguous()
        launch("hm_mhash", buf, _native.ptr(off), n, seed, num_features, _native.ptr(out))
    return out


def as_arrow(col, empty_type, plain):
    """One ``pyarrow.Array`` for a column, or None when it is nothing pyarrow reads as one.  Arrow
    arrays and Arrow-backed Series pass; chunks are combined.  Anything else goes through the
    caller's ``plain(col)``, which returns a list or tuple for ``pyarrow.array`` to infer (an empty
    one becomes ``empty_type``), an Arrow array, or None to refuse the column."""
    import pandas as pd
    import pyarrow as pa

    arr = col
    if isinstance(arr, pd.Series) and isinstance(arr.dtype, pd.ArrowDtype):
        arr = arr.array._pa_array
    try:
        if not isinstance(arr, (pa.Array, pa.ChunkedArray)):
            arr = plain(arr)
        if not isinstance(arr, (pa.Array, pa.ChunkedArray)):
            if not isinstance(arr, (list, tuple)):
                return None
            # inferred: mixed columns fail or come out as a type the caller refuses
            arr = pa.array(arr) if len(arr) else pa.array([], type=empty_type)
    except (pa.ArrowInvalid, pa.ArrowTypeError, pa.ArrowNotImplementedError, UnicodeError, OverflowError):
        return None
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.chunk(0) if arr.num_chunks == 1 else arr.combine_chunks()
        if isinstance(arr, pa.ChunkedArray):
            return None
    return arr
