"""MinHash signatures over packed feature strings (``csrc/kernels/minhash.hip``,
``csrc/host/minhash_cpu.cpp``): the engine behind ``knn.minhash`` / ``minhashes`` /
``bbit_minhash``.

Contract: for row ``r`` and hash ``h`` in ``0..H-1``, ``sig[r, h]`` is the unsigned minimum over
the row's feature names of ``MurmurHash3_x86_32(utf8(name), seed = (seed0 + h) mod 2^32)``; an
empty row gives 0; duplicated names, values and weights change nothing.  The name of a feature
string is everything before its first ``:`` (``knn._fv``).

The input is a packed list<string> column: ``buf`` (uint8 bytes), ``off`` (int64 [nnz + 1] string
offsets), ``nlen`` (int32 [nnz] name lengths) and ``rowptr`` (int64 [n_rows + 1] strings per row);
``pack_feature_column`` builds it from Python lists or an Arrow column.  The result is int32
``[n_rows, H]`` holding the uint32 bit patterns.  ``cuda`` tensors run the gfx950 kernel on the
current stream, CPU tensors the OpenMP twin; both are integer only and agree bit for bit.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _native
from . import _args, _packed

_P = C.c_void_p
_I64 = _native.c_i64
_native.register_hip("hm_minhash_sig", [_P, _P, _P, _P, _I64, C.c_int, C.c_uint32, _P, _P])
_native.register_host("hm_minhash_sig_cpu", [_P, _P, _P, _P, _I64, C.c_int, C.c_uint32, _P])
_native.register_host("hm_minhash_names", [_P, _P, _I64, _P], restype=_I64)

H_MAX = 1024
# the kernel's tiling (csrc/kernels/minhash.hip); the result depends on none of them
ROWS_PER_WG = 16        # MH_ROWS
FEATS_PER_PASS = 256    # MH_FEATS
BYTES_STAGED = 8192     # MH_BYTES
HASHES_PER_PASS = 256   # MH_HASHES
MAX_GRID = 4096         # MH_MAX_GRID


def minhash_signatures(buf: torch.Tensor, off: torch.Tensor, nlen: torch.Tensor, rowptr: torch.Tensor,
                       num_hashes: int, seed0: int = 0, *, check: bool = True) -> torch.Tensor:
    """int32 [n_rows, num_hashes]: the minhash signature of every row (uint32 bit patterns).
    ``check=False`` skips the passes over ``off``, ``nlen`` and ``rowptr`` (monotone offsets, name
    lengths inside their strings) for a caller that built them itself, as ``pack_feature_column``
    does; dtypes, shapes, devices and the two scalars are always checked."""
    _args.want("minhash", buf, "buf", torch.uint8, 1)
    _args.want("minhash", off, "off", torch.int64, 1)
    _args.want("minhash", nlen, "nlen", torch.int32, 1)
    _args.want("minhash", rowptr, "rowptr", torch.int64, 1)
    _args.same_device("minhash", (buf, off, nlen, rowptr), ("buf", "off", "nlen", "rowptr"))
    H = _args.int_in("minhash", num_hashes, "num_hashes", 1, H_MAX)
    seed0 = _args.int_in("minhash", seed0, "seed0", 0, 2**32 - 1)
    if check:
        _packed.check_offsets("minhash", off, "off", buf)
        _packed.check_offsets("minhash", rowptr, "rowptr")
    elif off.numel() < 1 or rowptr.numel() < 1:
        raise ValueError("minhash: off and rowptr must hold at least one offset")
    nnz = off.numel() - 1
    if nlen.numel() != nnz:
        raise ValueError(f"minhash: nlen must hold {nnz} lengths (off has {nnz + 1} offsets), "
                         f"got {nlen.numel()}")
    if check and int(rowptr[-1]) != nnz:
        raise ValueError(f"minhash: rowptr must end at nnz = {nnz}, got {int(rowptr[-1])}")
    if check and nnz and bool(((nlen < 0) | (nlen.long() > off[1:] - off[:-1])).any()):
        raise ValueError("minhash: nlen[s] must be in 0..off[s + 1] - off[s]")
    n_rows = rowptr.numel() - 1
    out = torch.empty((n_rows, H), dtype=torch.int32, device=buf.device)
    if n_rows == 0:
        return out
    off, nlen, rowptr = (t.contiguous() for t in (off, nlen, rowptr))
    p = _native.ptr
    _packed.launch("hm_minhash_sig", buf, p(off), p(nlen), p(rowptr), n_rows, H, seed0, p(out))
    return out


def cluster_ids(sig: torch.Tensor, key_groups: int) -> torch.Tensor:
    """int32 [n_rows, H / key_groups]: every run of ``key_groups`` hashes folded as ``minhashes``
    does it, ``h = (h * 31 + v) & 0x7FFFFFFF`` over the unsigned ``v``, starting from 0."""
    _args.want("minhash", sig, "sig", torch.int32, 2)
    H = sig.shape[1]
    kg = _args.int_in("minhash", key_groups, "key_groups", 1, max(H, 1))
    if H % kg:
        raise ValueError(f"minhash: key_groups = {kg} does not divide the {H} hashes of sig")
    v = (sig.long() & 0xFFFFFFFF).reshape(sig.shape[0], H // kg, kg)
    h = torch.zeros(v.shape[:2], dtype=torch.int64, device=sig.device)
    for j in range(kg):
        h = (h * 31 + v[:, :, j]) & 0x7FFFFFFF
    return h.to(torch.int32)


def bbit_pack(sig: torch.Tensor, b: int) -> list:
    """The hex strings of ``bbit_minhash``: the lowest ``b`` bits of hash ``i`` at bit ``i * b``."""
    _args.want("minhash", sig, "sig", torch.int32, 2)
    b = _args.int_in("minhash", b, "b", 1, 32)
    n, H = sig.shape
    if n == 0 or H == 0:
        return ["0"] * n
    v = sig.cpu().numpy().view(np.uint32)
    shifts = np.arange(b, dtype=np.uint32)
    out = []
    step = max(1, (1 << 24) // (H * b))                  # rows per piece: the bit image stays small
    for r0 in range(0, n, step):
        bits = ((v[r0:r0 + step, :, None] >> shifts) & 1).astype(np.uint8)        # [rows, H, b]
        packed = np.packbits(bits.reshape(bits.shape[0], -1), axis=1, bitorder="little")
        out.extend(format(int.from_bytes(row.tobytes(), "little"), "x") for row in packed)
    return out


# ------------------------------------------------------------------ packing a column
def _rows(col):
    """A column that is not Arrow yet, as a list of lists for pyarrow, or None: pyarrow would read
    a ``str`` row as a list of characters."""
    import pandas as pd

    if isinstance(col, (pd.Series, np.ndarray)):
        col = col.tolist()
    if isinstance(col, (list, tuple)) and all(r is None or isinstance(r, (list, tuple)) for r in col):
        return col
    return None


def _arrow_list_of_strings(arr):
    """``arr`` when it is a pyarrow list<string> array without NULL features, else None."""
    import pyarrow as pa

    ty = arr.type
    if not (pa.types.is_list(ty) or pa.types.is_large_list(ty)):
        return None
    vt = ty.value_type
    if pa.types.is_null(vt):
        if len(arr.values) != 0:
            return None                                   # lists of NULLs
        return arr.cast(pa.list_(pa.string()))
    if not (pa.types.is_string(vt) or pa.types.is_large_string(vt)):
        return None
    if arr.values.null_count:
        return None                                       # a NULL feature inside a row
    return arr


def _null_rows_are_empty(arr) -> bool:
    if arr.null_count == 0:
        return True
    lo = np.asarray(arr.offsets, dtype=np.int64)
    valid = np.asarray(arr.is_valid())
    return bool(((lo[1:] - lo[:-1])[~valid] == 0).all())


def pack_feature_column(col):
    """``(buf uint8, off int64 [nnz + 1], nlen int32 [nnz], rowptr int64 [n_rows + 1])`` CPU tensors
    for a column of feature-string lists (a sequence / pandas Series of lists of ``str``, or an
    Arrow list<string>); a NULL row counts as an empty row.  None when the column holds anything
    else (ints, dicts, numeric arrays, NULL features) or a ``name:value`` whose value text is not
    a plain decimal: those keep the per-row functions and whatever they raise."""
    import pyarrow as pa

    from ..io.ingest import arrow_buffers

    arr = _packed.as_arrow(col, pa.list_(pa.string()), _rows)
    arr = None if arr is None else _arrow_list_of_strings(arr)
    if arr is None:
        return None
    if not _null_rows_are_empty(arr):
        arr = pa.array([[] if r is None else r for r in arr.to_pylist()], type=arr.type)
    data, so, lo = arrow_buffers(arr)
    nnz = len(so) - 1
    if len(lo) == 0 or int(lo[-1]) != nnz:
        return None
    buf = np.ascontiguousarray(data) if len(data) else np.zeros(1, np.uint8)
    so = np.ascontiguousarray(so, dtype=np.int64)
    nlen = np.empty(nnz, dtype=np.int32)
    bad = int(_native.host().hm_minhash_names(buf.ctypes.data, so.ctypes.data, nnz, nlen.ctypes.data))
    if bad != -1:
        return None
    if not buf.flags.writeable:
        buf = buf.copy()                                  # torch wants a writable array
    return (torch.from_numpy(buf[:len(data)] if len(data) else buf[:0]), torch.from_numpy(so),
            torch.from_numpy(nlen), torch.from_numpy(np.ascontiguousarray(lo, dtype=np.int64)))
