"""HyperLogLog and Bloom sketches over one packed string column (``csrc/kernels/sketch.hip``,
``csrc/host/sketch_cpu.cpp``): the engine behind ``misc.approx_count_distinct`` / ``bloom`` /
``bloom_contains`` / ``bloom_contains_any``.

Contract (``docs/compat.md`` "Sketches"; the classes ``misc.HyperLogLog`` / ``misc.Bloom`` are the
definition).  ``mm3`` is MurmurHash3_x86_32 over the UTF-8 bytes of a value's text, unsigned.

* 64-bit hash: ``h64 = (mm3(s, 0x9747B28C) << 32) | mm3(s, 0x5BD1E995)``.
* HyperLogLog: ``p`` in 4..16, ``m = 2^p``; ``idx = h64 >> (64 - p)``; ``w = (h64 << p) mod 2^64``;
  ``rho = min(clz64(w), 64 - p) + 1`` with ``clz64(0) = 64``; ``reg[g, idx] = max(reg[g, idx], rho)``.
* Histogram: ``hist[g, r]`` = number of registers of group ``g`` equal to ``r``, int32 ``[G, 66]``.
* Estimate: on the host, from ``hist``, with the formulas of ``HyperLogLog.cardinality``:
  ``z = 1 / sum_r hist[r] * 2^-r`` summed from the largest ``r`` down, ``zeros = hist[0]``.  For
  ``p + max(reg) <= 53`` that sum and NumPy's over the registers are both exact, so the estimates
  are the same integer; beyond it they may differ by 1.
* Bloom: ``h1 = mm3(s, 0)``, ``h2 = mm3(s, h1)``; bit ``i_j = (h1 + j * h2) mod m`` for ``j`` in
  ``0..k-1`` in 64-bit arithmetic; bit ``i`` is bit ``i & 7`` of byte ``i >> 3``; ``m`` a multiple of
  32 in 32..2^26, ``k`` in 1..16.

The input is a packed column: ``buf`` (uint8 bytes), ``off`` (int64 [n + 1] offsets) and one int32
group (filter) id per value, in any order; ``pack_value_column`` builds the first two.  ``cuda``
tensors run the gfx950 kernels on the current stream, CPU tensors the OpenMP twin.  Everything is
integer and the merges (max, or) are commutative and idempotent: kernel, twin and the Python
classes agree bit for bit.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from .. import _native
from . import _args, _packed

_P = C.c_void_p
_I64 = _native.c_i64
_native.register_hip("hm_hll_update", [_P, _P, _P, _I64, C.c_int, C.c_int, _P, _P])
_native.register_hip("hm_hll_update_grid", [_P, _P, _P, _I64, C.c_int, C.c_int, _P, C.c_int, _P])
_native.register_hip("hm_hll_hist", [_P, C.c_int, C.c_int, _P, _P])
_native.register_hip("hm_bloom_add", [_P, _P, _P, _I64, C.c_int, _I64, C.c_int, _P, _P])
_native.register_hip("hm_bloom_test", [_P, _P, _P, _I64, _P, C.c_int, _I64, C.c_int, _P, _P])
_native.register_host("hm_hll_update_cpu", [_P, _P, _P, _I64, C.c_int, C.c_int, _P])
_native.register_host("hm_hll_hist_cpu", [_P, C.c_int, C.c_int, _P])
_native.register_host("hm_bloom_add_cpu", [_P, _P, _P, _I64, C.c_int, _I64, C.c_int, _P])
_native.register_host("hm_bloom_test_cpu", [_P, _P, _P, _I64, _P, C.c_int, _I64, C.c_int, _P])

P_MIN, P_MAX = 4, 16
M_MIN, M_MAX = 32, 1 << 26
K_MAX = 16
HIST_BINS = 66
# the kernels' tiling (csrc/kernels/sketch.hip); the result depends on none of them
STRINGS_PER_WG = 256        # SK_STRINGS
BYTES_STAGED = 8192         # SK_BYTES
LDS_REG_BYTES = 64 * 1024   # SK_LDS_REG_BYTES: G * 2^p up to here takes the LDS path
MAX_GRID = 2048             # SK_MAX_GRID
LDS_MAX_GRID = 512          # SK_LDS_MAX_GRID

# how often each engine entry ran (the tests assert the route a SQL query took)
CALLS = {"hll_registers": 0, "hll_histogram": 0, "bloom_bits": 0, "bloom_test": 0}


def _column(buf, off, ids, ids_name: str, n_ids: int, check: bool):
    """The checks shared by every entry; returns n."""
    _args.want("sketch", buf, "buf", torch.uint8, 1)
    _args.want("sketch", off, "off", torch.int64, 1)
    _args.want("sketch", ids, ids_name, torch.int32, 1)
    _args.same_device("sketch", (buf, off, ids), ("buf", "off", ids_name))
    if off.numel() < 1:
        raise ValueError("sketch: off must hold at least one offset")
    n = off.numel() - 1
    if ids.numel() != n:
        raise ValueError(f"sketch: {ids_name} must hold {n} ids (off has {n + 1} offsets), got {ids.numel()}")
    if check:
        _packed.check_offsets("sketch", off, "off", buf)
        if n and int((off[1:] - off[:-1]).max()) >= 2**31:
            raise ValueError("sketch: a value of 2^31 bytes or more")
        if n and (int(ids.min()) < 0 or int(ids.max()) >= n_ids):
            raise ValueError(f"sketch: {ids_name} must be in 0..{n_ids - 1}")
    return n


def _state(t, name: str, shape: tuple, device) -> torch.Tensor:
    """An in/out register file or bitmap: the caller's own tensor, updated in place."""
    _args.want("sketch", t, name, torch.uint8, 2)
    if tuple(t.shape) != shape:
        raise ValueError(f"sketch: {name} must have shape {shape}, got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"sketch: {name} is on {t.device}, buf on {device}")
    if not t.is_contiguous() or t.data_ptr() % 16:
        raise ValueError(f"sketch: {name} must be contiguous and 16-byte aligned")
    return t


def hll_registers(buf: torch.Tensor, off: torch.Tensor, gid: torch.Tensor, G: int, p: int,
                  reg: torch.Tensor | None = None, *, check: bool = True,
                  _lds_grid: int = 0) -> torch.Tensor:
    """uint8 ``[G, 2^p]``: the HyperLogLog registers of every group.  ``reg`` is in/out: the call
    merges into it (and returns it).  ``check=False`` skips the passes over ``off`` and ``gid`` for
    a caller that built them itself."""
    G = _args.int_in("sketch", G, "G", 1, 2**31 - 1)
    p = _args.int_in("sketch", p, "p", P_MIN, P_MAX)
    if (G << p) > 2**31 - 16:
        raise ValueError(f"sketch: G * 2^p = {G << p} registers, at most 2^31 - 16")
    n = _column(buf, off, gid, "gid", G, check)
    dev = buf.device
    if reg is None:
        reg = torch.zeros((G, 1 << p), dtype=torch.uint8, device=dev)
    else:
        _state(reg, "reg", (G, 1 << p), dev)
    CALLS["hll_registers"] += 1
    if n == 0:
        return reg
    off, gid = off.contiguous(), gid.contiguous()
    ptr = _native.ptr
    rest = (ptr(off), ptr(gid), n, G, p, ptr(reg))
    if _lds_grid and buf.is_cuda:                         # benchmarks/sketch_bench.py --sweep
        _packed.launch("hm_hll_update_grid", buf, *rest, int(_lds_grid))
    else:
        _packed.launch("hm_hll_update", buf, *rest)
    return reg


def _p_of(reg: torch.Tensor) -> int:
    m = reg.shape[1]
    p = m.bit_length() - 1
    if m != 1 << p or not P_MIN <= p <= P_MAX:
        raise ValueError(f"sketch: reg must hold 2^p registers per group, p in {P_MIN}..{P_MAX}, got {m}")
    return p


def hll_histogram(reg: torch.Tensor) -> torch.Tensor:
    """int32 ``[G, 66]``: how many registers of each group hold each value."""
    _args.want("sketch", reg, "reg", torch.uint8, 2)
    p = _p_of(reg)
    G = reg.shape[0]
    if G > 2**31 - 1:
        raise ValueError("sketch: too many groups")
    if not reg.is_contiguous() or reg.data_ptr() % 16:
        reg = reg.contiguous().clone()
    hist = torch.empty((G, HIST_BINS), dtype=torch.int32, device=reg.device)
    CALLS["hll_histogram"] += 1
    if G == 0:
        return hist
    args = (_native.ptr(reg), G, p, _native.ptr(hist))
    if reg.is_cuda:
        _native.call_hip("hm_hll_hist", reg.device, *args)
    else:
        _native.call_host("hm_hll_hist", *args)
    return hist


def hll_estimate(hist, p: int) -> list:
    """The cardinality estimate of every group, computed on the host from its histogram with the
    formulas of ``misc.HyperLogLog.cardinality``."""
    p = _args.int_in("sketch", p, "p", P_MIN, P_MAX)
    h = hist.cpu().numpy() if isinstance(hist, torch.Tensor) else np.asarray(hist)
    if h.ndim != 2 or h.shape[1] != HIST_BINS:
        raise ValueError(f"sketch: hist must have shape [G, {HIST_BINS}], got {tuple(h.shape)}")
    m = 1 << p
    alpha = 0.7213 / (1 + 1.079 / m)
    out = []
    for row in h.tolist():
        if sum(row) != m:
            raise ValueError(f"sketch: a histogram of {sum(row)} registers, p = {p} has {m}")
        s = 0.0
        for r in range(HIST_BINS - 1, -1, -1):
            s += row[r] * 2.0 ** -r
        z = 1.0 / s
        e = alpha * m * m * z
        zeros = row[0]
        if e <= 2.5 * m and zeros:
            e = m * math.log(m / zeros)
        out.append(int(round(e)))
    return out


def _bloom_mk(m, k) -> tuple:
    m = _args.int_in("sketch", m, "m", M_MIN, M_MAX)
    if m % 32:
        raise ValueError(f"sketch: m must be a multiple of 32, got {m}")
    return m, _args.int_in("sketch", k, "k", 1, K_MAX)


def bloom_bits(buf: torch.Tensor, off: torch.Tensor, gid: torch.Tensor, G: int, m: int = 65536, k: int = 4,
               bits: torch.Tensor | None = None, *, check: bool = True) -> torch.Tensor:
    """uint8 ``[G, m / 8]``: the Bloom filter of every group (the bytes of ``misc.Bloom.bits``).
    ``bits`` is in/out: the call merges into it (and returns it)."""
    G = _args.int_in("sketch", G, "G", 1, 2**31 - 1)
    m, k = _bloom_mk(m, k)
    n = _column(buf, off, gid, "gid", G, check)
    dev = buf.device
    if bits is None:
        bits = torch.zeros((G, m // 8), dtype=torch.uint8, device=dev)
    else:
        _state(bits, "bits", (G, m // 8), dev)
    CALLS["bloom_bits"] += 1
    if n == 0:
        return bits
    off, gid = off.contiguous(), gid.contiguous()
    ptr = _native.ptr
    _packed.launch("hm_bloom_add", buf, ptr(off), ptr(gid), n, G, m, k, ptr(bits))
    return bits


def bloom_test(bits: torch.Tensor, fid: torch.Tensor, buf: torch.Tensor, off: torch.Tensor, k: int, *,
               check: bool = True) -> torch.Tensor:
    """uint8 ``[n]``: 1 when all ``k`` bits of key ``s`` are set in filter ``fid[s]`` of ``bits``
    (uint8 ``[F, m / 8]``)."""
    _args.want("sketch", bits, "bits", torch.uint8, 2)
    F = bits.shape[0]
    if F < 1 or F > 2**31 - 1:
        raise ValueError(f"sketch: bits must hold at least one filter, got shape {tuple(bits.shape)}")
    m, k = _bloom_mk(bits.shape[1] * 8, k)
    n = _column(buf, off, fid, "fid", F, check)
    dev = buf.device
    if bits.device != dev:
        raise ValueError(f"sketch: bits is on {bits.device}, buf on {dev}")
    if not bits.is_contiguous() or bits.data_ptr() % 4:
        bits = bits.contiguous().clone()
    hit = torch.empty(n, dtype=torch.uint8, device=dev)
    CALLS["bloom_test"] += 1
    if n == 0:
        return hit
    off, fid = off.contiguous(), fid.contiguous()
    ptr = _native.ptr
    _packed.launch("hm_bloom_test", buf, ptr(off), ptr(fid), n, ptr(bits), F, m, k, ptr(hit))
    return hit


# ------------------------------------------------------------------ packing a column
def _values(col):
    """A column that is not Arrow yet, as pyarrow takes it, or None: object columns as a list,
    integer ones as an Arrow array."""
    import pandas as pd
    import pyarrow as pa

    if isinstance(col, pd.Series):
        if col.dtype == object:
            return col.tolist()
        if pd.api.types.is_integer_dtype(col.dtype) and not pd.api.types.is_bool_dtype(col.dtype):
            return pa.Array.from_pandas(col)
        return None
    if isinstance(col, np.ndarray):
        if col.ndim != 1:
            return None
        return pa.array(col) if col.dtype.kind in "iu" else col.tolist() if col.dtype == object else None
    return col


def pack_value_column(col):
    """``(buf uint8, off int64 [n + 1], keep int64 [n])`` CPU tensors for a column of values: the
    UTF-8 text of every non-NULL value back to back, and the positions of those values in the
    column.  Taken: a column of ``str`` (a sequence, an object Series or an Arrow string column)
    and an integer column, as the decimal text ``str(int)`` gives.  None for anything else
    (floats, bools, bytes, nested or mixed values): those keep the per-value Python loop and its
    ``str(v)``."""
    import pyarrow as pa

    from ..io.ingest import string_buffers

    arr = _packed.as_arrow(col, pa.string(), _values)
    if arr is None:
        return None
    ty = arr.type
    if pa.types.is_null(ty):
        arr = pa.array([None] * len(arr), type=pa.string())
    elif pa.types.is_integer(ty):
        arr = arr.cast(pa.large_string())
    elif not (pa.types.is_string(ty) or pa.types.is_large_string(ty)):
        return None
    keep = np.arange(len(arr), dtype=np.int64)
    if arr.null_count:
        keep = np.flatnonzero(np.asarray(arr.is_valid())).astype(np.int64)
        arr = arr.drop_null()
    data, so = string_buffers(arr)
    if len(arr) and int(np.max(so[1:] - so[:-1])) >= 2**31:
        return None
    return (torch.from_numpy(np.array(data, dtype=np.uint8)), torch.from_numpy(np.array(so, dtype=np.int64)),
            torch.from_numpy(keep))
