"""Pairwise similarity of sparse feature lists (``csrc/kernels/pair_sim.hip``,
``csrc/host/pair_sim_cpu.cpp``): the engine behind ``knn.pair_similarity_batch``,
``knn.pairwise_similarity`` and the column forms of the nine similarity / distance UDFs.

Contract (``docs/compat.md`` "Pair-similarity engine"; the functions of ``hivemall_amd.knn`` are the
definition).

* A set of feature lists is encoded once per distinct list by ``knn._fv`` itself (``FeatureLists``):
  its keys, its value parse, "the last duplicate wins at the first position" and its dict order are
  the functions' own.  Names become int32 ids through one Python dict over those keys.
* For a pair (A, B) the native code computes four primitives with a defined order of additions
  (``DOT``, ``SQ``, ``ABS``, ``INTER``); ``sq`` is each list's left-to-right sum of ``v * v``.
* Each measure is finished from them with single correctly rounded fp64 operations in the
  functions' own order.  ``math.acos`` of the angular measures runs on the host, value by value.

``cuda`` tensors run the gfx950 kernel on the current stream; CPU tensors run the OpenMP twin.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from .. import _native
from . import _args

_P = C.c_void_p
_I64 = _native.c_i64
_native.register_hip("hm_pair_sim", [_P] * 7 + [_I64, _I64, _I64, C.c_int, _P, _P])
_native.register_hip("hm_pair_sim_sq", [_P, _P, _I64, _P, _P])
_native.register_host("hm_pair_sim_cpu", [_P] * 7 + [_I64, _I64, _I64, C.c_int, _P])
_native.register_host("hm_pair_sim_sq_cpu", [_P, _P, _I64, _P])

DOT, SQ, ABS, INTER = range(4)
ALL = (1 << 4) - 1
MEASURES = ("cosine_similarity", "cosine_distance", "angular_similarity", "angular_distance",
            "euclid_distance", "euclid_similarity", "manhattan_distance", "jaccard_similarity",
            "jaccard_distance")
_MASK = {"cosine_similarity": 1 << DOT, "cosine_distance": 1 << DOT, "angular_similarity": 1 << DOT,
         "angular_distance": 1 << DOT, "euclid_distance": 1 << SQ, "euclid_similarity": 1 << SQ,
         "manhattan_distance": 1 << ABS, "jaccard_similarity": 1 << INTER, "jaccard_distance": 1 << INTER}
# euclid_distance squares with ``** 2``, which raises OverflowError where the square leaves fp64; a
# difference of two values inside this bound cannot
VALUE_MAX = 1e153
P_MAX = 2**31 - 1           # pairs of one call

# what the calls did (the tests assert the path taken, not its timing)
STATS = {"calls": 0, "hip": 0, "host": 0, "encoded": 0}

_OP = "pair_sim"


def _call(name: str, dev, *args) -> None:
    if dev.type == "cuda":
        _native.call_hip(name, dev, *args)
        STATS["hip"] += 1
    else:
        _native.call_host(name, *args)
        STATS["host"] += 1


@dataclass
class FeatureLists:
    """``n`` feature lists in CSR form.  ``ptr`` int64 ``[n + 1]``; ``ids`` int32 / ``vals`` fp64
    ``[nnz]`` in entry order (the order of ``knn._fv``'s dict; ids distinct inside a list); ``sids``
    int32 / ``svals`` fp64 ``[nnz]`` the same entries ascending by id inside a list, for lookup by
    binary search; ``sq`` fp64 ``[n]`` the left-to-right sum of ``v * v`` (filled by the engine:
    ``fill_sq``); ``names`` the id -> name list."""
    ptr: torch.Tensor
    ids: torch.Tensor
    vals: torch.Tensor
    sids: torch.Tensor
    svals: torch.Tensor
    sq: torch.Tensor | None
    max_len: int
    names: list | None = None

    @property
    def n_lists(self) -> int:
        return self.ptr.numel() - 1

    @property
    def device(self):
        return self.ptr.device

    def lengths(self) -> torch.Tensor:
        return self.ptr[1:] - self.ptr[:-1]

    def to(self, device) -> "FeatureLists":
        mv = lambda t: None if t is None else t.to(device)          # noqa: E731
        return FeatureLists(mv(self.ptr), mv(self.ids), mv(self.vals), mv(self.sids), mv(self.svals),
                            mv(self.sq), self.max_len, self.names)


def fill_sq(lists: FeatureLists) -> FeatureLists:
    """Computes ``lists.sq`` on the lists' device (``hm_pair_sim_sq``)."""
    sq = torch.zeros(lists.n_lists, dtype=torch.float64, device=lists.device)
    if lists.n_lists:
        _call("hm_pair_sim_sq", lists.device, _native.ptr(lists.ptr), _native.ptr(lists.vals), lists.n_lists,
              _native.ptr(sq))
    lists.sq = sq
    return lists


def from_dicts(dicts, device="cpu") -> FeatureLists:
    """The ``FeatureLists`` of ``{name: float}`` dicts (what ``knn._fv`` returns), entry order = dict
    order, on ``device`` with ``sq`` filled."""
    vocab: dict = {}
    lens = np.fromiter(map(len, dicts), dtype=np.int64, count=len(dicts))
    nnz = int(lens.sum())
    ids = np.fromiter((vocab.setdefault(k, len(vocab)) for d in dicts for k in d), dtype=np.int64, count=nnz)
    if len(vocab) > 2**31 - 1:
        raise ValueError(f"{_OP}: more than 2^31 - 1 distinct names")
    vals = np.fromiter((v for d in dicts for v in d.values()), dtype=np.float64, count=nnz)
    ptr = np.zeros(len(dicts) + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    owner = np.repeat(np.arange(len(dicts), dtype=np.int64), lens)
    order = np.argsort((owner << 32) | ids, kind="stable")         # by (list, id); ids are distinct in a list
    ids = ids.astype(np.int32)
    t = torch.from_numpy
    lists = FeatureLists(t(ptr), t(ids), t(vals), t(ids[order]), t(vals[order]), None,
                         int(lens.max()) if len(lens) else 0, list(vocab))
    STATS["encoded"] += len(dicts)
    return fill_sq(lists.to(device))


def available(device) -> bool:
    """Whether the native library that serves ``device`` loads."""
    try:
        _native.hip() if torch.device(device).type == "cuda" else _native.host()
    except (RuntimeError, OSError):
        return False
    return True


def sum_is_sequential() -> bool:
    """The functions add with ``sum()``: left to right up to Python 3.11, compensated from 3.12.  The
    engine adds left to right and never emulates compensation (the probe of the ranking engine)."""
    from ..evaluation import ranking

    return bool(ranking.SUM_IS_SEQUENTIAL)


def supports(device) -> bool:
    return sum_is_sequential() and available(device)


def _is_column(x) -> bool:
    import pandas as pd

    if isinstance(x, pd.Series):
        return True
    if isinstance(x, (list, tuple)):
        return all(r is None or isinstance(r, (list, tuple, np.ndarray)) for r in x) and \
            any(r is not None for r in x)
    return False


def _rows(x) -> list:
    return x.tolist() if hasattr(x, "tolist") else list(x)


def encode_lists(rows, device="cpu"):
    """``(lists, index)``: a ``FeatureLists`` on ``device`` holding every distinct list of ``rows``
    once and the int32 numpy array of each row's list.  Identical lists are parsed once: by object
    identity first, then by content.  A NULL row encodes as the empty list.  None where
    ``encode_columns`` declines."""
    from .. import knn

    if not supports(device):
        return None
    rows = rows if isinstance(rows, list) else list(rows)
    # distinct objects, vectorised: the rows stay alive in `rows`, so their ids are theirs alone
    obj_ids = np.fromiter(map(id, rows), dtype=np.int64, count=len(rows))
    _, first, inverse = np.unique(obj_ids, return_index=True, return_inverse=True)
    dicts, by_content, slot = [], {}, np.empty(len(first), dtype=np.int32)
    for u in np.argsort(first, kind="stable").tolist():        # lists numbered by first appearance
        row = rows[first[u]]
        if row is None:
            key = ()
        elif isinstance(row, (list, tuple, np.ndarray)):
            key = tuple(row.tolist() if isinstance(row, np.ndarray) else row)
            if not all(type(f) is str for f in key):
                return None
        else:
            return None
        at = by_content.get(key)
        if at is None:
            try:
                d = knn._fv(list(key))
            except Exception:                       # noqa: BLE001 - the per-row loop raises it
                return None
            if not all(math.isfinite(v) and abs(v) <= VALUE_MAX for v in d.values()):
                return None
            at = by_content[key] = len(dicts)
            dicts.append(d)
        slot[u] = at
    return from_dicts(dicts, device), slot[inverse.reshape(-1)]


def encode_columns(a, b, device="cpu"):
    """``(lists, ia, ib)`` of two feature columns, or of a column and one constant list (the query
    vector form; either side): a ``FeatureLists`` on ``device`` holding every distinct list once and
    the int32 numpy index arrays of the rows.  A column is a Series, or a list of lists / None;
    a constant is one list of ``"name[:value]"`` strings or None.  An N x M cross join calls
    ``knn._fv`` at most N + M times (``encode_lists``).

    None (the per-row functions serve) when an element of a list is not a ``str`` (dense arrays,
    minhash signatures, maps), a value is not finite or beyond ``VALUE_MAX``, ``knn._fv`` raises,
    both sides are constants, the columns differ in length, a row is neither a list nor NULL, the
    native library is missing or this Python's ``sum()`` compensates."""
    col_a, col_b = _is_column(a), _is_column(b)
    if not (col_a or col_b):
        return None
    rows_a = _rows(a) if col_a else [a]
    rows_b = _rows(b) if col_b else [b]
    if col_a and col_b and len(rows_a) != len(rows_b):
        return None
    enc = encode_lists(rows_a + rows_b, device)
    if enc is None:
        return None
    lists, index = enc
    ia, ib = index[: len(rows_a)], index[len(rows_a):]
    n = max(len(rows_a), len(rows_b))
    if not col_a:
        ia = np.repeat(ia, n)
    if not col_b:
        ib = np.repeat(ib, n)
    return lists, np.ascontiguousarray(ia), np.ascontiguousarray(ib)


# ------------------------------------------------------------------ primitives
def _check_lists(lists) -> None:
    if not isinstance(lists, FeatureLists):
        raise ValueError(f"{_OP}: lists must be a FeatureLists, got {type(lists).__name__}")
    if lists.sq is None:
        fill_sq(lists)


def _check_index(lists: FeatureLists, t, name: str, check: bool) -> torch.Tensor:
    _args.want(_OP, t, name, torch.int32, 1)
    _args.same_device(_OP, (lists.ptr, t), ("lists", name))
    if check and t.numel() and (int(t.min()) < 0 or int(t.max()) >= lists.n_lists):
        raise ValueError(f"{_OP}: {name} must index the {lists.n_lists} lists (0..{lists.n_lists - 1})")
    return t.contiguous()


def _launch(lists: FeatureLists, ia, ib, P: int, M: int, mask: int, out: torch.Tensor) -> None:
    STATS["calls"] += 1
    if P == 0 or mask == 0:
        return
    if P > P_MAX:
        raise ValueError(f"{_OP}: at most {P_MAX} pairs a call, got {P}")
    ptr = _native.ptr
    _call("hm_pair_sim", lists.device, ptr(lists.ptr), ptr(lists.ids), ptr(lists.vals), ptr(lists.sids),
          ptr(lists.svals), ptr(ia), ptr(ib), P, M, lists.max_len, mask, ptr(out))


def pair_primitives(lists: FeatureLists, ia: torch.Tensor, ib: torch.Tensor, mask: int = ALL, *,
                    check: bool = True) -> torch.Tensor:
    """fp64 ``[4, P]``: planes ``DOT, SQ, ABS, INTER`` of the pairs ``(ia[p], ib[p])`` (int32 ``[P]``
    indices into ``lists``).  Planes ``mask`` leaves out are zero.  ``check=False`` skips the range
    check of the indices (a device read) for callers that built them."""
    _check_lists(lists)
    ia = _check_index(lists, ia, "ia", check)
    ib = _check_index(lists, ib, "ib", check)
    if ia.numel() != ib.numel():
        raise ValueError(f"{_OP}: ia holds {ia.numel()} pairs, ib {ib.numel()}")
    mask = _args.int_in(_OP, mask, "mask", 0, ALL)
    out = torch.zeros((4, ia.numel()), dtype=torch.float64, device=lists.device)
    _launch(lists, ia, ib, ia.numel(), 0, mask, out)
    return out


def pair_primitives_cross(lists: FeatureLists, a_idx: torch.Tensor, b_idx: torch.Tensor, mask: int = ALL, *,
                          check: bool = True) -> torch.Tensor:
    """fp64 ``[4, N, M]``: the planes of every pair ``(a_idx[i], b_idx[j])``; no pair arrays are
    materialised."""
    _check_lists(lists)
    a_idx = _check_index(lists, a_idx, "a_idx", check)
    b_idx = _check_index(lists, b_idx, "b_idx", check)
    mask = _args.int_in(_OP, mask, "mask", 0, ALL)
    N, M = a_idx.numel(), b_idx.numel()
    out = torch.zeros((4, N, M), dtype=torch.float64, device=lists.device)
    _launch(lists, a_idx, b_idx, N * M, M, mask, out)
    return out


# ------------------------------------------------------------------ finishing
def _measure(measure) -> str:
    if measure not in _MASK:
        raise ValueError(f"{_OP}: measure must be one of {', '.join(MEASURES)}, got {measure!r}")
    return measure


def _angular(c: torch.Tensor) -> torch.Tensor:
    """``1 - acos(clamp(c)) / pi`` with ``math.acos`` on the host, value by value."""
    host = c.reshape(-1).cpu().tolist()
    sim = [1.0 - math.acos(max(-1.0, min(1.0, v))) / math.pi for v in host]
    return torch.tensor(sim, dtype=torch.float64).reshape(c.shape).to(c.device)


def _sqrt(t: torch.Tensor) -> torch.Tensor:
    """The correctly rounded fp64 square root.  torch's vectorised CPU ``sqrt`` is not (it differs
    from ``math.sqrt`` in the last bit on about one value in a hundred); NumPy's is."""
    if t.device.type == "cpu":
        return torch.from_numpy(np.sqrt(t.contiguous().numpy()))
    return torch.sqrt(t)


def _finish(measure: str, prim: torch.Tensor, sq_a, sq_b, len_a, len_b) -> torch.Tensor:
    """The measure from the primitive planes; ``sq_*`` / ``len_*`` broadcast against a plane."""
    if measure in ("cosine_similarity", "cosine_distance", "angular_similarity", "angular_distance"):
        na, nb = _sqrt(sq_a), _sqrt(sq_b)
        den = na * nb
        ok = (na > 0) & (nb > 0)
        c = torch.where(ok, prim[DOT] / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(den))
        if measure == "cosine_similarity":
            return c
        if measure == "cosine_distance":
            return 1.0 - c
        s = _angular(c)
        return s if measure == "angular_similarity" else 1.0 - s
    if measure in ("euclid_distance", "euclid_similarity"):
        d = _sqrt(prim[SQ])
        return d if measure == "euclid_distance" else 1.0 / (1.0 + d)
    if measure == "manhattan_distance":
        return prim[ABS]
    inter = prim[INTER]
    union = (len_a + len_b).to(torch.float64) - inter
    some = union > 0
    j = torch.where(some, inter / torch.where(some, union, torch.ones_like(union)), torch.zeros_like(union))
    return j if measure == "jaccard_similarity" else 1.0 - j


def pair_measures(lists: FeatureLists, ia: torch.Tensor, ib: torch.Tensor, measure: str, *,
                  check: bool = True) -> torch.Tensor:
    """fp64 ``[P]`` on the lists' device: ``measure`` (one of ``MEASURES``) of the pairs
    ``(ia[p], ib[p])``."""
    measure = _measure(measure)
    prim = pair_primitives(lists, ia, ib, _MASK[measure], check=check)
    a, b = ia.long(), ib.long()
    lens = lists.lengths()
    return _finish(measure, prim, lists.sq[a], lists.sq[b], lens[a], lens[b])


def pair_measures_cross(lists: FeatureLists, a_idx: torch.Tensor, b_idx: torch.Tensor, measure: str, *,
                        check: bool = True) -> torch.Tensor:
    """fp64 ``[N, M]``: ``measure`` of every pair ``(a_idx[i], b_idx[j])``."""
    measure = _measure(measure)
    prim = pair_primitives_cross(lists, a_idx, b_idx, _MASK[measure], check=check)
    a, b = a_idx.long(), b_idx.long()
    lens = lists.lengths()
    return _finish(measure, prim, lists.sq[a][:, None], lists.sq[b][None, :], lens[a][:, None], lens[b][None, :])
