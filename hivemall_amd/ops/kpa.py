"""``train_kpa``'s native engine (``csrc/kernels/kpa.hip``, ``csrc/host/kpa_cpu.cpp``): PA-I on the
explicit degree-2 polynomial expansion, as ``models.recommend.KPA.fit`` / ``_kpa_score`` define it.

Contract (``docs/compat.md`` "KPA engine").

* Rows are parsed by ``recommend._fv`` itself; names become int32 ids in first-seen order through one
  Python dict; rows become CSR (``ptr`` int64, ``ids`` int32, ``vals`` fp64) in entry order; labels
  become +-1 fp64 by ``float(lab) > 0``.  ``pair_base[r]`` counts the pair occurrences before row
  ``r``; the ordered pair key is ``(id_a << 32) | id_b`` for positions ``a < b``.
* ``build_table`` (kernel A) inserts every pair occurrence into an open-addressing table, chunk of
  rows by chunk, and ranks the used slots by first occurrence: the compact slot numbering of ``w3``
  and of the model table.
* ``train`` (kernel B) is the sequential learner: one workgroup, every row in order, ``iters`` passes.
* ``score`` (kernel C) probes the finished table, one wave a row.

``cuda`` tensors run the gfx950 kernels on the current stream, CPU tensors the C++ twin, which is
the Python learner bit for bit.  ``Decline`` says why an input stays with the Python loop.
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
_F64 = C.c_double
_native.register_hip("hm_kpa_table", [_P, _P, _P, _I64, _I64, _I64, _P, _P, _I64, _P, _P, _P])
_native.register_hip("hm_kpa_train", [_P] * 6 + [_I64, C.c_int] + [_F64] * 5 + [_P] * 5)
_native.register_hip("hm_kpa_score", [_P, _P, _P, _I64, _P, _P, _I64, _P, _P, _P, _P, _F64, _F64, _F64, _P, _P])
_native.register_host("hm_kpa_table_cpu", [_P, _P, _P, _I64, _I64, _I64, _P, _P, _I64, _P, _P])
_native.register_host("hm_kpa_train_cpu", [_P] * 6 + [_I64, C.c_int] + [_F64] * 5 + [_P] * 4)
_native.register_host("hm_kpa_score_cpu", [_P, _P, _P, _I64, _P, _P, _I64, _P, _P, _P, _P, _F64, _F64, _F64, _P])

MAX_LEN = 128               # entries of a row: the trainer's workgroup holds 8,128 pairs
# x ** 4 raises OverflowError beyond ~1e77 and the sums leave fp64 long before; inside this bound
# neither the learner's ``**`` nor a sum over 8,256 terms can
VALUE_MAX = 1e30
NAMES_MAX = 2**31 - 1       # int32 ids
OCC_MAX = 2**27             # pair occurrences of one training table (a table of at most 2^28 slots)
PAIR_BUDGET = 2**24         # pair occurrences of one table launch
_I64_MAX = 2**63 - 1

# what served (the tests assert the path taken): native launches by device kind, Python fits / scorings
STATS = {"hip": 0, "host": 0, "python": 0}

_OP = "kpa"


class Decline(Exception):
    """The engine cannot prove itself equal to the learner on this input; the message says why."""


def _call(name: str, dev, *args) -> None:
    if dev.type == "cuda":
        _native.call_hip(name, dev, *args)
        STATS["hip"] += 1
    else:
        _native.call_host(name, *args)
        STATS["host"] += 1


def available(device) -> bool:
    """Whether the native library that serves ``device`` loads."""
    try:
        _native.hip() if torch.device(device).type == "cuda" else _native.host()
    except (RuntimeError, OSError):
        return False
    return True


@dataclass
class Rows:
    """``n`` rows in CSR form on one device.  ``ptr`` int64 ``[n + 1]``; ``ids`` int32 / ``vals``
    fp64 ``[nnz]`` in entry order (``ids`` -1 marks a name a frozen vocabulary lacks); ``y`` fp64
    ``[n]`` in {-1, +1} or None; ``pair_base`` int64 ``[n + 1]``, the running count of
    ``len (len - 1) / 2``."""
    ptr: torch.Tensor
    ids: torch.Tensor
    vals: torch.Tensor
    y: torch.Tensor | None
    pair_base: torch.Tensor
    base_host: np.ndarray

    @property
    def n_rows(self) -> int:
        return self.ptr.numel() - 1

    @property
    def n_occ(self) -> int:
        return int(self.base_host[-1])

    @property
    def device(self):
        return self.ptr.device


def encode(features, labels=None, vocab: dict | None = None, *, frozen: bool = False, device="cpu") -> Rows:
    """The rows as tensors on ``device``.  Training (``frozen=False``): ``vocab`` grows in first-seen
    order and a row that repeats a name declines.  Scoring (``frozen=True``): a name outside
    ``vocab`` encodes as -1.  Declines: an entry ``_fv`` cannot parse, a value that is not finite or
    beyond ``VALUE_MAX``, a row of more than ``MAX_LEN`` entries, more than ``NAMES_MAX`` names."""
    from ..models.recommend import _fv

    vocab = {} if vocab is None else vocab
    try:
        parsed = [[_fv(f) for f in feats] for feats in features]
    except (ValueError, TypeError) as ex:
        raise Decline(f"an entry does not parse ({ex})") from None
    y = None
    if labels is not None:
        try:
            signs = [1.0 if float(lab) > 0 else -1.0 for lab in labels]
        except (ValueError, TypeError) as ex:
            raise Decline(f"a label does not parse ({ex})") from None
        n = min(len(parsed), len(signs))                        # the learner zips the two columns
        parsed, y = parsed[:n], torch.tensor(signs[:n], dtype=torch.float64)
    lens = np.fromiter(map(len, parsed), dtype=np.int64, count=len(parsed))
    if len(lens) and int(lens.max()) > MAX_LEN:
        raise Decline(f"a row holds {int(lens.max())} entries, the engine serves {MAX_LEN}")
    nnz = int(lens.sum())
    names = [h for xs in parsed for h, _ in xs]
    vals = np.fromiter((x for xs in parsed for _, x in xs), dtype=np.float64, count=nnz)
    if not bool(np.all(np.abs(vals) <= VALUE_MAX)):             # also false for a NaN
        raise Decline(f"a value is not finite or beyond {VALUE_MAX:g}")
    if frozen:
        ids = np.fromiter((vocab.get(h, -1) for h in names), dtype=np.int64, count=nnz)
    else:
        ids = np.fromiter((vocab.setdefault(h, len(vocab)) for h in names), dtype=np.int64, count=nnz)
        if len(vocab) > NAMES_MAX:
            raise Decline(f"more than {NAMES_MAX} distinct names")
        owner = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
        if len(np.unique((owner << 32) | ids)) != nnz:
            raise Decline("a row repeats a name (the learner then steps one weight twice in sequence)")
    ptr = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    base = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens * (lens - 1) // 2, out=base[1:])
    t = lambda a: torch.from_numpy(a).to(device)                # noqa: E731
    return Rows(t(ptr), t(ids.astype(np.int32)), t(vals), None if y is None else y.to(device), t(base), base)


def _check_rows(rows) -> None:
    if not isinstance(rows, Rows):
        raise ValueError(f"{_OP}: rows must be a Rows, got {type(rows).__name__}")
    _args.want(_OP, rows.ptr, "ptr", torch.int64, 1)
    _args.want(_OP, rows.ids, "ids", torch.int32, 1)
    _args.want(_OP, rows.vals, "vals", torch.float64, 1)
    _args.want(_OP, rows.pair_base, "pair_base", torch.int64, 1)
    _args.same_device(_OP, (rows.ptr, rows.ids, rows.vals, rows.pair_base), ("ptr", "ids", "vals", "pair_base"))
    if rows.ptr.numel() < 1 or rows.pair_base.numel() != rows.ptr.numel():
        raise ValueError(f"{_OP}: ptr and pair_base must both hold rows + 1 offsets")
    lens = (rows.ptr[1:] - rows.ptr[:-1]).cpu().numpy()
    if int(rows.ptr[0]) != 0 or (len(lens) and (int(lens.min()) < 0 or int(lens.max()) > MAX_LEN)) or \
            int(rows.ptr[-1]) != rows.ids.numel() or rows.vals.numel() != rows.ids.numel():
        raise ValueError(f"{_OP}: ptr must ascend from 0 to len(ids) in steps of at most {MAX_LEN}")
    base = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens * (lens - 1) // 2, out=base[1:])
    if not np.array_equal(base, rows.pair_base.cpu().numpy()) or not np.array_equal(base, rows.base_host):
        raise ValueError(f"{_OP}: pair_base must be the running count of len (len - 1) / 2")


@dataclass
class PairTable:
    """The finished pair table.  ``keys`` int64 ``[cap]`` (-1 = empty) and ``remap`` int32 ``[cap]``
    (table slot -> compact slot, -1 = empty), both None when no pair exists; ``ckeys`` int64
    ``[slots]``, the keys in first-seen order; ``occ`` int32, the compact slot of every pair
    occurrence; ``chunks``, the launches the build took."""
    keys: torch.Tensor | None
    remap: torch.Tensor | None
    ckeys: torch.Tensor
    occ: torch.Tensor
    chunks: int

    @property
    def slots(self) -> int:
        return self.ckeys.numel()

    @property
    def cap_mask(self) -> int:
        return 0 if self.keys is None else self.keys.numel() - 1


def build_table(rows: Rows, *, capacity: int | None = None, pair_budget: int = PAIR_BUDGET) -> PairTable:
    """Kernel A over the rows, in chunks of at most ``pair_budget`` pair occurrences (one row at
    least), into a table of ``capacity`` slots: a power of two, by default the smallest that holds
    twice the occurrences.  Raises ``ValueError`` when the finished table is more than half full."""
    _check_rows(rows)
    dev, n_occ = rows.device, rows.n_occ
    if rows.ids.numel() and int(rows.ids.min()) < 0:
        raise ValueError(f"{_OP}: training rows hold ids >= 0")
    pair_budget = _args.int_in(_OP, pair_budget, "pair_budget", 1)
    if n_occ > OCC_MAX:
        raise Decline(f"{n_occ} pair occurrences, the table serves {OCC_MAX}")
    if n_occ == 0:
        return PairTable(None, None, torch.empty(0, dtype=torch.int64, device=dev),
                         torch.empty(0, dtype=torch.int32, device=dev), 0)
    cap = 1 << max(1, (2 * n_occ - 1).bit_length()) if capacity is None else \
        _args.int_in(_OP, capacity, "capacity", 2, 2**31)
    if cap & (cap - 1):
        raise ValueError(f"{_OP}: capacity must be a power of two, got {cap}")
    keys = torch.full((cap,), -1, dtype=torch.int64, device=dev)
    first = torch.full((cap,), _I64_MAX, dtype=torch.int64, device=dev)
    occ = torch.empty(n_occ, dtype=torch.int32, device=dev)
    full = torch.zeros(1, dtype=torch.int32, device=dev)
    ptr = _native.ptr
    base, r0, chunks = rows.base_host, 0, 0
    while r0 < rows.n_rows:
        r1 = max(r0 + 1, int(np.searchsorted(base, base[r0] + pair_budget, side="right")) - 1)
        _call("hm_kpa_table", dev, ptr(rows.ptr), ptr(rows.ids), ptr(rows.pair_base), r0, r1,
              int(base[r1] - base[r0]), ptr(keys), ptr(first), cap - 1, ptr(occ), ptr(full))
        r0, chunks = r1, chunks + 1
    used = torch.nonzero(keys != -1).reshape(-1)
    if int(full) or 2 * used.numel() > cap:
        raise ValueError(f"{_OP}: {used.numel()} distinct pairs overfill a table of {cap} slots (load factor > 0.5)")
    order = used[torch.sort(first[used]).indices]               # the used slots by first occurrence
    remap = torch.full((cap,), -1, dtype=torch.int32, device=dev)
    remap[order] = torch.arange(order.numel(), dtype=torch.int32, device=dev)
    return PairTable(keys, remap, keys[order], remap[occ.long()], chunks)


def train(rows: Rows, table: PairTable, n_names: int, *, iters: int, c: float, pkc: float):
    """Kernel B: ``(w0 [1], w1 [names], w2 [names], w3 [slots])`` fp64 after ``iters`` passes of
    PA-I over the rows in order, from zero weights."""
    _check_rows(rows)
    dev = rows.device
    n_names = _args.int_in(_OP, n_names, "n_names", 0, NAMES_MAX)
    iters = _args.int_in(_OP, iters, "iters", 0)
    if rows.y is None:
        raise ValueError(f"{_OP}: training rows need labels")
    _args.want(_OP, rows.y, "y", torch.float64, 1)
    _args.want(_OP, table.occ, "occ", torch.int32, 1)
    _args.same_device(_OP, (rows.ptr, rows.y, table.occ), ("ptr", "y", "occ"))
    if rows.y.numel() != rows.n_rows or table.occ.numel() != rows.n_occ:
        raise ValueError(f"{_OP}: y holds one label a row and occ one slot a pair occurrence")
    if rows.ids.numel() and (int(rows.ids.min()) < 0 or int(rows.ids.max()) >= n_names):
        raise ValueError(f"{_OP}: ids must index the {n_names} names")
    if table.occ.numel() and (int(table.occ.min()) < 0 or int(table.occ.max()) >= table.slots):
        raise ValueError(f"{_OP}: occ must index the {table.slots} slots")
    if not pkc > 0:
        raise ValueError(f"{_OP}: pkc must be > 0, got {pkc}")
    zeros = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)      # noqa: E731
    w0, w1, w2, w3 = zeros(1), zeros(n_names), zeros(n_names), zeros(table.slots)
    ptr = _native.ptr
    if rows.n_rows and iters:
        _call("hm_kpa_train", dev, ptr(rows.ptr), ptr(rows.ids), ptr(rows.vals), ptr(rows.y), ptr(rows.pair_base),
              ptr(table.occ), rows.n_rows, iters, float(c), float(pkc), float(pkc), math.sqrt(2 * pkc),
              math.sqrt(2), ptr(w0), ptr(w1), ptr(w2), ptr(w3))
    return w0, w1, w2, w3


@dataclass
class Model:
    """A fitted learner on one device: the vocabulary (name -> id, first-seen order), the weights
    and the pair table."""
    vocab: dict
    pkc: float
    w0: torch.Tensor
    w1: torch.Tensor
    w2: torch.Tensor
    w3: torch.Tensor
    table: PairTable

    @property
    def device(self):
        return self.w0.device

    def pair_ids(self):
        """``(a, b)`` int64 numpy arrays: the two name ids of every slot, in first-seen order."""
        k = self.table.ckeys.cpu().numpy()
        return k >> 32, k & 0xFFFFFFFF

    def dicts(self):
        """``(w1, w2, w3)`` as the learner's dicts, keys in its insertion order."""
        from collections import defaultdict

        names = list(self.vocab)
        a, b = self.pair_ids()
        w3 = zip(zip(map(names.__getitem__, a.tolist()), map(names.__getitem__, b.tolist())), self.w3.tolist())
        return (defaultdict(float, zip(names, self.w1.tolist())), defaultdict(float, zip(names, self.w2.tolist())),
                defaultdict(float, w3))


def fit(features, labels, *, iters: int = 1, c: float = 1.0, pkc: float = 1.0, device="cpu",
        capacity: int | None = None, pair_budget: int = PAIR_BUDGET) -> Model:
    """The learner's ``fit`` on ``device``; ``Decline`` where the Python loop has to serve."""
    if not pkc > 0:
        raise Decline(f"-pkc {pkc} is not > 0")
    if not math.isfinite(c) or not math.isfinite(pkc):
        raise Decline("-c or -pkc is not finite")
    if iters < 1:
        raise Decline(f"-iters {iters} reads no row")
    device = torch.device(device)
    vocab: dict = {}
    rows = encode(features, labels, vocab, device=device)
    table = build_table(rows, capacity=capacity, pair_budget=pair_budget)
    w0, w1, w2, w3 = train(rows, table, len(vocab), iters=iters, c=c, pkc=pkc)
    return Model(vocab, float(pkc), w0, w1, w2, w3, table)


def score(model: Model, features) -> torch.Tensor:
    """Kernel C: fp64 ``[n]`` on the model's device, ``_kpa_score`` of every row.  A name or a pair
    the model never saw weighs 0.0.  Declines as ``encode`` does."""
    dev = model.device
    rows = encode(features, None, model.vocab, frozen=True, device=dev)
    _check_rows(rows)
    t = model.table
    n_names = model.w1.numel()
    for w, name in ((model.w0, "w0"), (model.w1, "w1"), (model.w2, "w2"), (model.w3, "w3")):
        _args.want(_OP, w, name, torch.float64, 1)
    _args.same_device(_OP, (rows.ptr, model.w0, model.w1, model.w2, model.w3), ("rows", "w0", "w1", "w2", "w3"))
    if model.w0.numel() != 1 or model.w2.numel() != n_names or model.w3.numel() != t.slots:
        raise ValueError(f"{_OP}: w0 [1], w1 / w2 [names], w3 [slots]")
    if rows.ids.numel() and int(rows.ids.max()) >= n_names:
        raise ValueError(f"{_OP}: ids must index the {n_names} names")
    if t.keys is not None and (t.remap.numel() != t.keys.numel() or int(t.remap.max()) >= t.slots):
        raise ValueError(f"{_OP}: remap must map the table onto the {t.slots} slots")
    out = torch.zeros(rows.n_rows, dtype=torch.float64, device=dev)
    ptr = _native.ptr
    if rows.n_rows:
        _call("hm_kpa_score", dev, ptr(rows.ptr), ptr(rows.ids), ptr(rows.vals), rows.n_rows, ptr(t.keys),
              ptr(t.remap), t.cap_mask, ptr(model.w0), ptr(model.w1), ptr(model.w2), ptr(model.w3),
              float(model.pkc), math.sqrt(2 * model.pkc), math.sqrt(2), ptr(out))
    return out
