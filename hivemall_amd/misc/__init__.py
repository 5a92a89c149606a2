"""Sketches, geospatial, dataset generator (upstream core/src/main/java/
hivemall/{sketch/hll/ApproxCountDistinctUDAF,sketch/bloom/*,geospatial/*,
dataset/LogisticRegressionDataGeneratorUDTF}.java)."""
from __future__ import annotations

import base64
import math
import random

import numpy as np

from ..registry import udaf, udf, udtf
from ..utils.hashing import murmurhash3


# ------------------------------------------------------------------ HyperLogLog++
class HyperLogLog:
    """HyperLogLog with 2^p registers, 64-bit hashing (two murmur3 halves) and the standard
    small-range (linear counting) correction — the estimator behind approx_count_distinct."""

    def __init__(self, p: int = 15):
        self.p = int(p)
        self.m = 1 << self.p
        self.reg = np.zeros(self.m, dtype=np.uint8)

    @staticmethod
    def _h64(v) -> int:
        s = str(v)
        return ((murmurhash3(s, seed=0x9747B28C) & 0xFFFFFFFF) << 32) | (murmurhash3(s, seed=0x5BD1E995) & 0xFFFFFFFF)

    def add(self, v) -> None:
        h = self._h64(v)
        idx = h >> (64 - self.p)
        w = (h << self.p) & ((1 << 64) - 1)
        rho = 1
        while rho <= 64 - self.p and not (w & (1 << 63)):
            rho += 1
            w = (w << 1) & ((1 << 64) - 1)
        if rho > self.reg[idx]:
            self.reg[idx] = rho

    def merge(self, other: "HyperLogLog") -> None:
        np.maximum(self.reg, other.reg, out=self.reg)

    def cardinality(self) -> int:
        m = self.m
        alpha = 0.7213 / (1 + 1.079 / m)
        z = 1.0 / np.sum(np.power(2.0, -self.reg.astype(np.float64)))
        e = alpha * m * m * z
        zeros = int((self.reg == 0).sum())
        if e <= 2.5 * m and zeros:
            e = m * math.log(m / zeros)
        return int(round(e))


def _acd_options(options) -> tuple:
    """``(p, engine)`` of the option string ``[-p N] [-engine auto|native|python]``."""
    p, engine = 15, "auto"
    o = options[0] if isinstance(options, (list, tuple)) and options else options
    if o:
        toks = str(o).split()
        if "-p" in toks:
            p = int(toks[toks.index("-p") + 1])
        if "-engine" in toks:
            engine = toks[toks.index("-engine") + 1]
            if engine not in ("auto", "native", "python"):
                raise ValueError(f"approx_count_distinct: -engine must be auto, native or python, got {engine!r}")
    return p, engine


@udaf("approx_count_distinct")
def approx_count_distinct(values, options=None):
    p, engine = _acd_options(options)
    if engine == "native":
        values = list(values) if not hasattr(values, "__len__") else values
        return approx_count_distinct_grouped(values, np.zeros(len(values), dtype=np.int32), 1, p)[0]
    h = HyperLogLog(p)
    for v in values:
        if v is not None:
            h.add(v)
    return h.cardinality()


# ---- the native engine (ops/sketch.py): whole columns, every group in one pass.  Contract as
# the classes above: h64 = (mm3(s, 0x9747B28C) << 32) | mm3(s, 0x5BD1E995), idx = h64 >> (64 - p),
# rho = min(clz64(h64 << p), 64 - p) + 1, reg = max(reg, rho); the estimate is computed on the
# host from the register histogram and equals cardinality() while p + max(reg) <= 53 (it may
# differ by 1 beyond).  Bloom: h1 = mm3(s, 0), h2 = mm3(s, h1), bits (h1 + j * h2) mod m.
_NATIVE_MAX_BYTES = 1 << 30          # G * 2^p registers the auto engine will allocate
_BLOOM_TEST_MAX_BYTES = 64 << 20     # F * m / 8 filter bytes the batch forms will stage


def _sketch_device(device):
    from ..models.base import resolve_device

    return resolve_device(device)


def _packed_groups(values, gid, G: int):
    """``(buf, off, gid int32)`` CPU tensors of the non-NULL values, or None when the column does
    not pack (``ops.sketch.pack_value_column``)."""
    import torch

    from ..ops import sketch as sk

    packed = sk.pack_value_column(values)
    if packed is None:
        return None
    buf, off, keep = packed
    g = np.asarray(gid)
    n = len(values)
    if g.ndim != 1 or len(g) != n:
        raise ValueError(f"sketch: gid must hold one group per value ({n}), got shape {g.shape}")
    g = g[keep.numpy()]
    if len(g) and (int(g.min()) < 0 or int(g.max()) >= G):
        raise ValueError(f"sketch: gid must be in 0..{G - 1}")
    return buf, off, torch.from_numpy(np.ascontiguousarray(g, dtype=np.int32))


def _acd_native(values, gid, G: int, p: int, device, strict: bool):
    from ..ops import sketch as sk

    G, p = int(G), int(p)
    if not (sk.P_MIN <= p <= sk.P_MAX) or G < 1 or (G << p) > _NATIVE_MAX_BYTES:
        if strict:
            raise ValueError(f"approx_count_distinct: the native engine takes p in {sk.P_MIN}..{sk.P_MAX} "
                             f"and G * 2^p <= {_NATIVE_MAX_BYTES}, got p = {p}, G = {G}")
        return None
    packed = _packed_groups(values, gid, G)
    if packed is None:
        if strict:
            raise ValueError("approx_count_distinct: the native engine takes a column of str or of "
                             "integers")
        return None
    dev = _sketch_device(device)
    reg = sk.hll_registers(*(t.to(dev) for t in packed), G, p, check=False)      # packed here
    return sk.hll_estimate(sk.hll_histogram(reg), p)


def approx_count_distinct_grouped(values, gid, G: int, p: int = 15, device=None) -> list:
    """``[approx_count_distinct(values of group g, f"-p {p}") for g in range(G)]`` in one native
    pass: ``values`` is a column of ``str`` or of integers (NULLs are skipped), ``gid`` the group of
    every value.  Runs on ``device`` (default: the GPU when there is one)."""
    return _acd_native(values, gid, G, p, device, strict=True)


def _acd_grouped(values, options=None, *, codes, n_groups, session=None):
    """The column-at-once form the SQL executor calls (``registry``): None -> the per-group loop."""
    if options is None:
        p, engine = 15, "auto"
    else:
        try:
            ops = set(options.tolist() if hasattr(options, "tolist") else options)
        except TypeError:
            return None
        if len(ops) != 1:                              # not one constant (or no rows at all)
            return None
        p, engine = _acd_options(ops.pop())
    if engine == "python":
        return None
    return _acd_native(values, codes, n_groups, p, None if session is None else session.device,
                       strict=engine == "native")


def _grouped_adapter(fn):
    def grouped(arg_series, codes, n_groups, session=None):
        return fn(*arg_series, codes=codes, n_groups=n_groups, session=session)
    return grouped


approx_count_distinct.grouped = _grouped_adapter(_acd_grouped)


# ------------------------------------------------------------------ Bloom filters
class Bloom:
    def __init__(self, m: int = 1 << 16, k: int = 4, bits: np.ndarray | None = None):
        self.m, self.k = int(m), int(k)
        self.bits = bits if bits is not None else np.zeros(self.m // 8, dtype=np.uint8)

    def _idx(self, v):
        s = str(v)
        h1 = murmurhash3(s, seed=0) & 0xFFFFFFFF
        h2 = murmurhash3(s, seed=h1) & 0xFFFFFFFF
        return [(h1 + i * h2) % self.m for i in range(self.k)]

    def add(self, v):
        for i in self._idx(v):
            self.bits[i >> 3] |= 1 << (i & 7)

    def contains(self, v) -> bool:
        return all(self.bits[i >> 3] >> (i & 7) & 1 for i in self._idx(v))

    def serialize(self) -> str:
        return f"{self.m}:{self.k}:" + base64.b64encode(self.bits.tobytes()).decode()

    @staticmethod
    def deserialize(s: str) -> "Bloom":
        m, k, b = s.split(":", 2)
        return Bloom(int(m), int(k), np.frombuffer(base64.b64decode(b), dtype=np.uint8).copy())


@udaf("bloom")
def bloom(values):
    b = Bloom()
    for v in values:
        if v is not None:
            b.add(v)
    return b.serialize()


def _bloom_serialize(m: int, k: int, bits) -> list:
    return [f"{m}:{k}:" + base64.b64encode(row.tobytes()).decode() for row in bits.cpu().numpy()]


def _bloom_native(values, gid, G: int, device, strict: bool):
    from ..ops import sketch as sk

    G = int(G)
    m, k = 1 << 16, 4                                  # Bloom()'s defaults, as bloom() uses them
    if G < 1 or G * (m // 8) > _NATIVE_MAX_BYTES:
        if strict:
            raise ValueError(f"bloom: the native engine takes 1..{_NATIVE_MAX_BYTES // (m // 8)} groups")
        return None
    packed = _packed_groups(values, gid, G)
    if packed is None:
        if strict:
            raise ValueError("bloom: the native engine takes a column of str or of integers")
        return None
    dev = _sketch_device(device)
    return _bloom_serialize(m, k, sk.bloom_bits(*(t.to(dev) for t in packed), G, m, k, check=False))


def bloom_grouped(values, gid, G: int, device=None) -> list:
    """``[bloom(values of group g) for g in range(G)]`` (the ``m:k:base64`` strings) in one native
    pass; see ``approx_count_distinct_grouped``."""
    return _bloom_native(values, gid, G, device, strict=True)


def _bloom_grouped_sql(values, *, codes, n_groups, session=None):
    return _bloom_native(values, codes, n_groups, None if session is None else session.device, strict=False)


bloom.grouped = _grouped_adapter(_bloom_grouped_sql)


@udf("bloom_and")
def bloom_and(a, b):
    A, B = Bloom.deserialize(a), Bloom.deserialize(b)
    return Bloom(A.m, A.k, A.bits & B.bits).serialize()


@udf("bloom_or")
def bloom_or(a, b):
    A, B = Bloom.deserialize(a), Bloom.deserialize(b)
    return Bloom(A.m, A.k, A.bits | B.bits).serialize()


@udf("bloom_not")
def bloom_not(a):
    A = Bloom.deserialize(a)
    return Bloom(A.m, A.k, ~A.bits).serialize()


@udf("bloom_contains")
def bloom_contains(a, key):
    return None if a is None else Bloom.deserialize(a).contains(key)


@udf("bloom_contains_any")
def bloom_contains_any(a, keys):
    B = Bloom.deserialize(a)
    return any(B.contains(k) for k in keys)


def _bloom_filter_arg(a, n: int):
    """``(bits uint8 [F, m / 8], fid int32 [n], null bool [n], k)`` for the filter argument of a
    batch call - a constant string or a column, factorised to its distinct strings - or None
    when it is anything else, a filter does not parse, the filters differ in ``(m, k)`` or are
    larger than ``_BLOOM_TEST_MAX_BYTES`` together."""
    import pandas as pd

    if isinstance(a, pd.Series):
        vals = a.tolist()
        if len(vals) != n:
            return None
    elif isinstance(a, str):
        vals = [a] * n if n else []
    else:
        return None
    ids: dict = {}
    fid = np.zeros(n, dtype=np.int32)
    null = np.zeros(n, dtype=bool)
    last, last_id = None, 0
    for r, v in enumerate(vals):
        if v is None:
            null[r] = True
        elif v is last:                                # a constant repeats one object
            fid[r] = last_id
        elif isinstance(v, str):
            last, last_id = v, ids.setdefault(v, len(ids))
            fid[r] = last_id
        else:
            return None
    if not ids:
        return None
    rows, mk = [], None
    for s in ids:                                      # insertion order = id order
        try:
            m, k, b = s.split(":", 2)
            m, k = int(m), int(k)
            bits = np.frombuffer(base64.b64decode(b), dtype=np.uint8)
        except ValueError:
            return None
        if not (32 <= m <= 1 << 26) or m % 32 or not 1 <= k <= 16 or len(bits) != m // 8:
            return None
        if mk is None:
            mk = (m, k)
        elif mk != (m, k):
            return None
        if (len(rows) + 1) * (m // 8) > _BLOOM_TEST_MAX_BYTES:
            return None
        rows.append(bits)
    return np.stack(rows), fid, null, mk[1]


def _bloom_hits(flt, fid, packed, session):
    import torch

    from ..ops import sketch as sk

    dev = _sketch_device(None if session is None else session.device)
    bits, k = torch.from_numpy(flt[0]).to(dev), flt[3]
    buf, off, _ = packed
    return sk.bloom_test(bits, torch.from_numpy(fid).to(dev), buf.to(dev), off.to(dev), k,
                         check=False).cpu().numpy().astype(bool)


def _bloom_result(hit, null):
    import pandas as pd

    vals = [None if z else bool(h) for h, z in zip(hit, null)]
    return pd.Series(vals, dtype=object).infer_objects() if vals else pd.Series([], dtype=object)


def _bloom_contains_batch(a, key, session=None):
    """Column-at-once ``bloom_contains``: a Series, or None (-> the per-row path and whatever it
    raises) unless the keys are a column of str or integers without NULLs and every filter parses
    (``_bloom_filter_arg``).  A NULL filter row stays NULL."""
    import pandas as pd

    from ..ops import sketch as sk

    if not isinstance(key, pd.Series):
        return None
    n = len(key)
    flt = _bloom_filter_arg(a, n)
    packed = sk.pack_value_column(key) if flt is not None else None
    if packed is None or packed[2].numel() != n:
        return None
    return _bloom_result(_bloom_hits(flt, flt[1], packed, session), flt[2])


def _bloom_contains_any_batch(a, keys, session=None):
    """Column-at-once ``bloom_contains_any``: the keys are a list column, tested key by key and
    reduced per row with an any; see ``_bloom_contains_batch``."""
    import pandas as pd

    from ..ops import sketch as sk

    if not isinstance(keys, pd.Series):
        return None
    rows = keys.tolist()
    n = len(rows)
    flt = _bloom_filter_arg(a, n)
    if flt is None:
        return None
    for r in rows:
        if not isinstance(r, (list, tuple, np.ndarray)):
            return None
    lens = np.fromiter((len(r) for r in rows), dtype=np.int64, count=n)
    flat = [k for r in rows for k in (r.tolist() if isinstance(r, np.ndarray) else r)]
    packed = sk.pack_value_column(flat)
    if packed is None or packed[2].numel() != len(flat):
        return None
    row_of = np.repeat(np.arange(n, dtype=np.int64), lens)
    hit = _bloom_hits(flt, np.ascontiguousarray(flt[1][row_of]), packed, session)
    return _bloom_result(np.bincount(row_of[hit], minlength=n) > 0, flt[2])


bloom_contains.batch = _bloom_contains_batch
bloom_contains_any.batch = _bloom_contains_any_batch


# ------------------------------------------------------------------ geospatial (slippy tiles)
@udf("lat2tiley")
def lat2tiley(lat, zoom):
    lat_r = math.radians(float(lat))
    n = 1 << int(zoom)
    return int((1.0 - math.log(math.tan(lat_r) + 1.0 / math.cos(lat_r)) / math.pi) / 2.0 * n)


@udf("lon2tilex")
def lon2tilex(lon, zoom):
    n = 1 << int(zoom)
    return int((float(lon) + 180.0) / 360.0 * n)


@udf("tilex2lon")
def tilex2lon(x, zoom):
    return float(x) / (1 << int(zoom)) * 360.0 - 180.0


@udf("tiley2lat")
def tiley2lat(y, zoom):
    n = math.pi - 2.0 * math.pi * float(y) / (1 << int(zoom))
    return math.degrees(math.atan(math.sinh(n)))


@udf("tile")
def tile(lat, lon, zoom):
    """Tile number ``y * 2^zoom + x``."""
    z = int(zoom)
    return lat2tiley(lat, z) * (1 << z) + lon2tilex(lon, z)


@udf("map_url")
def map_url(lat, lon, zoom, option: str = "-osm"):
    z = int(zoom)
    x, y = lon2tilex(lon, z), lat2tiley(lat, z)
    if "google" in str(option):
        return f"https://www.google.com/maps/@{lat},{lon},{z}z"
    return f"https://tile.openstreetmap.org/{z}/{x}/{y}.png"


@udf("haversine_distance")
def haversine_distance(lat1, lon1, lat2, lon2, mile: bool = False):
    R = 3958.8 if mile else 6371.0
    p1, p2 = math.radians(lat1), math.radians(lat2)
    dp, dl = p2 - p1, math.radians(lon2 - lon1)
    a = math.sin(dp / 2) ** 2 + math.cos(p1) * math.cos(p2) * math.sin(dl / 2) ** 2
    return 2 * R * math.asin(min(1.0, math.sqrt(a)))


# ------------------------------------------------------------------ dataset
@udtf("lr_datagen", per_row=False, cols=("label", "features"))
def lr_datagen(options=None):
    """Synthetic logistic-regression data (LogisticRegressionDataGeneratorUDTF):
    ``-n_examples -n_features -n_dims -eps -prob_one -seed -dense -sort -cl``."""
    import pandas as pd
    o = options[0] if isinstance(options, (list, tuple)) else options
    kv = {"n_examples": 1000, "n_features": 10, "n_dims": 200, "eps": 3.0, "prob_one": 0.6,
          "seed": 43}
    flags = set()
    if o:
        toks = str(o).split()
        i = 0
        while i < len(toks):
            k = toks[i].lstrip("-")
            if k in kv:
                kv[k] = type(kv[k])(toks[i + 1])
                i += 2
            else:
                flags.add(k)
                i += 1
    rng = np.random.default_rng(kv["seed"])
    rows = []
    for _ in range(kv["n_examples"]):
        y = 1 if rng.random() < kv["prob_one"] else 0
        if "dense" in flags:
            x = rng.normal(size=kv["n_dims"]) + (kv["eps"] if y else -kv["eps"]) / kv["n_dims"]
            feats = [float(v) for v in x]
        else:
            idx = rng.choice(kv["n_dims"], size=kv["n_features"], replace=False) + 1
            if "sort" in flags:
                idx = np.sort(idx)
            vals = rng.normal(size=kv["n_features"]) + (0.5 if y else -0.5) * kv["eps"] / 3
            feats = [f"{i}:{v:.6f}" for i, v in zip(idx, vals)]
        rows.append((y if "cl" in flags or True else float(y), feats))
    return pd.DataFrame(rows, columns=["label", "features"])
