"""Similarity / distance / LSH / top-k (upstream core/src/main/java/hivemall/
knn/{similarity,distance,lsh}/*.java, tools/EachTopKUDTF.java).

Row-wise functions take Hivemall feature arrays (``"name:value"`` strings, or plain numeric
arrays for the dense forms).  ``pairwise_cosine`` / ``topk_similar`` are the batched device
paths: an MFMA-backed GEMM (torch.matmul on ROCm -> hipBLASLt) over L2-normalised dense
matrices followed by ``torch.topk``.  ``topk_similar_csc`` is their sparse sibling: exact fp64
cosine top-k between the columns of a CSC matrix of any height (``ops/knn_sparse.py``: one
workgroup per query column, the candidates' dots accumulated in LDS; no dense matrix), which
is what ``train_slim`` needs as its neighbour lists.  ``cosine_knn`` is its SQL surface.
``pair_similarity_batch`` / ``pairwise_similarity`` and the ``.batch`` forms of the nine sparse
similarity / distance functions run whole columns of feature lists on ``ops/pair_sim.py``.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from ..registry import udf, udtf
from ..utils.hashing import murmurhash3


def _fv(x) -> dict:
    """Feature array -> {name: value}."""
    if x is None:
        return {}
    if isinstance(x, dict):
        return {k: float(v) for k, v in x.items()}
    out = {}
    for i, f in enumerate(x):
        if isinstance(f, str):
            p = f.find(":")
            if p < 0:
                out[f] = 1.0
            else:
                out[f[:p]] = float(f[p + 1:])
        elif isinstance(f, (int, np.integer)) and not isinstance(f, bool):
            out[int(f)] = 1.0
        else:
            out[i] = float(f)
    return out


def _dense_pair(a, b):
    if a is not None and len(a) and not isinstance(list(a)[0], str):
        return np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return None


# ------------------------------------------------------------------ similarity
@udf("cosine_similarity", "cosine_sim")
def cosine_similarity(a, b):
    A, B = _fv(a), _fv(b)
    dot = sum(v * B.get(k, 0.0) for k, v in A.items())
    na = math.sqrt(sum(v * v for v in A.values()))
    nb = math.sqrt(sum(v * v for v in B.values()))
    return dot / (na * nb) if na > 0 and nb > 0 else 0.0


@udf("jaccard_similarity")
def jaccard_similarity(a, b, k: int = 128):
    """Jaccard of two feature sets (or of two minhash signature arrays of length k)."""
    if a is None or b is None:
        return 0.0
    if len(a) and isinstance(list(a)[0], (int, np.integer)) and len(a) == len(b) and len(a) == k:
        return float(np.mean(np.asarray(a) == np.asarray(b)))
    A, B = set(_fv(a)), set(_fv(b))
    u = len(A | B)
    return len(A & B) / u if u else 0.0


@udf("angular_similarity")
def angular_similarity(a, b):
    c = max(-1.0, min(1.0, cosine_similarity(a, b)))
    return 1.0 - math.acos(c) / math.pi


@udf("euclid_similarity")
def euclid_similarity(a, b):
    return 1.0 / (1.0 + euclid_distance(a, b))


@udf("distance2similarity")
def distance2similarity(d):
    return 1.0 / (1.0 + float(d))


@udtf("dimsum_mapper", per_row=True, cols=("j", "k", "b_jk"))
def dimsum_mapper(row, col_norms, options=None):
    """DIMSUM all-pairs similarity mapper: emits (j, k, a_ij*a_ik / (|c_j||c_k|)) sampled with
    probability min(1, γ / (|c_j||c_k|)); ``-threshold`` sets γ = 4·log(n)/threshold."""
    import random
    gamma = 1e30
    if options:
        toks = str(options).split()
        if "-threshold" in toks:
            t = float(toks[toks.index("-threshold") + 1])
            gamma = 4.0 * math.log(max(2, len(col_norms))) / t
    R = _fv(row)
    items = sorted(R.items(), key=lambda kv: str(kv[0]))
    rng = random.Random(42)
    for ai, (j, vj) in enumerate(items):
        nj = float(col_norms.get(j, 0.0)) if isinstance(col_norms, dict) else 0.0
        if nj == 0:
            continue
        for k, vk in items[ai + 1:]:
            nk = float(col_norms.get(k, 0.0))
            if nk == 0:
                continue
            p = min(1.0, gamma / (nj * nk))
            if rng.random() < p:
                yield (j, k, vj * vk / (min(math.sqrt(gamma), nj) * min(math.sqrt(gamma), nk)))


# ------------------------------------------------------------------ distance
@udf("euclid_distance")
def euclid_distance(a, b):
    d = _dense_pair(a, b)
    if d is not None:
        return float(np.linalg.norm(d[0] - d[1]))
    A, B = _fv(a), _fv(b)
    keys = set(A) | set(B)
    return math.sqrt(sum((A.get(k, 0.0) - B.get(k, 0.0)) ** 2 for k in keys))


@udf("cosine_distance")
def cosine_distance(a, b):
    return 1.0 - cosine_similarity(a, b)


@udf("angular_distance")
def angular_distance(a, b):
    return 1.0 - angular_similarity(a, b)


@udf("manhattan_distance")
def manhattan_distance(a, b):
    d = _dense_pair(a, b)
    if d is not None:
        return float(np.abs(d[0] - d[1]).sum())
    A, B = _fv(a), _fv(b)
    return sum(abs(A.get(k, 0.0) - B.get(k, 0.0)) for k in set(A) | set(B))


@udf("minkowski_distance")
def minkowski_distance(a, b, p: float):
    p = float(p)
    A, B = _fv(a), _fv(b)
    s = sum(abs(A.get(k, 0.0) - B.get(k, 0.0)) ** p for k in set(A) | set(B))
    return s ** (1.0 / p)


@udf("jaccard_distance")
def jaccard_distance(a, b, k: int = 128):
    return 1.0 - jaccard_similarity(a, b, k)


@udf("hamming_distance")
def hamming_distance(a, b):
    """Bit differences of two ints or of two long arrays (bitsets)."""
    if isinstance(a, (int, np.integer)):
        return bin((int(a) ^ int(b)) & ((1 << 64) - 1)).count("1")
    return sum(bin((int(x) ^ int(y)) & ((1 << 64) - 1)).count("1") for x, y in zip(a, b))


@udf("popcnt")
def popcnt(a):
    if isinstance(a, (int, np.integer)):
        return bin(int(a) & ((1 << 64) - 1)).count("1")
    return sum(bin(int(x) & ((1 << 64) - 1)).count("1") for x in a)


@udf("kld")
def kld(mu1, sigma1, mu2, sigma2):
    """KL divergence between two univariate Gaussians N(mu1, sigma1) || N(mu2, sigma2)
    (sigma = variance)."""
    return 0.5 * (math.log(sigma2 / sigma1) + sigma1 / sigma2 + (mu1 - mu2) ** 2 / sigma2 - 1.0)


# ------------------------------------------------------------------ LSH
def _minhash_values(features, num_hashes: int, key_groups: int, seed0: int = 0):
    F = _fv(features)
    names = [str(k) for k in F]
    sig = []
    for h in range(num_hashes):
        m = None
        for n in names:
            v = murmurhash3(n, seed=seed0 + h) & 0xFFFFFFFF
            if m is None or v < m:
                m = v
        sig.append(m if m is not None else 0)
    return sig


@udf("minhashes")
def minhashes(features, no_weight: bool = False, num_hashes: int = 5, key_groups: int = 2):
    """Minhash signature (``num_hashes`` groups of ``key_groups`` concatenated hashes)."""
    sig = _minhash_values(features, int(num_hashes) * int(key_groups), int(key_groups))
    kg = int(key_groups)
    out = []
    for g in range(int(num_hashes)):
        part = sig[g * kg:(g + 1) * kg]
        h = 0
        for v in part:
            h = (h * 31 + v) & 0x7FFFFFFF
        out.append(h)
    return out


@udtf("minhash", per_row=True, cols=("clusterid", "item"))
def minhash(item, features, options=None):
    """Emit (clusterid, item) for every minhash group of the item's features."""
    nh, kg = 5, 2
    if options:
        toks = str(options).split()
        if "-n" in toks:
            nh = int(toks[toks.index("-n") + 1])
        if "-k" in toks:
            kg = int(toks[toks.index("-k") + 1])
    for c in minhashes(features, False, nh, kg):
        yield (c, item)


@udf("bbit_minhash")
def bbit_minhash(features, num_hashes: int = 128, b: int = 1):
    """b-bit minwise hashing: the lowest ``b`` bits of each of ``num_hashes`` minhashes packed
    into a hex string."""
    sig = _minhash_values(features, int(num_hashes), 1)
    bits = 0
    for i, v in enumerate(sig):
        bits |= (v & ((1 << int(b)) - 1)) << (i * int(b))
    return format(bits, "x")


# The column-at-once forms: one pass of ops/minhash.py (the gfx950 kernel, or its OpenMP twin on the
# CPU) over the whole packed column instead of num_hashes * len(row) ctypes calls per row.  The
# results equal the per-row functions above, row for row; a column the engine does not take
# (pack_feature_column -> None) goes through them.
def _engine_range(num_hashes: int, key_groups: int = 1) -> bool:
    from ..ops.minhash import H_MAX

    return num_hashes >= 1 and key_groups >= 1 and num_hashes * key_groups <= H_MAX


def _column_signatures(col, num_hashes: int, device=None):
    """int32 [n_rows, num_hashes] on ``device``, or None when the column cannot be packed."""
    from ..models.base import resolve_device
    from ..ops import minhash as mh

    packed = mh.pack_feature_column(col)
    if packed is None:
        return None
    dev = resolve_device(device)
    return mh.minhash_signatures(*(t.to(dev) for t in packed), num_hashes, check=False)   # packed here


def minhash_signatures(col, num_hashes: int, device=None) -> torch.Tensor:
    """int32 [n_rows, num_hashes] (uint32 bit patterns): per row of the feature column, the
    unsigned minimum over its feature names of MurmurHash3_x86_32 under the seeds
    ``0..num_hashes-1``; 0 for an empty or NULL row.  ``col`` is a sequence / Series of lists of
    ``"name[:value]"`` strings or an Arrow list<string>.  Runs on ``device`` (default: the GPU
    when there is one)."""
    sig = _column_signatures(col, num_hashes, device)
    if sig is None:
        raise ValueError("minhash_signatures wants a column of lists of 'name[:value]' strings "
                         "with plain decimal values")
    return sig


def minhashes_batch(col, num_hashes: int = 5, key_groups: int = 2, device=None) -> list:
    """``[minhashes(row, False, num_hashes, key_groups) for row in col]`` in one native pass."""
    from ..ops import minhash as mh

    nh, kg = int(num_hashes), int(key_groups)
    sig = _column_signatures(col, nh * kg, device) if _engine_range(nh, kg) else None
    if sig is None:
        return [minhashes(r, False, nh, kg) for r in _rows_of(col)]
    return mh.cluster_ids(sig, kg).cpu().numpy().tolist()


def bbit_minhash_batch(col, num_hashes: int = 128, b: int = 1, device=None) -> list:
    """``[bbit_minhash(row, num_hashes, b) for row in col]`` in one native pass."""
    from ..ops import minhash as mh

    nh, bb = int(num_hashes), int(b)
    sig = _column_signatures(col, nh, device) if _engine_range(nh) and 1 <= bb <= 32 else None
    if sig is None:
        return [bbit_minhash(r, nh, bb) for r in _rows_of(col)]
    return mh.bbit_pack(sig, bb)


def _rows_of(col):
    if hasattr(col, "to_pylist"):
        return col.to_pylist()
    return col.tolist() if hasattr(col, "tolist") else list(col)


def _session_device(session):
    return None if session is None else session.device


def _minhash_batch(item, features, options=None, session=None):
    """Column-at-once ``minhash(item, features [, options])``: ``(rows_idx, [clusterid, item])``,
    or None (-> the per-row path) for a non-constant option string, a ``-n * -k`` product outside
    the engine's range or a feature column the engine does not take."""
    nh, kg = 5, 2
    if options is not None:
        if isinstance(options, str):
            ops = {options}
        else:
            try:
                ops = set(options)
            except TypeError:
                return None
        if len(ops) != 1:
            return None
        options = ops.pop()
        if options:
            try:
                toks = str(options).split()
                if "-n" in toks:
                    nh = int(toks[toks.index("-n") + 1])
                if "-k" in toks:
                    kg = int(toks[toks.index("-k") + 1])
            except (ValueError, IndexError):
                return None                      # the per-row path raises it
    if not _engine_range(nh, kg):
        return None
    from ..ops import minhash as mh

    sig = _column_signatures(features, nh * kg, _session_device(session))
    if sig is None:
        return None
    ids = mh.cluster_ids(sig, kg).cpu().numpy()
    items = _rows_of(item)
    if len(items) != ids.shape[0]:
        return None
    rows_idx = np.repeat(np.arange(ids.shape[0], dtype=np.int64), nh)
    return rows_idx, [ids.reshape(-1).astype(np.int64).tolist(), [items[i] for i in rows_idx]]


_minhash_batch.wants_session = True
minhash.batch = _minhash_batch
minhash.batch_select = True        # also taken by SELECT minhash(...) (sql/executor._select_udtf)


def _udf_column(features):
    """(column, NULL mask) of a UDF's first argument when it is a whole column, else None."""
    import pandas as pd

    if not isinstance(features, pd.Series):
        return None
    if isinstance(features.dtype, pd.ArrowDtype):
        return features, features.isna().to_numpy()
    vals = features.tolist()
    return vals, np.fromiter((v is None for v in vals), dtype=bool, count=len(vals))


def _udf_result(vals: list, null, null_first: bool):
    import pandas as pd

    if null_first and null.any():
        vals = [None if m else v for v, m in zip(vals, null)]
    return pd.Series(vals, dtype=object).infer_objects() if vals else pd.Series([], dtype=object)


def _const_int(v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise TypeError
    return int(v)


def _minhashes_udf_batch(features, no_weight=False, num_hashes=5, key_groups=2, session=None,
                         null_first=True):
    """Column-at-once ``minhashes``: a Series, or None (-> the per-row path) unless the features
    are a column and the other arguments int constants in the engine's range.  ``null_first``:
    rows whose features are NULL stay NULL (the SQL rule for a NULL first argument)."""
    from ..ops import minhash as mh

    cm = _udf_column(features)
    try:
        nh, kg = _const_int(num_hashes), _const_int(key_groups)
    except TypeError:
        return None
    if cm is None or not _engine_range(nh, kg):
        return None
    sig = _column_signatures(cm[0], nh * kg, _session_device(session))
    if sig is None:
        return None
    return _udf_result(mh.cluster_ids(sig, kg).cpu().numpy().tolist(), cm[1], null_first)


def _bbit_minhash_udf_batch(features, num_hashes=128, b=1, session=None, null_first=True):
    """Column-at-once ``bbit_minhash``; see ``_minhashes_udf_batch``."""
    from ..ops import minhash as mh

    cm = _udf_column(features)
    try:
        nh, bb = _const_int(num_hashes), _const_int(b)
    except TypeError:
        return None
    if cm is None or not _engine_range(nh) or not 1 <= bb <= 32:
        return None
    sig = _column_signatures(cm[0], nh, _session_device(session))
    if sig is None:
        return None
    return _udf_result(mh.bbit_pack(sig, bb), cm[1], null_first)


minhashes.batch = _minhashes_udf_batch
bbit_minhash.batch = _bbit_minhash_udf_batch


# ------------------------------------------------------------------ pair similarity, column at once
# The native route of the nine sparse similarity / distance functions above: ops/pair_sim.py (the
# gfx950 kernel, or its OpenMP twin on the CPU) parses every distinct feature list once with _fv and
# computes whole columns of pairs.  It is taken only where the result provably equals the
# functions' (docs/compat.md "Pair-similarity engine"); every other input is declined and goes
# through them, with their results and their exceptions.  Direct calls on two lists keep their loop.
PAIR_SIM_CALLS = {"native": 0, "python": 0}        # how the column calls were served (tests assert the route)
_PAIR_FUNCTIONS = {f.__name__: f for f in (
    cosine_similarity, cosine_distance, angular_similarity, angular_distance, euclid_distance,
    euclid_similarity, manhattan_distance, jaccard_similarity, jaccard_distance)}


def _pair_function(measure):
    if measure not in _PAIR_FUNCTIONS:
        raise ValueError(f"pair_sim: measure must be one of {', '.join(_PAIR_FUNCTIONS)}, got {measure!r}")
    return _PAIR_FUNCTIONS[measure]


def _pair_native(a, b, measure, device):
    """fp64 [P] tensor of ``measure`` over the rows of two columns (or a column and a constant
    list) from the engine, or None where it declines."""
    from ..models.base import resolve_device
    from ..ops import pair_sim as ps

    if os.environ.get("HM_SQL_BATCH_UDTF", "1") == "0":
        return None
    dev = resolve_device(device)
    enc = ps.encode_columns(a, b, dev)
    if enc is None:
        return None
    lists, ia, ib = enc
    return ps.pair_measures(lists, torch.from_numpy(ia).to(dev), torch.from_numpy(ib).to(dev), measure,
                            check=False)                    # the indices were built here


def pair_similarity_batch(a, b, measure: str, device=None):
    """``[measure(x, y) for x, y in zip(a, b)]`` in one native pass: an fp64 tensor on ``device``
    (default: the GPU when there is one).  ``a`` and ``b`` are columns (a Series or a list of lists
    of ``"name[:value]"`` strings, None for NULL) of one length, or one of them is a single
    constant list, the query vector.  ``measure`` is the name of one of the nine functions
    (``"cosine_similarity"``, ..., ``"jaccard_distance"``).  Inputs the engine declines (dense
    arrays, maps, non-finite values, ...) are served by the function itself, row by row, and come
    back as a list."""
    from ..ops import pair_sim as ps

    fn = _pair_function(measure)
    res = _pair_native(a, b, measure, device)
    if res is not None:
        PAIR_SIM_CALLS["native"] += 1
        return res
    PAIR_SIM_CALLS["python"] += 1
    col_a, col_b = ps._is_column(a), ps._is_column(b)
    if not (col_a or col_b):
        raise ValueError("pair_sim: one of a, b must be a column of feature lists")
    rows_a, rows_b = (_rows_of(a) if col_a else None), (_rows_of(b) if col_b else None)
    n = len(rows_a if col_a else rows_b)
    if col_a and col_b and len(rows_b) != n:
        raise ValueError(f"pair_sim: a holds {n} rows, b {len(rows_b)}")
    return [fn(rows_a[i] if col_a else a, rows_b[i] if col_b else b) for i in range(n)]


def pairwise_similarity(A, B, measure: str, device=None) -> torch.Tensor:
    """fp64 ``[N, M]`` on ``device``: ``measure(A[i], B[j])`` for every pair of the two columns of
    feature lists, without materialising the pairs (the cross form of the engine).  Inputs the
    engine declines are served by the function itself, pair by pair."""
    from ..models.base import resolve_device
    from ..ops import pair_sim as ps

    fn = _pair_function(measure)
    rows_a, rows_b = _rows_of(A), _rows_of(B)
    dev = resolve_device(device)
    enc = ps.encode_lists(rows_a + rows_b, dev) if os.environ.get("HM_SQL_BATCH_UDTF", "1") != "0" else None
    if enc is None:
        PAIR_SIM_CALLS["python"] += 1
        vals = [[fn(x, y) for y in rows_b] for x in rows_a]
        return torch.tensor(vals, dtype=torch.float64).reshape(len(rows_a), len(rows_b)).to(dev)
    PAIR_SIM_CALLS["native"] += 1
    lists, index = enc
    index = torch.from_numpy(index).to(dev)
    return ps.pair_measures_cross(lists, index[: len(rows_a)].contiguous(), index[len(rows_a):].contiguous(),
                                  measure, check=False)


def _pair_udf_batch(measure: str, extra_args: int = 0):
    """The column-at-once form of one pair UDF for the SQL executor: a Series, or None (-> the
    per-row loop) unless one of the two arguments is a column and the engine takes the input.
    Rows whose first argument is NULL stay NULL (the SQL rule for a NULL first argument); a NULL
    second argument is the empty list, as in the function."""
    def batch(a, b, *rest, session=None, null_first=True):
        import pandas as pd

        if len(rest) > extra_args:
            return None                                     # the per-row loop raises it
        res = None
        if (isinstance(a, pd.Series) or isinstance(b, pd.Series)) and a is not None:
            res = _pair_native(a, b, measure, _session_device(session))
        if res is None:
            PAIR_SIM_CALLS["python"] += 1
            return None
        PAIR_SIM_CALLS["native"] += 1
        if isinstance(a, pd.Series):
            null = np.fromiter((v is None for v in a.tolist()), dtype=bool, count=len(a))
        else:
            null = np.zeros(res.numel(), dtype=bool)
        return _udf_result(res.cpu().tolist(), null, null_first)
    return batch


for _name, _fn in _PAIR_FUNCTIONS.items():
    # jaccard_*'s third argument k belongs to the minhash-signature form, which is declined
    _fn.batch = _pair_udf_batch(_name, extra_args=1 if _name.startswith("jaccard") else 0)
del _name, _fn


# ------------------------------------------------------------------ top-k
def _each_top_k_python(k, group, score, *cols):
    """The definition of ``each_top_k``: the per-row loop the native engine is checked against and
    the path of every input the engine declines."""
    import pandas as pd
    kk = int(k[0] if isinstance(k, (list, tuple)) else k)
    rev = kk > 0
    kk = abs(kk)
    rows = []
    n = len(group)
    order = {}
    for i in range(n):
        order.setdefault(group[i], []).append(i)
    for g, idxs in order.items():
        idxs = sorted(idxs, key=lambda i: score[i], reverse=rev)[:kk]
        for r, i in enumerate(idxs, start=1):
            rows.append((r, score[i]) + tuple(c[i] for c in cols))
    return pd.DataFrame(rows, columns=["rank", "key"] + [f"c{i}" for i in range(len(cols))])


# The native route: ops/each_top_k.py (the gfx950 kernels, or their OpenMP twin on the CPU) returns
# the selected row indices in output order, which is all the loop above computes.  It is taken
# only where the result provably equals the loop's (docs/compat.md "each_top_k engine"); every
# other input is declined and goes through the loop, with its results and its exceptions.
EACH_TOP_K_CALLS = {"native": 0, "python": 0}      # how the calls were served (tests assert the route)
_FP64_EXACT = 2**53


def _etk_k(k):
    """The int the loop reads from its first argument; None where it would raise."""
    try:
        return int(k[0] if isinstance(k, (list, tuple)) else k)
    except Exception:
        return None


def _etk_scores(score):
    """The score column as fp64 when that loses nothing: a list of Python ints and floats (no
    bool, None, Decimal, str or NumPy scalar), or a numeric array, with every int inside
    +-2^53 and no NaN.  None otherwise."""
    try:
        if isinstance(score, np.ndarray):
            if score.ndim != 1 or score.dtype.kind not in "fiu":
                return None
            if score.dtype.kind != "f" and score.size and \
                    (int(score.max()) > _FP64_EXACT or int(score.min()) < -_FP64_EXACT):
                return None
            arr = score.astype(np.float64)
        elif isinstance(score, (list, tuple)):
            types = set(map(type, score))
            if not types <= {int, float}:
                return None
            if types == {int}:
                ints = np.array(score, dtype=np.int64)
                if ints.size and (int(ints.max()) > _FP64_EXACT or int(ints.min()) < -_FP64_EXACT):
                    return None
                arr = ints.astype(np.float64)
            else:
                if int in types and not all(-_FP64_EXACT <= v <= _FP64_EXACT for v in score if type(v) is int):
                    return None
                arr = np.array(score, dtype=np.float64)
        else:
            return None
    except OverflowError:
        return None
    return None if np.isnan(arr).any() else arr


def _etk_codes(group):
    """``(codes int32 [n], number of groups)``, groups numbered by first appearance as the loop's
    dict orders them, for a column of only ``int``, only ``str`` or only finite ``float`` values
    (or such an array).  None for nulls, NaN and mixed types, whose dict semantics stay the
    loop's."""
    import pandas as pd

    if isinstance(group, np.ndarray):
        if group.ndim != 1 or group.dtype.kind not in "fiuU":
            return None
        vals = group
    elif isinstance(group, (list, tuple)):
        types = set(map(type, group))
        if len(types) != 1 or not types <= {int, float, str}:
            return None
        t = types.pop()
        try:
            vals = np.array(group, dtype=np.int64 if t is int else np.float64 if t is float else object)
        except OverflowError:
            return None
    else:
        return None
    if vals.dtype.kind == "f":
        if not np.isfinite(vals).all():
            return None
        vals = vals + 0.0                           # -0.0 and 0.0 are one dict key
    codes, uniques = pd.factorize(vals)
    return codes.astype(np.int32), len(uniques)


def _each_top_k_native(kk, group, score, device):
    """``(rows int64 [M], rank int64 [M])`` of ``each_top_k`` from the native engine, or None where
    it declines."""
    from ..models.base import resolve_device
    from ..ops import each_top_k as etk

    if kk is None or kk == 0 or not etk.supports(kk) or os.environ.get("HM_SQL_BATCH_UDTF", "1") == "0":
        return None
    try:
        n = len(group)
        if len(score) != n:
            return None
    except TypeError:
        return None
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    if n > etk.N_MAX:
        return None
    arr = _etk_scores(score)
    gc = _etk_codes(group) if arr is not None else None
    if gc is None:
        return None
    dev = resolve_device(device)
    try:
        from .. import _native

        _native.hip() if dev.type == "cuda" else _native.host()
    except (RuntimeError, OSError):
        return None                                 # no native library: the loop serves
    rows, outptr = etk.segment_topk(torch.from_numpy(arr).to(dev), torch.from_numpy(gc[0]).to(dev), gc[1],
                                    abs(kk), largest=kk > 0)
    rows, outptr = rows.cpu().numpy().astype(np.int64), outptr.cpu().numpy()
    rank = np.arange(1, len(rows) + 1, dtype=np.int64) - np.repeat(outptr[:-1], np.diff(outptr))
    return rows, rank


def each_top_k_batch(k, group, score, device=None):
    """``(rows int64 [M], rank int64 [M])``: the input row and the rank (from 1) of every output
    row of ``each_top_k(k, group, score)``, in its output order, for callers that hold columns
    (lists or NumPy arrays) and gather their own payload.  Runs the native engine on ``device``
    (default: the GPU when there is one) where it applies and the Python loop's ordering
    otherwise; the result is the same."""
    kk = int(k)
    res = _each_top_k_native(kk, group, score, device)
    if res is not None:
        return res
    order = {}
    for i in range(len(group)):
        order.setdefault(group[i], []).append(i)
    rows, rank = [], []
    for idxs in order.values():
        idxs = sorted(idxs, key=lambda i: score[i], reverse=kk > 0)[:abs(kk)]
        rows.extend(idxs)
        rank.extend(range(1, len(idxs) + 1))
    return np.asarray(rows, dtype=np.int64), np.asarray(rank, dtype=np.int64)


@udtf("each_top_k", per_row=False)
def each_top_k(k, group, score, *cols, session=None):
    """Top-|k| rows by ``score`` within each consecutive ``group`` (k < 0: bottom-k).
    Output columns: (rank, key(=score), cols...)."""
    import pandas as pd

    res = _each_top_k_native(_etk_k(k), group, score, _session_device(session))
    if res is None:
        EACH_TOP_K_CALLS["python"] += 1
        return _each_top_k_python(k, group, score, *cols)
    EACH_TOP_K_CALLS["native"] += 1
    idx = res[0].tolist()
    # the loop's own construction (a list of tuples holding the original objects), so the
    # inferred dtypes are the loop's too
    data = [res[1].tolist(), [score[i] for i in idx]] + [[c[i] for i in idx] for c in cols]
    return pd.DataFrame(list(zip(*data)), columns=["rank", "key"] + [f"c{i}" for i in range(len(cols))])


each_top_k.wants_session = True


def topk_similar(X: torch.Tensor, Y: torch.Tensor | None = None, k: int = 10):
    """Batched cosine top-k on the device: (scores, indices) of the k most similar rows of Y
    for every row of X (self-matches excluded when Y is None)."""
    Xn = torch.nn.functional.normalize(X.float(), dim=1)
    Yn = Xn if Y is None else torch.nn.functional.normalize(Y.float(), dim=1)
    if k <= 64 and Xn.shape[1] <= 256:
        # fused MFMA similarity + running top-k (ops/topk_mips.py): no N x N matrix in HBM
        from ..ops.topk_mips import mips_topk

        ix, sc = mips_topk(Xn, Yn, min(k, Yn.shape[0]), exclude_self_offset=0 if Y is None else None)
        return sc, ix
    dt = torch.bfloat16 if X.is_cuda else torch.float32
    S = (Xn.to(dt) @ Yn.to(dt).T).float()
    if Y is None:
        S.fill_diagonal_(-float("inf"))
    return torch.topk(S, min(k, S.shape[1]), dim=1)


def topk_similar_csc(R, k: int, queries=None, device=None):
    """Exact cosine top-k between the columns of a sparse matrix: (scores fp64 [n, k], indices
    int32 [n, k]) of the ``k`` most similar columns for every column in ``queries`` (default:
    all), best first, the column itself excluded, ``0.0`` / ``-1`` where fewer than ``k`` columns
    share a row with it.  Ties go to the smaller column id.

    ``R`` is a ``utils.matrix.CSCMatrix`` or a ``(colptr, rows, vals)`` triple (rows strictly
    increasing inside a column); columns are the vectors, of any height.  Runs
    ``ops.knn_sparse.knn_cols`` on ``device`` (default: the GPU when there is one)."""
    from ..models.base import resolve_device
    from ..ops.knn_sparse import knn_cols
    from ..utils.matrix import CSCMatrix

    n_rows = None
    if isinstance(R, CSCMatrix):
        n_rows = R.n_rows
        R = (R.indptr, R.indices, R.values)
    dev = resolve_device(device)
    try:
        colptr = torch.as_tensor(np.ascontiguousarray(R[0], dtype=np.int64))
        rows = torch.as_tensor(np.ascontiguousarray(R[1], dtype=np.int32))
        vals = torch.as_tensor(np.ascontiguousarray(R[2], dtype=np.float64))
        q = None if queries is None else torch.as_tensor(
            np.ascontiguousarray(queries, dtype=np.int32).reshape(-1)).to(dev)
    except (TypeError, ValueError) as ex:
        raise ValueError(f"topk_similar_csc wants a numeric (colptr, rows, vals) and queries: {ex}") from ex
    idx, score = knn_cols(colptr.to(dev), rows.to(dev), vals.to(dev), k, q, n_rows=n_rows)
    return score, idx


@udtf("cosine_knn", per_row=False, cols=("key", "rank", "other", "similarity"))
def cosine_knn(k, key, feature, value, session=None):
    """cosine_knn(const int k, key, feature, double value) -> table (key, rank, other, similarity):
    for every key, its k most cosine-similar other keys over their sparse (feature, value)
    vectors, rank 1 = best; only keys that share a feature are candidates, ties go to the key
    seen first. Extension (not in upstream Hivemall): item-item similarity + each_top_k in one
    native step (ops/knn_sparse.py)."""
    import pandas as pd

    from ..models.base import resolve_device
    from ..ops.knn_sparse import knn_cols
    from ..utils.options import UDFArgumentException

    kk = k[0] if isinstance(k, (list, tuple, np.ndarray, pd.Series)) and len(k) else k
    try:
        kk = int(kk)
    except (TypeError, ValueError):
        raise UDFArgumentException(f"cosine_knn: k must be a constant int, got {kk!r}") from None
    if not 1 <= kk <= 128:
        raise UDFArgumentException(f"cosine_knn: k must be in 1..128, got {kk}")
    out_cols = ["key", "rank", "other", "similarity"]
    keep = [t for t in zip(key, feature, value) if not any(x is None for x in t)]
    if not keep:
        return pd.DataFrame([], columns=out_cols)
    kc, labels = pd.factorize(np.asarray([t[0] for t in keep], dtype=object))
    fc, feats = pd.factorize(np.asarray([t[1] for t in keep], dtype=object))
    try:
        v = np.asarray([float(t[2]) for t in keep], dtype=np.float64)
    except (TypeError, ValueError) as ex:
        raise UDFArgumentException(f"cosine_knn: value must be numeric: {ex}") from None
    if len(feats) > np.iinfo(np.int32).max or len(labels) > np.iinfo(np.int32).max:
        raise UDFArgumentException("cosine_knn: more than 2^31 - 1 distinct keys or features")
    o = np.lexsort((fc, kc))
    kc, fc, v = kc[o], fc[o], v[o]
    dup = (kc[1:] == kc[:-1]) & (fc[1:] == fc[:-1])
    if dup.any():
        d = int(np.flatnonzero(dup)[0])
        raise UDFArgumentException(f"cosine_knn: duplicate (key, feature) pair "
                                   f"({labels[kc[d]]!r}, {feats[fc[d]]!r})")
    colptr = np.zeros(len(labels) + 1, dtype=np.int64)
    np.cumsum(np.bincount(kc, minlength=len(labels)), out=colptr[1:])
    dev = resolve_device(None if session is None else session.device)
    idx, score = knn_cols(torch.from_numpy(colptr).to(dev), torch.from_numpy(fc.astype(np.int32)).to(dev),
                          torch.from_numpy(v).to(dev), kk, n_rows=len(feats))
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    q, r = np.nonzero(idx >= 0)                      # row-major: keys in order, best first
    return pd.DataFrame({"key": labels[q].tolist(), "rank": (r + 1).tolist(),
                         "other": labels[idx[q, r]].tolist(), "similarity": score[q, r]},
                        columns=out_cols)


cosine_knn.wants_session = True
