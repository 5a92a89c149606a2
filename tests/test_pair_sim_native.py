"""The pair-similarity engine (csrc/kernels/pair_sim.hip, csrc/host/pair_sim_cpu.cpp,
ops/pair_sim.py and the column forms of the nine similarity / distance UDFs of hivemall_amd.knn).

Contract (docs/compat.md "Pair-similarity engine").

* cosine_similarity, cosine_distance, angular_similarity, angular_distance, jaccard_similarity and
  jaccard_distance equal the per-row functions bit for bit: ``==`` on fp64 bit patterns, no tolerance.
* euclid_distance, manhattan_distance and euclid_similarity sum over ``set(A) | set(B)`` in the
  functions, an order that changes with the process's hash seed.  The engine uses the canonical
  order (A's entries in entry order, then B's entries A does not hold) and is (a) bit for bit equal
  to ``canonical`` below, an oracle of this file in that order, and (b) within a relative
  ``2 n 2^-53`` of the function, ``n = max(1, |A u B|)`` (``(2 n + 2) 2^-53`` for euclid_similarity):
  both are left-to-right sums of n non-negative terms, each within ``(n - 1) 2^-53`` relative of the
  exact sum; ``sqrt`` halves the relative error and adds one rounding.

The corpora carry list lengths at every lanes-per-pair boundary (8, 16, 32, 64) and the first
multi-chunk lengths (65, 129); pair counts that leave tail waves with fewer pairs than slots; a name
pool that gives about half overlap and one that gives near-total overlap; values
``repr(uniform(-3, 3))``, so every product and square is inexact and a fused multiply-add shows."""
import functools
from fractions import Fraction
import math
import os
import random
import subprocess

import numpy as np
import pandas as pd
import pytest
import torch

from hivemall_amd import knn
from hivemall_amd.ops import pair_sim as ps

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
HERE = os.path.dirname(os.path.abspath(__file__))
EXACT = ("cosine_similarity", "cosine_distance", "angular_similarity", "angular_distance", "jaccard_similarity",
         "jaccard_distance")
ORDERED = ("euclid_distance", "manhattan_distance", "euclid_similarity")
FN = {m: getattr(knn, m) for m in EXACT + ORDERED}
LENS = (0, 1, 7, 8, 9, 16, 17, 32, 33, 64, 65, 129)
PAIRS = (1, 7, 9, 63, 65)
EPS = 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _feature_list(rng, length, pool):
    """``length`` distinct names of the first ``max(pool, length * 3 // 2)`` (pool 80: about half to
    two thirds of two lists overlap) or ``max(pool, length)`` (pool 5: near-total overlap)."""
    names = max(pool, length * 3 // 2 if pool > 5 else length)
    return [f"n{i}:{rng.uniform(-3, 3)!r}" for i in rng.sample(range(names), length)]


@functools.lru_cache(maxsize=None)
def corpus(P, L, pool=80, seed=0):
    """``(A, B)``: two columns of ``P`` feature lists with lengths from the boundaries up to ``L``
    (the left side takes them in turn, the right side draws them); pair 0 holds a list of ``L`` on
    each side, so ``L`` is the longest list."""
    rng = random.Random(f"{P}/{L}/{pool}/{seed}")
    lens = [n for n in LENS if n <= L]
    A = [_feature_list(rng, L if p == 0 else lens[(p - 1) % len(lens)], pool) for p in range(P)]
    B = [_feature_list(rng, L if p == 0 else rng.choice(lens), pool) for p in range(P)]
    return A, B


def special():
    """Named pairs ``(a, b)`` of the special cases."""
    rng = random.Random(7)
    x = _feature_list(rng, 33, 80)
    return {
        "disjoint": ([f"a{i}:{rng.uniform(-3, 3)!r}" for i in range(17)], [f"b{i}:{rng.uniform(-3, 3)!r}" for i in range(9)]),
        "identical lists": (x, list(x)),
        "the same list": (x, x),
        "empty, empty": ([], []),
        "empty, some": ([], x),
        "some, empty": (x, []),
        "names without values": (["a", "b", "c:2.5", "d"], ["b", "d:0.3", "e"]),
        "duplicate names": (["a:1.5", "b:0.7", "a:-2.25", "c:0.1", "b:3.3"], ["c:0.2", "a:0.9", "c:-1.1", "d:0.4"]),
        "zeros": (["a:0.0", "b:-0.0", "c:1.5"], ["a:-0.0", "b:0.0", "d:0.0"]),
        "all zero": (["a:0.0", "b:-0.0"], ["a:0.0", "c:-0.0"]),
        "squares underflow": (["a:1e-200", "b:1e-200"], ["a:1e-200", "c:1e-200"]),
        "underflow against plain": (["a:1e-200", "b:1e-200"], ["a:1.5", "b:2.5"]),
        "near overflow": (["a:1e150", "b:-1e150", "c:0.3"], ["a:1e150", "b:1e150", "d:1e150"]),
        "near overflow, opposite": (["a:1e150"], ["a:-1e150"]),
    }


def canonical(a, b):
    """``(SQ, ABS)`` in the engine's order, in Python: A's entries in entry order with ``b = 0.0`` on
    a miss, then B's entries in entry order that A does not hold."""
    A, B = knn._fv(a), knn._fv(b)
    sq = ab = 0.0
    for k, v in A.items():
        d = v - B.get(k, 0.0)
        sq = sq + d * d
        ab = ab + abs(d)
    for k, v in B.items():
        if k not in A:
            sq = sq + v * v
            ab = ab + abs(v)
    return sq, ab


def canonical_measure(measure, a, b):
    sq, ab = canonical(a, b)
    if measure == "manhattan_distance":
        return ab
    d = math.sqrt(sq)
    return d if measure == "euclid_distance" else 1.0 / (1.0 + d)


def bound(measure, a, b):
    n = max(1, len(set(knn._fv(a)) | set(knn._fv(b))))
    return ((2 * n + 2) if measure == "euclid_similarity" else 2 * n) * EPS


@functools.lru_cache(maxsize=None)
def oracle(key, measure):
    """fp64 ``[P]`` from the per-row function (its own process's set order for ``ORDERED``)."""
    A, B = corpus(*key) if isinstance(key, tuple) else map(list, zip(*special().values()))
    out = np.array([FN[measure](a, b) for a, b in zip(A, B)], dtype=np.float64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def encoded(key, device):
    A, B = corpus(*key) if isinstance(key, tuple) else map(list, zip(*special().values()))
    lists, ia, ib = ps.encode_columns(list(A), list(B), torch.device(device))
    return lists, torch.from_numpy(ia).to(device), torch.from_numpy(ib).to(device)


def engine(key, measure, device):
    lists, ia, ib = encoded(key, device)
    before = dict(ps.STATS)
    got = ps.pair_measures(lists, ia, ib, measure)
    path = "hip" if device == "cuda" else "host"
    assert ps.STATS["calls"] == before["calls"] + 1 and ps.STATS[path] == before[path] + 1
    assert got.device.type == device and got.dtype == torch.float64 and got.shape == ia.shape
    return got.cpu().numpy()


def check_against_functions(key, device):
    A, B = corpus(*key) if isinstance(key, tuple) else map(list, zip(*special().values()))
    A, B = list(A), list(B)
    for m in EXACT:
        assert np.array_equal(_bits(engine(key, m, device)), _bits(oracle(key, m))), (key, m)
    for m in ORDERED:
        got = engine(key, m, device)
        want = np.array([canonical_measure(m, a, b) for a, b in zip(A, B)], dtype=np.float64)
        assert np.array_equal(_bits(got), _bits(want)), (key, m)
        fn = oracle(key, m)
        tol = np.array([bound(m, a, b) for a, b in zip(A, B)])
        assert (np.abs(got - fn) <= tol * np.abs(fn)).all(), (key, m)


CORPORA = ([(PAIRS[i % len(PAIRS)], L) for i, L in enumerate(LENS)]
           + [(P, L) for L in (8, 16, 32, 65) for P in PAIRS]
           + [(PAIRS[i % len(PAIRS)], L, 5) for i, L in enumerate(LENS)])


# ------------------------------------------------------------------ 1. the engine is the functions
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("key", CORPORA, ids=lambda v: "-".join(map(str, v)))
def test_engine_equals_the_functions(device, key):
    check_against_functions(key, device)


@pytest.mark.parametrize("device", DEVICES)
def test_special_cases(device):
    check_against_functions("special", device)
    cases = special()
    names = list(cases)
    cos = engine("special", "cosine_similarity", device)
    a, b = cases["identical lists"]
    # bit-equal to the function's value, whatever it is: not to 1.0 by fiat
    assert _bits(cos[names.index("identical lists")]) == _bits(knn.cosine_similarity(a, b))
    assert abs(cos[names.index("identical lists")] - 1.0) < 1e-15
    assert cos[names.index("disjoint")] == 0.0 and cos[names.index("empty, empty")] == 0.0
    assert cos[names.index("squares underflow")] == 0.0            # the na > 0 branch
    assert cos[names.index("all zero")] == 0.0
    jac = engine("special", "jaccard_similarity", device)
    assert jac[names.index("empty, empty")] == 0.0 and jac[names.index("the same list")] == 1.0
    assert jac[names.index("duplicate names")] == 2 / 4            # {a, b, c} and {c, a, d}
    euc = engine("special", "euclid_distance", device)
    assert euc[names.index("near overflow, opposite")] == 2e150


def test_corpora_overlap_and_lengths():
    A, B = corpus(65, 65)
    shared = np.mean([len(set(knn._fv(a)) & set(knn._fv(b))) / max(1, min(len(a), len(b)))
                      for a, b in zip(A, B) if a and b])
    assert 0.3 < shared < 0.8
    A5, B5 = corpus(65, 65, 5)
    shared = np.mean([len(set(knn._fv(a)) & set(knn._fv(b))) / max(1, min(len(a), len(b)))
                      for a, b in zip(A5, B5) if a and b])
    assert shared > 0.9
    assert {len(a) for a in A} >= {0, 1, 65} and len(A[0]) == len(B[0]) == 65
    lists, _, _ = encoded((65, 129), "cpu")
    assert lists.max_len == 129
    # the values make a fused multiply-add visible: the squares are inexact
    v = [float(f.split(":")[1]) for f in A[0]]
    assert sum(Fraction(x) * Fraction(x) != Fraction(x * x) for x in v) > len(v) // 2


@pytest.mark.gpu
def test_kernel_equals_twin():
    keys = CORPORA + ["special"]
    for key in keys:
        gl, gia, gib = encoded(key, "cuda")
        cl, cia, cib = encoded(key, "cpu")
        assert torch.equal(gl.sq.cpu(), cl.sq), key
        pair_gpu = ps.pair_primitives(gl, gia, gib)
        pair_cpu = ps.pair_primitives(cl, cia, cib)
        assert pair_gpu.is_cuda and tuple(pair_gpu.shape) == (4, cia.numel())
        assert np.array_equal(_bits(pair_gpu.cpu().numpy()), _bits(pair_cpu.numpy())), key
        # the cross form: every left list against every right list, equal to the pair form on the
        # expanded index arrays
        N, M = cia.numel(), cib.numel()
        cross_gpu = ps.pair_primitives_cross(gl, gia, gib)
        cross_cpu = ps.pair_primitives_cross(cl, cia, cib)
        assert tuple(cross_gpu.shape) == (4, N, M)
        assert np.array_equal(_bits(cross_gpu.cpu().numpy()), _bits(cross_cpu.numpy())), key
        expanded = ps.pair_primitives(gl, gia.repeat_interleave(M), gib.repeat(N))
        assert torch.equal(expanded.view(torch.int64), cross_gpu.reshape(4, N * M).view(torch.int64)), key


@pytest.mark.parametrize("device", DEVICES)
def test_cross_form_and_masks(device):
    key = (9, 65)
    lists, ia, ib = encoded(key, device)
    N, M = ia.numel(), ib.numel()
    full = ps.pair_primitives(lists, ia.repeat_interleave(M), ib.repeat(N))
    cross = ps.pair_primitives_cross(lists, ia, ib)
    assert torch.equal(cross.reshape(4, -1).view(torch.int64), full.view(torch.int64))
    for mask in (0, 1 << ps.DOT, 1 << ps.SQ, 1 << ps.ABS, 1 << ps.INTER, (1 << ps.DOT) | (1 << ps.ABS)):
        got = ps.pair_primitives_cross(lists, ia, ib, mask)
        for m in range(4):
            want = cross[m] if (mask >> m) & 1 else torch.zeros_like(cross[m])
            assert torch.equal(got[m].view(torch.int64), want.view(torch.int64)), (mask, m)
    A, B = corpus(*key)
    for m in EXACT:
        got = ps.pair_measures_cross(lists, ia, ib, m).cpu().numpy()
        want = [[FN[m](a, b) for b in B] for a in A]
        assert np.array_equal(_bits(got), _bits(want)), m
    got = knn.pairwise_similarity(list(A), list(B), "cosine_similarity", device=device)
    assert got.device.type == device and tuple(got.shape) == (N, M)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits([[knn.cosine_similarity(a, b) for b in B] for a in A]))


# ------------------------------------------------------------------ 2. FeatureLists
@pytest.mark.parametrize("device", DEVICES)
def test_feature_lists(device):
    cases = special()
    rows = [r for pair in cases.values() for r in pair] + [None] + list(corpus(7, 129)[0])
    lists, index = ps.encode_lists(rows, torch.device(device))
    assert lists.ptr.dtype == torch.int64 and lists.ids.dtype == torch.int32 and lists.vals.dtype == torch.float64
    assert lists.sids.dtype == torch.int32 and lists.svals.dtype == torch.float64 and lists.sq.dtype == torch.float64
    assert lists.sq.device.type == device and index.dtype == np.int32 and len(index) == len(rows)
    ptr, ids, vals = lists.ptr.cpu().numpy(), lists.ids.cpu().numpy(), lists.vals.cpu().numpy()
    sids, svals, sq = lists.sids.cpu().numpy(), lists.svals.cpu().numpy(), lists.sq.cpu().numpy()
    assert lists.n_lists < len(rows)                               # identical lists are held once
    for r, row in enumerate(rows):
        l = index[r]
        lo, hi = ptr[l], ptr[l + 1]
        want = knn._fv(row)
        assert [lists.names[i] for i in ids[lo:hi]] == list(want)  # entry order = dict order
        assert np.array_equal(_bits(vals[lo:hi]), _bits(list(want.values())))
        assert len(set(ids[lo:hi].tolist())) == hi - lo            # distinct inside a list
        assert (np.diff(sids[lo:hi]) > 0).all()                    # ascending
        assert dict(zip(sids[lo:hi].tolist(), svals[lo:hi].tolist())) == dict(zip(ids[lo:hi].tolist(), vals[lo:hi].tolist()))
        s = 0.0
        for v in want.values():
            s = s + v * v
        assert _bits(sq[l]) == _bits(s), r
    assert index[rows.index(None)] == index[rows.index([])]        # NULL is the empty list
    assert lists.max_len == 129


def test_a_cross_join_parses_every_list_once(monkeypatch):
    monkeypatch.delenv("HM_SQL_BATCH_UDTF", raising=False)
    rng = random.Random(3)
    f_test = [_feature_list(rng, 9, 80) for _ in range(40)]
    f_train = [_feature_list(rng, 9, 80) for _ in range(50)]
    f_train[7] = list(f_test[3])                                    # equal content, another object
    test = pd.DataFrame({"id": range(40), "features": pd.Series(f_test, dtype=object)})
    train = pd.DataFrame({"id": range(50), "features": pd.Series(f_train, dtype=object)})
    s = _session("cpu")
    s.register("test", test)
    s.register("train", train)
    calls = []
    real = knn._fv
    monkeypatch.setattr(knn, "_fv", lambda x: (calls.append(1), real(x))[1])
    before = knn.PAIR_SIM_CALLS["native"]
    got = s.sql("SELECT t.id AS a, s.id AS b, cosine_similarity(t.features, s.features) AS v "
                "FROM test t CROSS JOIN train s")
    assert knn.PAIR_SIM_CALLS["native"] == before + 1
    assert len(got) == 2000 and 0 < len(calls) <= 90
    monkeypatch.setattr(knn, "_fv", real)
    want = [knn.cosine_similarity(f_test[a], f_train[b]) for a, b in zip(got["a"], got["b"])]
    assert np.array_equal(_bits(got["v"].to_numpy()), _bits(want))


# ------------------------------------------------------------------ 3. the SQL route
def _session(device):
    from hivemall_amd.sql import Session

    return Session(device=device)


def _tables(s, n_test=12, n_train=15, seed=5):
    rng = random.Random(seed)
    lens = (0, 1, 7, 9, 17, 33)
    test = pd.DataFrame({"id": range(n_test),
                         "features": [_feature_list(rng, rng.choice(lens), 80) for _ in range(n_test)]})
    train = pd.DataFrame({"id": range(100, 100 + n_train),
                          "features": [_feature_list(rng, rng.choice(lens), 80) for _ in range(n_train)]})
    s.register("test", test)
    s.register("train", train)
    return test, train


def _same_frames(a, b, measure, sets=None):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for c in a.columns:
        x, y = a[c].to_numpy(), b[c].to_numpy()
        if a[c].dtype.kind != "f" or measure in EXACT:
            assert np.array_equal(_bits(x.astype(float)), _bits(y.astype(float))), (measure, c)
        else:
            assert (np.abs(x - y) <= sets * np.abs(y)).all(), (measure, c)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("measure", EXACT + ORDERED)
def test_sql_cross_join(device, measure, monkeypatch):
    monkeypatch.delenv("HM_SQL_BATCH_UDTF", raising=False)
    s = _session(device)
    test, train = _tables(s)
    feats = {**dict(zip(test["id"], test["features"])), **dict(zip(train["id"], train["features"]))}
    knn_q = (f"SELECT each_top_k(4, t.id, {measure}(t.features, s.features), t.id, s.id) "
             "FROM test t CROSS JOIN train s")
    flat_q = (f"SELECT t.id AS a, s.id AS b, {measure}(t.features, s.features) AS v "
              "FROM test t CROSS JOIN train s")
    const_q = f"SELECT id, {measure}(features, array('n3:0.25', 'n11', 'n40:-1.75', 'zz:2.0')) AS v FROM train"
    before = dict(knn.PAIR_SIM_CALLS)
    got = [s.sql(q) for q in (knn_q, flat_q, const_q)]
    assert knn.PAIR_SIM_CALLS == {"native": before["native"] + 3, "python": before["python"]}
    monkeypatch.setenv("HM_SQL_BATCH_UDTF", "0")
    want = [s.sql(q) for q in (knn_q, flat_q, const_q)]
    assert knn.PAIR_SIM_CALLS["native"] == before["native"] + 3
    const = ["n3:0.25", "n11", "n40:-1.75", "zz:2.0"]
    tol_flat = np.array([bound(measure, feats[a], feats[b]) for a, b in zip(want[1]["a"], want[1]["b"])])
    tol_knn = np.array([bound(measure, feats[a], feats[b]) for a, b in zip(want[0]["c0"], want[0]["c1"])])
    tol_const = np.array([bound(measure, f, const) for f in train["features"]])
    _same_frames(got[0], want[0], measure, tol_knn)
    _same_frames(got[1], want[1], measure, tol_flat)
    _same_frames(got[2], want[2], measure, tol_const)
    assert len(got[0]) == 12 * 4 and len(got[1]) == 12 * 15 and len(got[2]) == 15


@pytest.mark.parametrize("device", DEVICES)
def test_sql_nulls(device, monkeypatch):
    monkeypatch.delenv("HM_SQL_BATCH_UDTF", raising=False)
    rng = random.Random(9)
    a = [_feature_list(rng, 9, 80) for _ in range(10)]
    b = [_feature_list(rng, 7, 80) for _ in range(10)]
    a[2] = a[7] = None
    b[4] = b[7] = None
    s = _session(device)
    s.register("t", pd.DataFrame({"a": pd.Series(a, dtype=object), "b": pd.Series(b, dtype=object)}))
    for m in EXACT + ORDERED:
        q = f"SELECT {m}(a, b) AS v, {m}(a, NULL) AS w FROM t"
        monkeypatch.delenv("HM_SQL_BATCH_UDTF", raising=False)
        before = dict(knn.PAIR_SIM_CALLS)
        got = s.sql(q)
        assert knn.PAIR_SIM_CALLS == {"native": before["native"] + 2, "python": before["python"]}
        for i in range(10):
            if a[i] is None:                                       # a NULL first argument gives NULL
                assert pd.isna(got["v"][i]) and pd.isna(got["w"][i]), (m, i)
            else:
                # a NULL second argument gives the function's value for None
                own = FN[m] if m in EXACT else functools.partial(canonical_measure, m)
                assert _bits(got["v"][i]) == _bits(own(a[i], b[i])), (m, i)
                assert _bits(got["w"][i]) == _bits(own(a[i], None)), (m, i)
        monkeypatch.setenv("HM_SQL_BATCH_UDTF", "0")
        off = s.sql(q)
        assert got["v"].isna().tolist() == off["v"].isna().tolist() == [x is None for x in a]
        for c, other in (("v", b), ("w", [None] * 10)):
            x, y = got[c].to_numpy(dtype=float), off[c].to_numpy(dtype=float)
            if m in EXACT:
                assert np.array_equal(_bits(x), _bits(y)), (m, c)
            else:
                live = [i for i in range(10) if a[i] is not None]
                tol = np.array([bound(m, a[i], other[i]) for i in live])
                assert (np.abs(x[live] - y[live]) <= tol * np.abs(y[live])).all(), (m, c)


# ------------------------------------------------------------------ 4. what the engine declines
def _plain(n=8, seed=13):
    rng = random.Random(seed)
    return ([_feature_list(rng, 5, 80) for _ in range(n)], [_feature_list(rng, 4, 80) for _ in range(n)])


def _patch(col, i, value):
    col = list(col)
    col[i] = value
    return col


def _declined():
    a, b = _plain()
    n = len(a)
    rng = np.random.default_rng(17)
    sig = [rng.integers(0, 3, 4).tolist() for _ in range(2 * n)]
    return {
        "dense float arrays": dict(a=[rng.uniform(-3, 3, 6).tolist() for _ in range(n)],
                                   b=[rng.uniform(-3, 3, 6).tolist() for _ in range(n)]),
        "one dense row": dict(a=_patch(a, 3, [0.5, 1.5]), b=_patch(b, 3, [2.5, -1.0])),
        "int arrays": dict(a=[rng.integers(0, 9, 5).tolist() for _ in range(n)],
                           b=[rng.integers(0, 9, 5).tolist() for _ in range(n)]),
        "jaccard signatures": dict(a=sig[:n], b=sig[n:], args=", 4", only=("jaccard_similarity", "jaccard_distance")),
        "a map": dict(a=_patch(a, 2, {"n1": 0.5, "n2": -1.5})),
        "a map on the right": dict(b=_patch(b, 2, {"n1": 0.5, "n2": -1.5})),
        "a value of inf": dict(a=_patch(a, 1, ["n1:0.5", "n2:inf"])),
        "a value of nan": dict(b=_patch(b, 1, ["n1:0.5", "n2:nan"])),
        "a value beyond the squaring range": dict(a=_patch(a, 1, ["n1:0.5", "n2:1e160"])),
        "an unparsable value": dict(a=_patch(a, 5, ["n1:0.5", "n2:abc"]), raises=True),
        "a scalar row": dict(b=_patch(b, 5, "n1:0.5")),
    }


DECLINED = list(_declined())


def _run(s, q):
    try:
        return s.sql(q), None
    except Exception as ex:                                        # noqa: BLE001 - whatever the loop raises
        return None, ex


def _loop_serves(s, queries, monkeypatch, raises=False):
    """Every query takes the per-row loop (no native call) and gives what it gives with the route
    switched off: the same frame, or the same exception."""
    for q in queries:
        monkeypatch.delenv("HM_SQL_BATCH_UDTF", raising=False)
        before, calls = dict(knn.PAIR_SIM_CALLS), ps.STATS["calls"]
        got, err = _run(s, q)
        assert knn.PAIR_SIM_CALLS["native"] == before["native"] and ps.STATS["calls"] == calls, q
        assert knn.PAIR_SIM_CALLS["python"] > before["python"], q
        monkeypatch.setenv("HM_SQL_BATCH_UDTF", "0")
        want, want_err = _run(s, q)
        assert type(err) is type(want_err), (q, err, want_err)
        if raises:
            assert err is not None and str(err) == str(want_err), (q, err)
        if err is None:
            assert np.array_equal(_bits(got["v"].to_numpy(dtype=float)), _bits(want["v"].to_numpy(dtype=float))), q


@pytest.mark.parametrize("case", DECLINED)
def test_declined_inputs_keep_the_loop(case, monkeypatch):
    spec = _declined()[case]
    a, b = _plain()
    s = _session("cpu")
    s.register("t", pd.DataFrame({"a": pd.Series(spec.get("a", a), dtype=object),
                                  "b": pd.Series(spec.get("b", b), dtype=object)}))
    measures = spec.get("only", EXACT + ORDERED)
    _loop_serves(s, [f"SELECT {m}(a, b{spec.get('args', '')}) AS v FROM t" for m in measures], monkeypatch,
                 spec.get("raises"))


def _plain_session():
    a, b = _plain()
    s = _session("cpu")
    s.register("t", pd.DataFrame({"a": pd.Series(a, dtype=object), "b": pd.Series(b, dtype=object)}))
    return s


def test_declines_without_a_native_library(monkeypatch):
    from hivemall_amd import _native

    def missing():
        raise RuntimeError("no library")

    monkeypatch.setattr(_native, "host", missing)
    monkeypatch.setattr(_native, "hip", missing)
    _loop_serves(_plain_session(), [f"SELECT {m}(a, b) AS v FROM t" for m in EXACT + ORDERED], monkeypatch)


def test_declines_under_a_compensating_sum(monkeypatch):
    from hivemall_amd.evaluation import ranking

    monkeypatch.setattr(ranking, "SUM_IS_SEQUENTIAL", False)
    _loop_serves(_plain_session(), [f"SELECT {m}(a, b) AS v FROM t" for m in EXACT + ORDERED], monkeypatch)
    assert ps.encode_columns(*_plain()) is None


def test_the_plain_frame_is_taken(monkeypatch):
    """The frame the declined cases are patched from does run the engine."""
    monkeypatch.delenv("HM_SQL_BATCH_UDTF", raising=False)
    before = knn.PAIR_SIM_CALLS["native"]
    _plain_session().sql("SELECT cosine_similarity(a, b) AS v, jaccard_similarity(a, b, 4) AS j FROM t")
    assert knn.PAIR_SIM_CALLS["native"] == before + 2


def test_direct_calls_keep_the_loop():
    a, b = _plain()
    before, calls = dict(knn.PAIR_SIM_CALLS), ps.STATS["calls"]
    for m in EXACT + ORDERED:
        assert isinstance(FN[m](a[0], b[0]), float)
    assert knn.PAIR_SIM_CALLS == before and ps.STATS["calls"] == calls


@pytest.mark.parametrize("device", DEVICES)
def test_batch_forms(device):
    a, b = _plain()
    for m in EXACT:
        got = knn.pair_similarity_batch(a, b, m, device=device)
        assert isinstance(got, torch.Tensor) and got.device.type == device
        assert np.array_equal(_bits(got.cpu().numpy()), _bits([FN[m](x, y) for x, y in zip(a, b)]))
        # the query-vector form, either side
        got = knn.pair_similarity_batch(a, b[0], m, device=device)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits([FN[m](x, b[0]) for x in a]))
        got = knn.pair_similarity_batch(a[0], b, m, device=device)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits([FN[m](a[0], y) for y in b]))
    before = dict(knn.PAIR_SIM_CALLS)
    dense = [[0.5, 1.5], [2.5, -1.0]]
    got = knn.pair_similarity_batch(dense, dense[::-1], "euclid_distance", device=device)
    assert got == [knn.euclid_distance(x, y) for x, y in zip(dense, dense[::-1])]       # a list: the loop
    assert knn.PAIR_SIM_CALLS == {"native": before["native"], "python": before["python"] + 1}
    with pytest.raises(ValueError, match="measure must be one of"):
        knn.pair_similarity_batch(a, b, "minkowski_distance", device=device)


# ------------------------------------------------------------------ 5. refusals
def test_argument_errors():
    a, b = _plain()
    lists, ia, ib = ps.encode_columns(a, b)
    ia, ib = torch.from_numpy(ia), torch.from_numpy(ib)
    n = lists.n_lists
    with pytest.raises(ValueError, match="ia must be torch.int32"):
        ps.pair_measures(lists, ia.long(), ib, "cosine_similarity")
    with pytest.raises(ValueError, match="ib must be torch.int32"):
        ps.pair_measures(lists, ia, ib.double(), "cosine_similarity")
    with pytest.raises(ValueError, match="dimension"):
        ps.pair_measures(lists, ia.reshape(2, -1), ib, "cosine_similarity")
    with pytest.raises(ValueError, match="must be a torch tensor"):
        ps.pair_measures(lists, ia.numpy(), ib, "cosine_similarity")
    with pytest.raises(ValueError, match=f"ia must index the {n} lists"):
        ps.pair_measures(lists, _patch_t(ia, 3, n), ib, "cosine_similarity")
    with pytest.raises(ValueError, match=f"ib must index the {n} lists"):
        ps.pair_measures(lists, ia, _patch_t(ib, 0, -1), "cosine_similarity")
    with pytest.raises(ValueError, match=f"b_idx must index the {n} lists"):
        ps.pair_measures_cross(lists, ia, _patch_t(ib, 0, n + 5), "jaccard_similarity")
    with pytest.raises(ValueError, match="ia holds 8 pairs, ib 7"):
        ps.pair_measures(lists, ia, ib[:7].contiguous(), "cosine_similarity")
    with pytest.raises(ValueError, match="measure must be one of"):
        ps.pair_measures(lists, ia, ib, "hamming_distance")
    with pytest.raises(ValueError, match="mask must be"):
        ps.pair_primitives(lists, ia, ib, 16)
    with pytest.raises(ValueError, match="lists must be a FeatureLists"):
        ps.pair_measures((lists.ptr, lists.ids), ia, ib, "cosine_similarity")
    empty = torch.zeros(0, dtype=torch.int32)
    assert ps.pair_measures(lists, empty, empty, "euclid_distance").shape == (0,)
    assert ps.pair_measures_cross(lists, empty, ib, "euclid_distance").shape == (0, 8)
    assert ps.pair_measures_cross(lists, ia, empty, "euclid_distance").shape == (8, 0)


def _patch_t(t, i, v):
    t = t.clone()
    t[i] = v
    return t


@pytest.mark.gpu
def test_one_device():
    a, b = _plain()
    lists, ia, ib = ps.encode_columns(a, b, torch.device("cuda"))
    assert lists.ptr.is_cuda and lists.sq.is_cuda
    with pytest.raises(ValueError, match="ia is on cpu, lists on cuda"):
        ps.pair_measures(lists, torch.from_numpy(ia), torch.from_numpy(ib).cuda(), "cosine_similarity")
    with pytest.raises(ValueError, match="b_idx is on cpu, lists on cuda"):
        ps.pair_measures_cross(lists, torch.from_numpy(ia).cuda(), torch.from_numpy(ib), "cosine_similarity")


# ------------------------------------------------------------------ 6. the twin under sanitizers
def test_twin_standalone_under_sanitizers(tmp_path):
    """tests/native/pair_sim_san.cpp: the twin over an edge corpus (empty lists, lists of 1 and of
    129 entries, index arrays of length 0, the cross form with an empty side, every mask) in a
    program of its own built with -fsanitize=address,undefined; it checks INTER and the walked sums
    against loops of its own.  Host only."""
    exe = tmp_path / "pair_sim_san"
    root = os.path.dirname(HERE)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, "native", "pair_sim_san.cpp"),
                           os.path.join(root, "csrc", "host", "pair_sim_cpu.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pair_sim_san ok" in out.stdout
