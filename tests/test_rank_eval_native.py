"""The ranking-measures engine (csrc/kernels/rank_eval.hip, csrc/host/rank_eval_cpu.cpp,
ops/rank_eval.py, evaluation/ranking.py and the grouped forms of the rank UDAFs).

Contract (docs/compat.md "Ranking-measures engine"): per row, the seven values of
``precision_at_one``, ``recall_at_one``, ``hitrate_one``, ``mrr_one``, ``average_precision_one``,
``ndcg_one`` and ``ranking_auc``, bit for bit.  The oracle is those functions, called row by row;
every comparison is ``==`` on the fp64 bit patterns and there is no tolerance anywhere.

The corpora carry list lengths at every lanes-per-row boundary (8, 16, 32, 64), the first
multi-chunk length (65), 128 / 129 and ``L_MAX``; row counts that leave tail waves with fewer rows
than slots; truth rows of 0, 1, 2, 1000 and 20000 items, unsorted and with duplicates; ids that
include ``-2^63`` and ``2^63 - 1``; duplicated rank items, hit and miss."""
import decimal
import functools
import math
import os
import subprocess

import numpy as np
import pandas as pd
import pytest
import torch

from hivemall_amd import evaluation
from hivemall_amd.evaluation import metrics as M
from hivemall_amd.ops import rank_eval as re

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
HERE = os.path.dirname(os.path.abspath(__file__))
ONE = (M.precision_at_one, M.recall_at_one, M.hitrate_one, M.mrr_one, M.average_precision_one, M.ndcg_one,
       M.ranking_auc)
I64_MIN, I64_MAX = -2**63, 2**63 - 1
# truth ids are even (and I64_MAX), miss ids odd: a rank position hits exactly when it was drawn
# from the row's truth
MISS_POOL = np.array([I64_MIN + 1, -1, 1, 3, I64_MAX - 2], dtype=np.int64)
TRUTH_SIZES = (0, 1, 2, 1000, 5, 17)
# every LPR boundary, the first multi-chunk length, the limit; the row counts leave tail waves
# with fewer rows than slots at every LPR (8, 4, 2 and 1 rows per wave)
L_TO_U = {1: 65, 7: 63, 8: 9, 9: 65, 15: 7, 16: 63, 17: 2, 31: 9, 32: 65, 33: 1, 63: 7, 64: 63, 65: 65,
          128: 9, 129: 63, re.L_MAX: 7}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _tensor(a, device):
    return torch.from_numpy(np.array(a)).to(device)             # a copy: the corpora are read-only


def _ks(L):
    return (None, 0, 1, L - 1, L, L + 1)


def _truth_row(rng, size):
    ids = 2 * rng.choice(np.arange(-40000, 40000, dtype=np.int64), size=size, replace=False)
    if size >= 2:
        ids[0], ids[1] = I64_MIN, I64_MAX
    row = np.concatenate([ids, ids[: max(1, size // 3)]]) if size else ids     # duplicates
    return rng.permutation(row)


@functools.lru_cache(maxsize=None)
def corpus(U, L, p_hit=0.5, ragged=False, graded=False, big=False, seed=0):
    """``(rank int64 [U, L], lengths int32 [U] or None, truth rows, grade rows or None)``."""
    rng = np.random.default_rng([U, L, int(p_hit * 4), ragged, graded, big, seed])
    sizes = [TRUTH_SIZES[(u + seed) % len(TRUTH_SIZES)] for u in range(U)]
    if big:
        sizes[U // 2] = 20000
    if p_hit == 1.0:
        sizes = [max(s, 1) for s in sizes]
    truth = [_truth_row(rng, s) for s in sizes]
    rank = np.empty((U, L), dtype=np.int64)
    for u in range(U):
        hit = (rng.random(L) < p_hit) & (sizes[u] > 0)
        rank[u] = rng.choice(MISS_POOL, L)
        if hit.any():
            rank[u, hit] = rng.choice(rng.choice(truth[u], 6), int(hit.sum()))     # few ids: duplicates
    lengths = None
    if ragged:
        lengths = rng.integers(0, L + 1, U).astype(np.int32)
        lengths[0] = 0
        lengths[-1] = min(1, L)
        if U > 2:
            lengths[1] = L
    grades = None
    if graded:
        grades = [rng.integers(0, 5, len(t)) for t in truth]       # duplicate keys, different grades
        big_row = next(u for u in range(U) if sizes[u] >= 2)
        grades[big_row][-1] = 62
    for a in [rank] + truth + (grades or []):
        a.setflags(write=False)
    return rank, lengths, truth, grades


@functools.lru_cache(maxsize=None)
def oracle(key, k):
    """fp64 ``[7, U]`` from the seven Python functions, row by row."""
    rank, lengths, truth, grades = corpus(*key)
    out = np.empty((7, len(rank)), dtype=np.float64)
    for u in range(len(rank)):
        r = rank[u, : (lengths[u] if lengths is not None else None)].tolist()
        t = truth[u].tolist()
        for m, fn in enumerate(ONE):
            out[m, u] = fn(r, t, k)
        if grades is not None:
            out[re.NDCG, u] = M.ndcg_one(r, list(zip(t, grades[u].tolist())), k)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _index(key, device):
    _, _, truth, grades = corpus(*key)
    rowptr = np.zeros(len(truth) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in truth], out=rowptr[1:])
    cat = lambda rows: _tensor(np.concatenate(rows).astype(np.int64), device)   # noqa: E731
    return re.build_truth(_tensor(rowptr, device), cat(truth), None if grades is None else cat(grades))


def engine(key, k, device, measures=re.ALL, out=None):
    rank, lengths, _, _ = corpus(*key)
    index = _index(key, device)
    before = dict(re.STATS)
    got = re.rank_measures(_tensor(rank, device), index, k,
                           lengths=None if lengths is None else _tensor(lengths, device),
                           measures=measures, out=out)
    path = "hip" if device == "cuda" else "host"
    assert re.STATS["calls"] == before["calls"] + 1 and re.STATS[path] == before[path] + 1
    assert got.device.type == device and got.dtype == torch.float64
    return got.cpu().numpy()


CORPORA = ([(U, L) for L, U in L_TO_U.items()]
           + [(U, L) for L in (8, 16, 32, 65) for U in (1, 2, 7, 9, 63, 65)])
SPECIAL = {
    "all hits": (65, 33, 1.0),
    "no hits": (65, 17, 0.0),
    "all hits, long": (7, 129, 1.0),
    "ragged short": (65, 9, 0.5, True),
    "ragged long": (63, 129, 0.5, True),
    "ragged limit": (9, re.L_MAX, 0.5, True),
    "row of 20000": (9, 64, 0.5, False, False, True),
    "graded": (65, 17, 0.5, False, True),
    "graded ragged long": (9, 129, 0.5, True, True),
    "graded row of 20000": (7, 33, 0.5, False, True, True),
}


# ------------------------------------------------------------------ 1. the engine is the functions
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("U,L", CORPORA, ids=lambda v: str(v))
def test_engine_equals_the_functions(device, U, L):
    for k in _ks(L):
        got = engine((U, L), k, device)
        assert np.array_equal(_bits(got), _bits(oracle((U, L), k))), (U, L, k)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name", list(SPECIAL))
def test_special_corpora(device, name):
    key = SPECIAL[name]
    rank, lengths, truth, _ = corpus(*key)
    L = rank.shape[1]
    for k in _ks(L):
        got = engine(key, k, device)
        want = oracle(key, k)
        assert np.array_equal(_bits(got), _bits(want)), (name, k)
    full = oracle(key, None)
    if name.startswith("all hits"):
        assert (full[re.PRECISION] == 1.0).all() and (full[re.AUC] == 1.0).all()
    if name == "no hits":
        assert not full.any()
    if name.startswith("ragged"):
        assert {0, 1} <= set(lengths.tolist())
    if "20000" in name:
        assert max(len(set(t.tolist())) for t in truth) == 20000


def test_corpora_hit_about_half_and_repeat_items():
    rank, _, truth, _ = corpus(65, 65)
    hit = np.array([[v in set(truth[u].tolist()) for v in rank[u]] for u in range(65) if len(truth[u])])
    assert 0.4 < hit.mean() < 0.6
    assert any(len(set(r.tolist())) < len(r) for r in rank)
    assert rank.min() < 0 and any(I64_MIN in t for t in truth) and any(I64_MAX in t for t in truth)


@pytest.mark.gpu
def test_kernel_equals_twin():
    keys = [(U, L) for U, L in CORPORA] + list(SPECIAL.values())
    for key in keys:
        L = key[1]
        for k in (None, L - 1):
            assert np.array_equal(_bits(engine(key, k, "cuda")), _bits(engine(key, k, "cpu"))), (key, k)
        if len(key) > 4 and key[4]:
            assert torch.equal(_index(key, "cuda").idcg.cpu(), _index(key, "cpu").idcg)


# ------------------------------------------------------------------ 2. truth index, tables, masks
@pytest.mark.parametrize("device", DEVICES)
def test_truth_index(device):
    key = SPECIAL["graded row of 20000"]
    _, _, truth, grades = corpus(*key)
    before = re.STATS["idcg"]
    _index.cache_clear()
    ix = _index(key, device)
    assert re.STATS["idcg"] == before + 1
    assert ix.items.dtype == torch.int64 and ix.gain.dtype == torch.float64 and ix.idcg.dtype == torch.float64
    rowptr, items = ix.rowptr.cpu().numpy(), ix.items.cpu().numpy()
    gain, idcg = ix.gain.cpu().numpy(), ix.idcg.cpu().numpy()
    assert ix.max_len == 20000
    for u, (t, g) in enumerate(zip(truth, grades)):
        rel = dict(zip(t.tolist(), g.tolist()))                    # the last grade of a key wins
        lo, hi = rowptr[u], rowptr[u + 1]
        assert items[lo:hi].tolist() == sorted(rel)
        want_gain = [2 ** float(rel[i]) - 1 for i in sorted(rel)]
        assert np.array_equal(_bits(gain[lo:hi]), _bits(want_gain))
        s, want = 0.0, []
        for i, x in enumerate(sorted(want_gain, reverse=True)):
            s += x / math.log2(i + 2)
            want.append(s)
        assert np.array_equal(_bits(idcg[lo:hi]), _bits(want)), u
    assert 2.0 ** 62 - 1 in gain


def test_tables_are_python_loops():
    log2tab, ideal = re.tables(5000)
    assert len(log2tab) >= 5000 and len(ideal) == len(log2tab)
    assert np.array_equal(_bits(log2tab[:5000]), _bits([math.log2(i + 2) for i in range(5000)]))
    s, want = 0.0, [0.0]
    for i in range(4999):
        s += 1.0 / math.log2(i + 2)
        want.append(s)
    assert np.array_equal(_bits(ideal[:5000]), _bits(want))
    builds = re.STATS["table_builds"]
    assert re.tables(5000)[0] is log2tab and re.STATS["table_builds"] == builds     # cached
    grown = re.tables(len(log2tab) + 1)[0]
    assert len(grown) > len(log2tab) and np.array_equal(_bits(grown[: len(log2tab)]), _bits(log2tab))


@pytest.mark.parametrize("device", DEVICES)
def test_measures_mask(device):
    key = (63, 129)
    full = engine(key, 100, device)
    for mask in (1 << re.NDCG, 1 << re.AP, (1 << re.AUC) | (1 << re.PRECISION), (1 << re.MRR) | (1 << re.RECALL),
                 1 << re.HITRATE):
        fill = torch.full((7, 63), 7.5, dtype=torch.float64, device=device)
        got = engine(key, 100, device, measures=mask, out=fill)
        for m in range(7):
            want = full[m] if (mask >> m) & 1 else np.full(63, 7.5)
            assert np.array_equal(_bits(got[m]), _bits(want)), (mask, m)


# ------------------------------------------------------------------ 3. refusals
def _small():
    rank = torch.tensor([[1, 2, 3], [4, 5, 6]], dtype=torch.int64)
    rowptr = torch.tensor([0, 2, 3], dtype=torch.int64)
    items = torch.tensor([3, 1, 4], dtype=torch.int64)
    return rank, rowptr, items


def test_argument_errors():
    rank, rowptr, items = _small()
    ix = re.build_truth(rowptr, items)
    for k in (-1, 2**31, 2.0, True, "3"):
        with pytest.raises(ValueError, match="k must be"):
            re.rank_measures(rank, ix, k)
    with pytest.raises(ValueError, match="1..1024 positions"):
        re.rank_measures(torch.zeros((2, re.L_MAX + 1), dtype=torch.int64), ix)
    with pytest.raises(ValueError, match="1..1024 positions"):
        re.rank_measures(torch.zeros((2, 0), dtype=torch.int64), ix)
    with pytest.raises(ValueError, match="rank must be torch.int64"):
        re.rank_measures(rank.int(), ix)
    with pytest.raises(ValueError, match="dimension"):
        re.rank_measures(rank.reshape(-1), ix)
    with pytest.raises(ValueError, match="must be a torch tensor"):
        re.rank_measures(rank.numpy(), ix)
    with pytest.raises(ValueError, match="truth must be a TruthIndex"):
        re.rank_measures(rank, (rowptr, items))
    with pytest.raises(ValueError, match="truth holds 2 rows, rank 1"):
        re.rank_measures(rank[:1], ix)
    with pytest.raises(ValueError, match="lengths must be torch.int32"):
        re.rank_measures(rank, ix, lengths=torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="lengths must hold 2"):
        re.rank_measures(rank, ix, lengths=torch.tensor([1], dtype=torch.int32))
    with pytest.raises(ValueError, match="measures must be"):
        re.rank_measures(rank, ix, measures=1 << 7)
    with pytest.raises(ValueError, match="out must be"):
        re.rank_measures(rank, ix, out=torch.zeros((2, 7), dtype=torch.float64))
    with pytest.raises(ValueError, match="rowptr must be torch.int64"):
        re.build_truth(rowptr.int(), items)
    with pytest.raises(ValueError, match="items must be torch.int64"):
        re.build_truth(rowptr, items.double())
    for bad in ([0, 3, 2, 3], [1, 2, 3], [0, 2, 4]):           # not monotone, not from 0, not to nnz
        with pytest.raises(ValueError, match="rowptr must rise"):
            re.build_truth(torch.tensor(bad, dtype=torch.int64), items)
    with pytest.raises(ValueError, match="rel must be torch.int64"):
        re.build_truth(rowptr, items, torch.ones(3))
    for g in (-1, 63):
        with pytest.raises(ValueError, match=r"grades must be in 0\.\.62"):
            re.build_truth(rowptr, items, torch.tensor([0, g, 1], dtype=torch.int64))
    # lengths beyond the list are cut to it, below zero to zero
    got = re.rank_measures(rank, ix, lengths=torch.tensor([99, -5], dtype=torch.int32))
    assert got[re.PRECISION].tolist() == [2 / 3, 0.0]


@pytest.mark.gpu
def test_one_device():
    rank, rowptr, items = _small()
    ix = re.build_truth(rowptr, items)
    with pytest.raises(ValueError, match="truth is on cpu, rank on cuda"):
        re.rank_measures(rank.cuda(), ix)
    with pytest.raises(ValueError, match="lengths is on cpu"):
        re.rank_measures(rank.cuda(), re.build_truth(rowptr.cuda(), items.cuda()),
                         lengths=torch.tensor([1, 2], dtype=torch.int32))
    with pytest.raises(ValueError, match="rowptr is on cpu"):
        re.build_truth(rowptr, items.cuda())


# ------------------------------------------------------------------ 4. the batch form
@pytest.mark.parametrize("device", DEVICES)
def test_batch_form(device):
    key = (65, 17)
    rank, _, truth, _ = corpus(*key)
    rowptr = np.zeros(66, dtype=np.int64)
    np.cumsum([len(t) for t in truth], out=rowptr[1:])
    flat = np.concatenate(truth)
    want = oracle(key, 10)
    for r, t in ((rank, (rowptr, flat)),
                 (_tensor(rank, device), (torch.from_numpy(rowptr), _tensor(flat, "cpu"))),
                 ((np.arange(66) * 17, rank.reshape(-1)), _index(key, device))):
        got = evaluation.ranking_measures_batch(r, t, 10, device=device)
        assert set(got) == set(re.NAMES) | {"mean"}
        for m, name in enumerate(re.NAMES):
            assert got[name].device.type == device and got["mean"][name].device.type == device
            assert np.array_equal(_bits(got[name].cpu().numpy()), _bits(want[m]))
            assert float(got["mean"][name]) == pytest.approx(np.mean(want[m]), rel=1e-14)
    # graded, from a triple
    gkey = SPECIAL["graded"]
    rank, _, truth, grades = corpus(*gkey)
    rowptr = np.zeros(len(truth) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in truth], out=rowptr[1:])
    got = evaluation.ranking_measures_batch(rank, (rowptr, np.concatenate(truth), np.concatenate(grades)),
                                            device=device)
    assert np.array_equal(_bits(got["ndcg"].cpu().numpy()), _bits(oracle(gkey, None)[re.NDCG]))
    with pytest.raises(ValueError, match="rank must be torch.int64"):
        evaluation.ranking_measures_batch(rank.astype(np.float64), (rowptr, np.concatenate(truth)), device=device)


@pytest.mark.gpu
def test_from_recommend_topk():
    """The item tensor of ``recommend_topk`` (``ops.topk_mips.mips_topk``: int64 ``[U, 10]`` on the
    GPU) goes in as it is and every output stays on the device."""
    from hivemall_amd.ops import topk_mips

    g = torch.Generator().manual_seed(3)
    P = torch.randn(300, 16, generator=g).cuda()
    Q = torch.randn(500, 16, generator=g).cuda()
    items, _ = topk_mips.mips_topk(P, Q, 10)
    assert items.is_cuda and items.dtype == torch.int64 and tuple(items.shape) == (300, 10)
    rng = np.random.default_rng(4)
    truth = [rng.integers(0, 500, rng.integers(0, 60)) for _ in range(300)]
    rowptr = np.zeros(301, dtype=np.int64)
    np.cumsum([len(t) for t in truth], out=rowptr[1:])
    ix = re.build_truth(torch.from_numpy(rowptr).cuda(), torch.from_numpy(np.concatenate(truth)).cuda())
    seen = []
    real = re.rank_measures
    try:
        re.rank_measures = lambda rank, *a, **kw: (seen.append(rank), real(rank, *a, **kw))[1]
        got = evaluation.ranking_measures_batch(items, ix, 10)
    finally:
        re.rank_measures = real
    assert seen[0].data_ptr() == items.data_ptr()                  # the tensor itself, no copy
    host = items.cpu().numpy()
    for m, name in enumerate(re.NAMES):
        assert got[name].is_cuda and got["mean"][name].is_cuda
        want = [ONE[m](host[u].tolist(), truth[u].tolist(), 10) for u in range(300)]
        assert np.array_equal(_bits(got[name].cpu().numpy()), _bits(want)), name


# ------------------------------------------------------------------ 5. the SQL route
def _session(device):
    from hivemall_amd.sql import Session

    return Session(device=device)


class _Route:
    """How the calls were served since the last look: (engine calls, native, python)."""

    def __init__(self):
        self.look()

    def look(self):
        self.engine, self.served = re.STATS["calls"], dict(M.RANK_EVAL_CALLS)

    def took(self):
        d = (re.STATS["calls"] - self.engine, M.RANK_EVAL_CALLS["native"] - self.served["native"],
             M.RANK_EVAL_CALLS["python"] - self.served["python"])
        self.look()
        return d


def _frame(n=300, seed=5, L=12):
    rng = np.random.default_rng(seed)
    rec = [rng.integers(-20, 20, rng.integers(0, L + 1)).tolist() for _ in range(n)]
    truth = [rng.integers(-20, 20, rng.integers(0, 9)).tolist() for _ in range(n)]
    return pd.DataFrame({"g": [f"g{v}" for v in rng.integers(0, 7, n)], "rec": rec, "truth": truth,
                         "kk": [10 if i % 2 else 3 for i in range(n)]})


QUERY = ("SELECT g, ndcg(rec, truth, 10) AS a, precision_at(rec, truth) AS b, auc(rec, truth, 5) AS c, "
         "recall_at(rec, truth, 4) AS d, hitrate(rec, truth) AS e, mrr(rec, truth, 0) AS f, "
         "average_precision(rec, truth, 3) AS h FROM t GROUP BY g")


def _same(a: pd.DataFrame, b: pd.DataFrame):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for c in a.columns:
        if c == "g":
            assert a[c].tolist() == b[c].tolist()
        else:
            assert np.array_equal(_bits(a[c].astype(float).to_numpy()), _bits(b[c].astype(float).to_numpy())), c


@pytest.mark.parametrize("device", DEVICES)
def test_sql_query_runs_the_engine(device, monkeypatch):
    monkeypatch.delenv("HM_SQL_BATCH_UDTF", raising=False)
    s = _session(device)
    df = _frame()
    s.register("t", df)
    route = _Route()
    got = s.sql(QUERY)
    assert route.took() == (7, 7, 0)
    # ungrouped: one group
    one = s.sql("SELECT ndcg(rec, truth, 10) AS a, auc(rec, truth) AS c FROM t")
    assert route.took() == (2, 2, 0)
    monkeypatch.setenv("HM_SQL_BATCH_UDTF", "0")
    off = s.sql(QUERY)
    engine_calls, native, python = route.took()
    assert (engine_calls, native) == (0, 0) and python >= 7
    _same(got, off)
    _same(one, s.sql("SELECT ndcg(rec, truth, 10) AS a, auc(rec, truth) AS c FROM t"))
    # and the loop is the functions
    groups = df.groupby("g", sort=False)
    want = {g: float(np.mean([M.ndcg_one(r, t, 10) for r, t in zip(d["rec"], d["truth"])])) for g, d in groups}
    assert np.array_equal(_bits([want[g] for g in got["g"]]), _bits(got["a"].astype(float).to_numpy()))


@pytest.mark.parametrize("device", DEVICES)
def test_sql_graded_ndcg(device, monkeypatch):
    monkeypatch.delenv("HM_SQL_BATCH_UDTF", raising=False)
    s = _session(device)
    df = _frame(120, seed=6)
    rng = np.random.default_rng(7)
    graded = []
    for i, t in enumerate(df["truth"]):
        if i % 3 == 0:
            graded.append(t)                                       # a plain row among graded ones
        elif i % 3 == 1:
            graded.append({int(x): int(r) for x, r in zip(t, rng.integers(0, 5, len(t)))} or {1: 62})
        else:
            graded.append([(int(x), float(r)) for x, r in zip(t, rng.integers(0, 5, len(t)))])
    df["truth"] = graded
    s.register("t", df)
    q = "SELECT g, ndcg(rec, truth, 8) AS a, ndcg(rec, truth) AS b FROM t GROUP BY g"
    route = _Route()
    got = s.sql(q)
    assert route.took() == (2, 2, 0)
    monkeypatch.setenv("HM_SQL_BATCH_UDTF", "0")
    _same(got, s.sql(q))


def _rows(n=24):
    rng = np.random.default_rng(11)
    return ([rng.integers(0, 9, 6).tolist() for _ in range(n)], [rng.integers(0, 9, 3).tolist() for _ in range(n)])


def _patch(col, i, value):
    col = list(col)
    col[i] = value
    return col


def _declined():
    rec, truth = _rows()
    n = len(rec)
    ten = [10] * n
    return {
        "null rank row": dict(rec=_patch(rec, 3, None)),
        "null truth row": dict(truth=_patch(truth, 3, None)),
        "bool ids": dict(rec=_patch(rec, 2, [True, False, 1])),
        "float ids": dict(rec=_patch(rec, 2, [1.0, 2.0, 3.5])),
        "float truth ids": dict(truth=_patch(truth, 2, [1.0, 2.0])),
        "str ids": dict(rec=[[str(v) for v in r] for r in rec], truth=[[str(v) for v in t] for t in truth]),
        "Decimal ids": dict(rec=_patch(rec, 5, [decimal.Decimal(1), decimal.Decimal(2)])),
        "mixed ids": dict(rec=_patch(rec, 5, [1, "1", 2.0])),
        "ids beyond int64": dict(rec=_patch(rec, 5, [2**63, 1])),
        "k not constant": dict(k=[10 if i % 2 else 3 for i in range(n)]),
        "k with a null": dict(k=_patch(ten, 4, None)),
        "k negative": dict(k=[-1] * n),
        "k a float": dict(k=[2.0] * n),
        "list longer than L_MAX": dict(rec=_patch(rec, 1, list(range(re.L_MAX + 1)))),
        "grade above 62": dict(truth=_patch(truth, 1, {1: 63, 2: 1}), fn="ndcg"),
        "grade negative": dict(truth=_patch(truth, 1, [(1, -1), (2, 1)]), fn="ndcg"),
        "grade not an integer": dict(truth=_patch(truth, 1, {1: 1.5}), fn="ndcg"),
        "graded truth, binary measure": dict(truth=_patch(truth, 1, {1: 1}), fn="recall_at"),
        "scalar truth": dict(truth=_patch(truth, 1, 4)),
    }


DECLINED = list(_declined())
FNS = ("precision_at", "recall_at", "hitrate", "mrr", "average_precision", "ndcg", "auc")


def _run(s, q):
    try:
        return s.sql(q), None
    except Exception as ex:                                        # noqa: BLE001 - whatever the loop raises
        return None, ex


@pytest.mark.parametrize("case", DECLINED)
def test_declined_inputs_keep_the_loop(case, monkeypatch):
    monkeypatch.delenv("HM_SQL_BATCH_UDTF", raising=False)
    spec = _declined()[case]
    rec, truth = _rows()
    n = len(rec)
    df = pd.DataFrame({"g": [i % 3 for i in range(n)], "rec": pd.Series(spec.get("rec", rec), dtype=object),
                       "truth": pd.Series(spec.get("truth", truth), dtype=object),
                       "kk": pd.Series(spec.get("k", [4] * n), dtype=object)})
    s = _session("cpu")
    s.register("t", df)
    for fn in ((spec["fn"],) if "fn" in spec else FNS):
        q = f"SELECT g, {fn}(rec, truth, kk) AS v FROM t GROUP BY g"
        monkeypatch.delenv("HM_SQL_BATCH_UDTF", raising=False)
        route = _Route()
        got, err = _run(s, q)
        engine_calls, native, python = route.took()
        assert (engine_calls, native) == (0, 0), (case, fn)
        monkeypatch.setenv("HM_SQL_BATCH_UDTF", "0")
        want, want_err = _run(s, q)
        assert type(err) is type(want_err), (case, fn, err, want_err)
        if err is None:
            assert python >= 1
            _same(got, want)


def test_declines_without_a_native_library(monkeypatch):
    from hivemall_amd import _native

    def missing():
        raise RuntimeError("no library")

    monkeypatch.delenv("HM_SQL_BATCH_UDTF", raising=False)
    s = _session("cpu")
    s.register("t", _frame(40))
    want = s.sql(QUERY)
    monkeypatch.setattr(_native, "host", missing)
    monkeypatch.setattr(_native, "hip", missing)
    route = _Route()
    got = s.sql(QUERY)
    engine_calls, native, python = route.took()
    assert (engine_calls, native) == (0, 0) and python >= 7
    _same(got, want)


def test_direct_calls_keep_the_loop():
    df = _frame(50)
    route = _Route()
    v = M.ndcg(df["rec"].tolist(), df["truth"].tolist(), 10)
    assert route.took() == (0, 0, 1)
    assert v == float(np.mean([M.ndcg_one(r, t, 10) for r, t in zip(df["rec"], df["truth"])]))
    # auc's (score, label) form has no grouped route
    assert M.auc.grouped([pd.Series([0.1, 0.9, 0.4]), pd.Series([0, 1, 0])], np.zeros(3, dtype=np.int64), 1) is None
    assert route.took() == (0, 0, 0)
    # a group without rows is nan, as _mean's
    got = M.hitrate.grouped([pd.Series([[1], [2]], dtype=object), pd.Series([[1], [3]], dtype=object)],
                            np.array([2, 0]), 3)
    assert got[0] == 0.0 and math.isnan(got[1]) and got[2] == 1.0


# ------------------------------------------------------------------ 6. the twin under sanitizers
def test_twin_standalone_under_sanitizers(tmp_path):
    """tests/native/rank_eval_san.cpp: the twin over an edge corpus (empty rows, L = 1 and L_MAX,
    ragged lengths beyond L and below 0, every mask) in a program of its own built with
    -fsanitize=address,undefined; it checks the integer measures against a loop of its own."""
    exe = tmp_path / "rank_eval_san"
    root = os.path.dirname(HERE)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, "native", "rank_eval_san.cpp"),
                           os.path.join(root, "csrc", "host", "rank_eval_cpu.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rank_eval_san ok" in out.stdout
