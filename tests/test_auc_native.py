"""The AUC engine (csrc/kernels/auc.hip, csrc/host/auc_cpu.cpp, ops/auc.py, evaluation/auc.py and
the (score, label) form of SQL's auc).  Contract: docs/compat.md "AUC engine".

``auc_groups`` is compared with a brute-force integer 2U (a NumPy outer compare), the final values
with ``metrics.auc`` per group; every comparison is ``==`` (nan matches nan), no tolerance.  Group
sizes sit on every boundary between the kernels' size classes."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from hivemall_amd import evaluation
from hivemall_amd.evaluation import metrics as M
from hivemall_amd.ops import auc as A

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
SIZES = (0, 1, 2, 8, 9, A.SMALL_MAX - 1, A.SMALL_MAX, A.SMALL_MAX + 1, A.MEDIUM_MAX, A.MEDIUM_MAX + 1,
         2 * A.TILE + 3)
FAMILIES = ("normal", "five values", "all equal", "specials", "all positive", "all negative")
SPECIALS = np.array([-0.0, 0.0, np.inf, -np.inf, 5e-324, -5e-324, np.nan, 1.5, -1.5])


def _column(rng, family, m):
    """``(scores fp64 [m], labels fp64 [m])`` of one score family."""
    y = (rng.random(m) < 0.4).astype(np.float64)
    if family == "five values":
        s = rng.integers(0, 5, m) / 4.0
    elif family == "all equal":
        s = np.full(m, 0.25)
    elif family == "specials":
        s = rng.choice(SPECIALS, m)
        y[rng.random(m) < 0.1] = np.nan
        y[rng.random(m) < 0.1] = -3.0
    else:
        s = rng.standard_normal(m)
    if family.startswith("all "):
        y[:] = family == "all positive"
    return s, y


def brute(s, y):
    """``(2U, n_pos, n_neg)`` of one group in Python integers."""
    ok = ~np.isnan(s) & ~np.isnan(y)
    p, q = s[ok & (y > 0)], s[ok & ~(y > 0)]
    return int(2 * (p[:, None] > q[None, :]).sum() + (p[:, None] == q[None, :]).sum()), p.size, q.size


@functools.lru_cache(maxsize=None)
def corpus(name):
    """``(scores, labels, rowptr, order or None, expected int64 [3, G])``, read-only."""
    rng = np.random.default_rng(sorted(map(ord, name)))
    if name == "mixed":                            # ~1000 groups of 0..100 rows and two long ones, shuffled
        sizes = rng.integers(0, 101, 1000)
        sizes[[17, 600]] = (3 * A.TILE + 5, A.TILE + A.MEDIUM_MAX // 2)
        cols = [_column(rng, FAMILIES[g % 4] if sizes[g] < 101 else "five values", m) for g, m in enumerate(sizes)]
    else:                                          # one family: every boundary size, each twice
        sizes = np.array(SIZES + SIZES[::-1])
        cols = [_column(rng, name, m) for m in sizes]
    rowptr = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=rowptr[1:])
    want = np.array([brute(s, y) for s, y in cols], dtype=np.int64).T
    s, y = (np.concatenate(c) for c in zip(*cols))
    order = None
    if name == "mixed":
        order = rng.permutation(len(s))
        inv = np.argsort(order)
        s, y = s[inv], y[inv]                      # group rows are s[order[rowptr[g]:rowptr[g + 1]]]
    for a in (s, y, rowptr, want) + (() if order is None else (order,)):
        a.setflags(write=False)
    return s, y, rowptr, order, want


def _tensor(a, device):
    return None if a is None else torch.from_numpy(np.array(a)).to(device)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name", FAMILIES + ("mixed",))
def test_auc_groups_counts_the_pairs(device, name):
    s, y, rowptr, order, want = corpus(name)
    before = dict(A.STATS)
    got = A.auc_groups(*(_tensor(a, device) for a in (s, y, rowptr, order)))
    path = "hip" if device == "cuda" else "host"
    assert A.STATS["calls"] == before["calls"] + 1 and A.STATS[path] == before[path] + 1
    assert all(t.dtype == torch.int64 and t.device.type == device for t in got)
    assert np.array_equal(torch.stack(got).cpu().numpy(), want)
    if name == "all positive":
        assert not want[0].any() and not want[2].any() and want[1].any()
    # integer labels and fp32 scores: the same classes, the widened scores
    s32 = s.astype(np.float32)
    yi = np.where(np.isnan(y), 0, y).astype(np.int32)
    got = A.auc_groups(*(_tensor(a, device) for a in (s32, yi, rowptr, order)))
    lo, hi = rowptr[:-1], rowptr[1:]
    rows = (lambda g: slice(lo[g], hi[g])) if order is None else (lambda g: order[lo[g]:hi[g]])
    want32 = np.array([brute(s32[rows(g)].astype(np.float64), yi[rows(g)].astype(np.float64))
                       for g in range(len(lo))], dtype=np.int64).T
    assert np.array_equal(torch.stack(got).cpu().numpy(), want32)


def test_limits_and_argument_errors():
    s, y = torch.zeros(4, dtype=torch.float64), torch.ones(4)
    rp = torch.tensor([0, 4])
    for bad in ([0, 3], [1, 4], [0, 5, 4]):
        with pytest.raises(ValueError, match="rowptr must rise"):
            A.auc_groups(s, y, torch.tensor(bad))
    with pytest.raises(ValueError, match="scores must be one of"):
        A.auc_groups(s.to(torch.int64), y, rp)
    with pytest.raises(ValueError, match="labels must hold 4 rows"):
        A.auc_groups(s, y[:3], rp)
    with pytest.raises(ValueError, match="rowptr must be torch.int64"):
        A.auc_groups(s, y, rp.int())
    big = torch.zeros(1, dtype=torch.float32).expand(2**26)        # one stored element
    with pytest.raises(ValueError, match="the limit is"):
        A.auc_groups(big, big, torch.tensor([0, 2**26]))
    # an order entry outside the rows is an absent row
    got = A.auc_groups(torch.tensor([0.5, 0.1]), torch.tensor([1, 0]), torch.tensor([0, 4]), torch.tensor([0, 7, -1, 1]))
    assert [int(t) for t in got] == [2, 1, 1]


@pytest.mark.parametrize("device", DEVICES)
def test_auc_batch_equals_metrics_auc(device):
    s, y, rowptr, order, _ = corpus("mixed")
    codes = np.empty(len(s), dtype=np.int32)
    codes[order] = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    s32 = s.astype(np.float32)
    got = evaluation.auc_batch(_tensor(s32, device), _tensor(y, device), _tensor(codes, device))
    assert got.dtype == torch.float64 and got.device.type == device and got.numel() == len(rowptr) - 1
    want = [M.auc(s32[codes == g], y[codes == g]) for g in range(len(rowptr) - 1)]
    assert np.array_equal(got.cpu().numpy(), np.array(want), equal_nan=True)
    assert np.isnan(want).any() and not np.isnan(want).all()
    one = evaluation.auc_batch(s32, y.tolist(), device=device)             # arrays and lists, one group
    assert one.tolist() == [M.auc(s32, y)]


@pytest.mark.parametrize("device", DEVICES)
def test_sql_auc_runs_the_engine(device, monkeypatch):
    from hivemall_amd.sql import Session

    monkeypatch.delenv("HM_SQL_BATCH_UDTF", raising=False)
    rng = np.random.default_rng(3)
    n = 3000
    prob = (rng.integers(0, 50, n) / 50.0).astype(object)
    prob[::97] = None                                                      # a null score: the row is absent
    df = pd.DataFrame({"g": [f"g{v}" for v in rng.integers(0, 9, n) ** 2 % 11], "prob": prob,
                       "label": rng.integers(0, 2, n)})
    df.loc[df["g"] == "g3", "label"] = 1                                   # a group without a negative
    s = Session(device=device)
    s.register("t", df)
    queries = ("SELECT g, auc(prob, label) AS a FROM t GROUP BY g", "SELECT auc(prob, label) AS a FROM t")
    native, engine_calls = M.AUC_CALLS["native"], A.STATS["calls"]
    got = [s.sql(q) for q in queries]
    assert (M.AUC_CALLS["native"], A.STATS["calls"]) == (native + 2, engine_calls + 2)
    monkeypatch.setenv("HM_SQL_BATCH_UDTF", "0")
    for a, q in zip(got, queries):
        b = s.sql(q)
        assert np.array_equal(a["a"].to_numpy(float), b["a"].to_numpy(float), equal_nan=True)
        assert a.drop(columns="a").equals(b.drop(columns="a"))
    assert np.isnan(got[0]["a"].to_numpy(float)).sum() == 1 and 0.3 < got[1]["a"][0] < 0.7
    # a string in the column: the route declines and the loop raises what it always raised
    monkeypatch.delenv("HM_SQL_BATCH_UDTF")
    df["prob"] = df["prob"].where(df.index != 5, "high")
    s.register("t", df)
    for q in queries:
        with pytest.raises(ValueError, match="could not convert string to float"):
            s.sql(q)
    assert M.AUC_CALLS["native"] == native + 2 and A.STATS["calls"] == engine_calls + 2
