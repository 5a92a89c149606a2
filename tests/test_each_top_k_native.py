"""The each_top_k engine (csrc/kernels/each_top_k.hip, csrc/host/each_top_k_cpu.cpp,
ops/each_top_k.py and the routing of ``knn.each_top_k``).

Contract: a group is every row with the same group value; inside a group the rows are ordered by
the pair (score in the chosen direction, input position), ``-0.0`` and ``0.0`` equal, the
infinities ordinary; the first ``min(|k|, group size)`` rows are kept, groups in order of first
appearance.  The pair order is total, so the selected row indices are one integer array and every
comparison here is integer equality.

The oracle is ``np.lexsort((arange(n), -score if largest else score, codes))`` cut at rank
``< k``; ``test_model_is_the_specification`` pins it to the Python loop ``_each_top_k_python``,
which is too slow to be the oracle of the larger cases.

The corpora carry segment lengths one below / at / one above ``WAVE_SEG_MAX`` (one wave per
segment up to it), the default ``chunk`` and ``CHUNK_MIN`` (one work item up to a chunk), lengths
0 and 1, and the kernel's round of 1024 rows several times over inside one work item."""
import decimal
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from hivemall_amd import knn
from hivemall_amd.ops import each_top_k as etk

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
KS = [1, 2, 63, 64, 65, etk.K_MAX]
TIES = np.array([-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0, -0.0, np.inf, -np.inf])


# ------------------------------------------------------------------ the NumPy model
def model_rows(score: np.ndarray, codes: np.ndarray, G: int, k: int, largest: bool):
    """(rows, rank from 1) in output order."""
    n = len(score)
    s = score + 0.0                                             # -0.0 -> 0.0
    order = np.lexsort((np.arange(n), -s if largest else s, codes))
    lens = np.bincount(codes, minlength=G)
    rank = np.arange(n) - (np.cumsum(lens) - lens)[codes[order]]
    keep = rank < k
    return order[keep].astype(np.int32), rank[keep] + 1


def run(device, score, codes, G, k, largest, chunk=None):
    rows, outptr = etk.segment_topk(torch.from_numpy(score).to(device), torch.from_numpy(codes).to(device), G, k,
                                    largest=largest, chunk=chunk)
    assert rows.dtype == torch.int32 and outptr.dtype == torch.int64
    assert rows.device.type == device and outptr.device.type == device
    lens = np.bincount(codes, minlength=G)
    assert outptr.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum(np.minimum(lens, k))]).tolist()
    return rows.cpu().numpy()


def check(device, score, codes, G, k, largest, chunk=None):
    got = run(device, score, codes, G, k, largest, chunk)
    want = model_rows(score, codes, G, k, largest)[0]
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"first difference at output row {int(np.flatnonzero(got != want)[0])}"


def mixed_scores(n: int, seed: int) -> np.ndarray:
    """Half tie-heavy values, half distinct ones."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n) < 0.5, rng.choice(TIES, n), rng.normal(size=n))


def codes_of(lens) -> np.ndarray:
    return np.repeat(np.arange(len(lens), dtype=np.int32), lens)


@functools.lru_cache(maxsize=None)
def corpus(name: str):
    """(score, codes, G, chunk)"""
    W, C, M = etk.WAVE_SEG_MAX, etk.CHUNK_DEFAULT, etk.CHUNK_MIN
    if name == "edges":            # empty segments at both ends and in the middle
        lens = [0, W - 1, W, W + 1, 1, 0, 0, C - 1, C, C + 1, 5, 63, 64, 65, 129, 0]
        chunk = None
    elif name == "min_chunk":
        lens = [0, M - 1, M, M + 1, 1, 300, 2 * M, 2 * M + 1, 0]
        chunk = M
    elif name == "one_group":
        lens = [3000]
        chunk = None
    elif name == "short_and_long":
        rng = np.random.default_rng(5)
        lens = rng.integers(1, 6, 3000).tolist()
        lens[1500] = 20000
        chunk = None
    else:
        raise KeyError(name)
    codes = codes_of(lens)
    return mixed_scores(len(codes), len(name)), codes, len(lens), chunk


# ------------------------------------------------------------------ 1. the oracle itself
@pytest.mark.parametrize("k", [5, -5, 700])
def test_model_is_the_specification(k):
    rng = np.random.default_rng(0)
    n = 20000
    group = rng.integers(0, 37, n)
    score = rng.choice(TIES, n)
    df = knn._each_top_k_python(k, group.tolist(), score.tolist(), list(range(n)))
    codes, uniq = pd.factorize(group)
    rows, rank = model_rows(score, codes.astype(np.int32), len(uniq), abs(k), k > 0)
    assert df["c0"].tolist() == rows.tolist()
    assert df["rank"].tolist() == rank.tolist()


# ------------------------------------------------------------------ 2. engine against model
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["edges", "min_chunk", "one_group", "short_and_long"])
@pytest.mark.parametrize("device", DEVICES)
def test_engine_is_the_model(device, name, k, largest):
    score, codes, G, chunk = corpus(name)
    check(device, score, codes, G, k, largest, chunk)


@pytest.mark.parametrize("device", DEVICES)
def test_no_rows_and_no_groups(device):
    e64, e32 = np.zeros(0, np.float64), np.zeros(0, np.int32)
    assert run(device, e64, e32, 0, 3, True).shape == (0,)
    assert run(device, e64, e32, 4, 3, True).shape == (0,)
    check(device, np.array([1.0, 2.0]), np.array([6, 6], dtype=np.int32), 9, 1, True)


# ------------------------------------------------------------------ 3. adversarial orders
N_ADV = 5000          # one work item at the default chunk, five of its rounds; three items at CHUNK_MIN


def adversarial(kind: str) -> np.ndarray:
    i = np.arange(N_ADV, dtype=np.float64)
    if kind == "equal":
        return np.full(N_ADV, 1.5)
    if kind == "rising":
        return i - 2500.0
    if kind == "falling":
        return 2500.0 - i
    if kind == "two_values":
        return np.where((np.arange(N_ADV) * 7) % 11 < 4, 2.0, -2.0)
    if kind == "zeros":
        return np.where(np.arange(N_ADV) % 2 == 0, -0.0, 0.0)
    if kind == "infinities":
        s = mixed_scores(N_ADV, 9)
        s[::97] = np.inf
        s[5::89] = -np.inf
        return s
    raise KeyError(kind)


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("k", [1, 64, etk.K_MAX])
@pytest.mark.parametrize("kind", ["equal", "rising", "falling", "two_values", "zeros", "infinities"])
@pytest.mark.parametrize("device", DEVICES)
def test_adversarial_orders(device, kind, k, largest):
    score = adversarial(kind)
    codes = np.zeros(N_ADV, dtype=np.int32)
    for chunk in (None, etk.CHUNK_MIN):
        check(device, score, codes, 1, k, largest, chunk)
    if kind in ("equal", "zeros"):                              # the earliest k positions win
        assert run(device, score, codes, 1, k, largest).tolist() == list(range(k))


# ------------------------------------------------------------------ 4. multi-level merge
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("device", DEVICES)
def test_three_levels(device, largest):
    n, k = 70001, etk.K_MAX
    score = mixed_scores(n, 3)
    codes = np.zeros(n, dtype=np.int32)
    small = run(device, score, codes, 1, k, largest, etk.CHUNK_MIN)
    assert etk.STATS["levels"] == 3 and etk.STATS["items"] == 35 + 3 + 1
    default = run(device, score, codes, 1, k, largest)
    want = model_rows(score, codes, 1, k, largest)[0]
    assert np.array_equal(small, want) and np.array_equal(default, want)


# ------------------------------------------------------------------ 5. the sort path
@pytest.mark.parametrize("device", DEVICES)
def test_unclustered_codes_take_the_sort_path(device):
    rng = np.random.default_rng(11)
    n, G = 30000, 40
    lens = rng.multinomial(n - 6000, np.ones(G - 1) / (G - 1)).tolist() + [6000]
    clustered = codes_of(lens)
    score = mixed_scores(n, 12)
    before = dict(etk.STATS)
    check(device, score, clustered, G, 10, True)
    assert etk.STATS["no_perm"] == before["no_perm"] + 1 and etk.STATS["perm"] == before["perm"]
    shuffled = rng.permutation(clustered)
    for k, largest in ((10, True), (etk.K_MAX, False)):
        check(device, score, shuffled, G, k, largest)
    assert etk.STATS["perm"] == before["perm"] + 2 and etk.STATS["no_perm"] == before["no_perm"] + 1


# ------------------------------------------------------------------ 6. routing
def _session(device):
    from hivemall_amd.sql import Session

    return Session(device=device)


class _Route:
    """How the calls were served since the last look."""

    def __init__(self):
        self.look()

    def look(self):
        self.engine, self.served = etk.STATS["calls"], dict(knn.EACH_TOP_K_CALLS)

    def took(self):
        d = (etk.STATS["calls"] - self.engine, knn.EACH_TOP_K_CALLS["native"] - self.served["native"],
             knn.EACH_TOP_K_CALLS["python"] - self.served["python"])
        self.look()
        return d


def _columns(n=4000, seed=2):
    rng = np.random.default_rng(seed)
    return {
        "int_group": rng.integers(-5, 30, n).tolist(),
        "str_group": [f"u{v}" for v in rng.integers(0, 50, n)],
        "float_group": rng.choice([0.0, -0.0, 1.5, -2.25, 1e300], n).tolist(),
        "int_score": rng.integers(-4, 5, n).tolist(),
        "float_score": rng.choice(TIES, n).tolist(),
        "mixed_score": [int(v) if i % 3 else float(v) for i, v in enumerate(rng.integers(-3, 4, n))],
        "str_payload": [f"item{i}" for i in range(n)],
        "none_payload": [None if i % 5 == 0 else f"p{i % 7}" for i in range(n)],
        "int_payload": list(range(n)),
    }


@pytest.mark.parametrize("device", DEVICES)
def test_routed_frames_equal_the_loop(device):
    s = _session(device)
    c = _columns()
    route = _Route()
    for k in (3, -3, [2] * 4000, etk.K_MAX, -1):
        for g in ("int_group", "str_group", "float_group"):
            for sc in ("int_score", "float_score", "mixed_score"):
                cols = (c["str_payload"], c["none_payload"], c["int_payload"], c[sc])
                got = knn.each_top_k(k, c[g], c[sc], *cols, session=s)
                assert route.took() == (1, 1, 0)
                want = knn._each_top_k_python(k, c[g], c[sc], *cols)
                pd.testing.assert_frame_equal(got, want)
    # no payload columns, and no rows
    pd.testing.assert_frame_equal(knn.each_top_k(2, c["int_group"], c["float_score"], session=s),
                                  knn._each_top_k_python(2, c["int_group"], c["float_score"]))
    pd.testing.assert_frame_equal(knn.each_top_k(2, [], [], [], [], session=s),
                                  knn._each_top_k_python(2, [], [], [], []))


@pytest.mark.parametrize("device", DEVICES)
def test_sql_query_runs_the_engine(device, monkeypatch):
    s = _session(device)
    c = _columns(600)
    s.register("t", pd.DataFrame({"g": c["str_group"], "x": c["float_score"], "item": c["str_payload"]}))
    q = "SELECT each_top_k(-4, g, x, g, item) AS (rank, key, g, item) FROM t"
    route = _Route()
    got = s.sql(q)
    assert route.took() == (1, 1, 0)
    want = knn._each_top_k_python(-4, c["str_group"], c["float_score"], c["str_group"], c["str_payload"])
    want.columns = ["rank", "key", "g", "item"]
    assert list(got.columns) == list(want.columns) and got.values.tolist() == want.values.tolist()
    monkeypatch.setenv("HM_SQL_BATCH_UDTF", "0")
    off = s.sql(q)
    assert route.took() == (0, 0, 1)
    pd.testing.assert_frame_equal(off, got)


def _both(k, group, score, *cols, session):
    """The routed call and the loop: equal frames, or the same exception type."""
    try:
        want = knn._each_top_k_python(k, group, score, *cols)
    except Exception as ex:                                    # noqa: BLE001 - whatever the loop raises
        with pytest.raises(type(ex)):
            knn.each_top_k(k, group, score, *cols, session=session)
        return
    pd.testing.assert_frame_equal(knn.each_top_k(k, group, score, *cols, session=session), want)


DECLINED = {
    "k above K_MAX": dict(k=etk.K_MAX + 1),
    "k below -K_MAX": dict(k=-etk.K_MAX - 1),
    "k zero": dict(k=0),
    "k not a number": dict(k="many"),
    "bool score": dict(score=lambda n: [bool(i % 2) for i in range(n)]),
    "None score": dict(score=lambda n: [None if i == 7 else float(i % 5) for i in range(n)]),
    "Decimal score": dict(score=lambda n: [decimal.Decimal(i % 5) for i in range(n)]),
    "str score": dict(score=lambda n: [str(i % 5) for i in range(n)]),
    "NumPy scalar score": dict(score=lambda n: [np.float64(i % 5) for i in range(n)]),
    "int beyond fp64": dict(score=lambda n: [2**53 + 1 if i == 3 else 2**53 for i in range(n)]),
    "huge int": dict(score=lambda n: [10**30 if i == 3 else i for i in range(n)]),
    "NaN score": dict(score=lambda n: [float("nan") if i == 11 else float(i % 5) for i in range(n)]),
    "None group": dict(group=lambda n: [None if i == 2 else i % 4 for i in range(n)]),
    "NaN group": dict(group=lambda n: [float("nan") if i == 2 else float(i % 4) for i in range(n)]),
    "infinite group": dict(group=lambda n: [float("inf") if i == 2 else float(i % 4) for i in range(n)]),
    "mixed group": dict(group=lambda n: [str(i % 4) if i % 2 else i % 4 for i in range(n)]),
    "int and float group": dict(group=lambda n: [float(i % 4) if i % 2 else i % 4 for i in range(n)]),
    "bool group": dict(group=lambda n: [bool(i % 2) for i in range(n)]),
    "short score column": dict(score=lambda n: [1.0] * (n - 1)),
}


@pytest.mark.parametrize("case", list(DECLINED))
def test_declined_inputs_keep_the_loop(case):
    n = 40
    spec = DECLINED[case]
    k = spec.get("k", 3)
    group = spec["group"](n) if "group" in spec else [i % 4 for i in range(n)]
    score = spec["score"](n) if "score" in spec else [float((i * 7) % 5) for i in range(n)]
    route = _Route()
    _both(k, group, score, list(range(n)), session=_session("cpu"))
    engine, native, _ = route.took()
    assert (engine, native) == (0, 0)


def test_declines_without_a_native_library(monkeypatch):
    from hivemall_amd import _native

    def missing():
        raise RuntimeError("no library")

    s = _session("cpu")
    monkeypatch.setattr(_native, "host", missing)
    monkeypatch.setattr(_native, "hip", missing)
    route = _Route()
    _both(2, [1, 1, 2], [0.5, 1.5, 2.5], ["a", "b", "c"], session=s)
    assert route.took() == (0, 0, 1)


@pytest.mark.parametrize("device", DEVICES)
def test_batch_form(device):
    c = _columns(3000, seed=8)
    for group, score in ((c["str_group"], c["float_score"]), (np.asarray(c["int_group"]), np.asarray(c["int_score"]))):
        for k in (4, -4):
            rows, rank = knn.each_top_k_batch(k, group, score, device=device)
            df = knn._each_top_k_python(k, list(group), list(score), list(range(3000)))
            assert rows.tolist() == df["c0"].tolist() and rank.tolist() == df["rank"].tolist()
    # a declined column (a None group) goes through the loop's ordering
    group = [None if i % 9 == 0 else i % 5 for i in range(200)]
    rows, rank = knn.each_top_k_batch(2, group, c["float_score"][:200], device=device)
    df = knn._each_top_k_python(2, group, c["float_score"][:200], list(range(200)))
    assert rows.tolist() == df["c0"].tolist() and rank.tolist() == df["rank"].tolist()


def test_supports():
    assert etk.supports(1) and etk.supports(-etk.K_MAX) and etk.supports(etk.K_MAX)
    assert not etk.supports(0) and not etk.supports(etk.K_MAX + 1) and not etk.supports(None) and not etk.supports(True)


# ------------------------------------------------------------------ 7. argument errors
def _args(n=6):
    return torch.arange(n, dtype=torch.float64), torch.zeros(n, dtype=torch.int32)


def test_argument_errors():
    score, codes = _args()
    with pytest.raises(ValueError, match="score must be torch.float64"):
        etk.segment_topk(score.float(), codes, 1, 2)
    with pytest.raises(ValueError, match="codes must be torch.int32"):
        etk.segment_topk(score, codes.long(), 1, 2)
    with pytest.raises(ValueError, match="dimension"):
        etk.segment_topk(score.reshape(2, 3), codes, 1, 2)
    with pytest.raises(ValueError, match="must be a torch tensor"):
        etk.segment_topk(score.numpy(), codes, 1, 2)
    with pytest.raises(ValueError, match="codes must hold 6"):
        etk.segment_topk(score, codes[:5], 1, 2)
    for k in (0, -1, etk.K_MAX + 1, 2.0, True):
        with pytest.raises(ValueError, match="k must be"):
            etk.segment_topk(score, codes, 1, k)
    for chunk in (0, etk.CHUNK_MIN - 1, etk.CHUNK_MAX + 1):
        with pytest.raises(ValueError, match="chunk must be"):
            etk.segment_topk(score, codes, 1, 2, chunk=chunk)
    bad = score.clone()
    bad[3] = float("nan")
    bad[5] = float("nan")
    with pytest.raises(ValueError, match=r"score\[3\] is NaN"):
        etk.segment_topk(bad, codes, 1, 2)
    for c in (-1, 1):
        off = codes.clone()
        off[4] = c
        with pytest.raises(ValueError, match=r"codes must be in 0\.\.0"):
            etk.segment_topk(score, off, 1, 2)
    with pytest.raises(ValueError, match="n_groups"):
        etk.segment_topk(score, codes, -1, 2)
    # the infinities are values
    inf = torch.tensor([float("inf"), -float("inf"), 0.0])
    rows, _ = etk.segment_topk(inf.double(), torch.zeros(3, dtype=torch.int32), 1, 3)
    assert rows.tolist() == [0, 2, 1]


@pytest.mark.gpu
def test_one_device():
    score, codes = _args()
    with pytest.raises(ValueError, match="codes is on cpu"):
        etk.segment_topk(score.cuda(), codes, 1, 2)
    with pytest.raises(ValueError, match="codes is on cuda"):
        etk.segment_topk(score, codes.cuda(), 1, 2)
