"""The MinHash engine (csrc/kernels/minhash.hip, csrc/host/minhash_cpu.cpp, ops/minhash.py, the
``knn.*_batch`` functions and the SQL hooks of ``minhash`` / ``minhashes`` / ``bbit_minhash``).

Contract: sig[r, h] = unsigned min over the names of row r of MurmurHash3_x86_32(utf8(name),
seed = (seed0 + h) mod 2^32), 0 for an empty row; the name is the text before the first ':'.

Every comparison is exact integer equality: the work is integer only and has no ordering issue.
The oracle is ``utils.hashing.murmur3_batch(names, seed)`` per seed (pinned against the Java
vectors by tests/test_hashing.py), reduced with ``np.minimum.reduceat``, empty rows set to 0.  It
is computed once per seed for the shared corpus and reused by every case; a hash index depends on
``seed0 + h`` alone, so the oracle of ``H`` hashes is a slice of the oracle of 1024.

The corpus carries, besides the edge rows, rows one below / at / one above every tiling constant
of the kernel: ROWS_PER_WG (rows per workgroup, as row counts: ``test_rows_per_workgroup_edges``),
FEATS_PER_PASS (strings per pass), BYTES_STAGED (bytes per pass: as one row of short names and as
one single name) and HASHES_PER_PASS (as H).  MAX_GRID * ROWS_PER_WG rows is the launcher's
largest single sweep (``test_grid_stride``)."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from hivemall_amd import knn
from hivemall_amd.utils.hashing import murmur3_batch, murmurhash3_x86_32_py

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
SEEDS = [0, 0x9747B28C, 0xFFFFFFFE]                 # the last one wraps past 2^32


def _ops():
    from hivemall_amd.ops import minhash

    return minhash


def _tiling():
    m = _ops()
    return m.ROWS_PER_WG, m.FEATS_PER_PASS, m.BYTES_STAGED, m.HASHES_PER_PASS, m.MAX_GRID


def _hashes():
    hpp = _tiling()[3]
    return sorted({1, 2, 10, 63, 64, 65, 128, 200, 1024, hpp - 1, hpp, hpp + 1})


def _name(s: str) -> str:
    p = s.find(":")
    return s if p < 0 else s[:p]


def _row_of_bytes(total: int, tag: str) -> list:
    """A row of distinct 60-byte names (the last one shorter or longer) of ``total`` bytes."""
    out, left, i = [], total, 0
    while left > 0:
        n = 60 if left >= 120 else left
        out.append(f"{tag}{i:05d}".ljust(n, "z")[:n])
        left -= n
        i += 1
    assert sum(len(s) for s in out) == total
    return out


@functools.lru_cache(maxsize=None)
def corpus() -> tuple:
    rpw, fpp, staged, _, _ = _tiling()
    lens = [0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33]
    rows = [
        [],                                                          # first row empty
        ["a"],
        ["a:1", "b:2.5"],
        [f"f{i}" for i in range(63)],
        [f"g{i}:{i}.5" for i in range(64)],
        [f"h{i}" for i in range(65)],
        [],                                                          # two adjacent empty rows
        [],
        [f"n{i:07d}" for i in range(1000)],                          # 9,000 bytes of short names
        ["q" * n + ":1" for n in lens],                              # every tail case, name < string
        ["w" * n for n in lens[1:]],                                 # the same without a value
        ["日本語:1", "特徴量", "😀", "😀😀x:2", "é", "aé😀日"],        # 3-byte CJK, 4-byte emoji
        ["L" * 40000 + ":1", "s"],                                   # longer than any LDS window
        ["dup", "dup", "dup:3", "other", "other:1e-3", "dup"],       # duplicates, name:value
        [":1", ":2.5", "a:7", "a"],                                  # the empty name
        [f"p{i}" for i in range(fpp - 1)],                           # FEATS_PER_PASS - 1 / = / + 1
        [f"p{i}" for i in range(fpp)],
        [f"p{i}" for i in range(fpp + 1)],
        _row_of_bytes(staged - 1, "x"),                              # BYTES_STAGED - 1 / = / + 1
        _row_of_bytes(staged, "y"),
        _row_of_bytes(staged + 1, "z"),
        ["B" * (staged - 1)],                                        # one name around the window
        ["C" * staged, "c"],
        ["D" * (staged + 1) + ":2", "d"],
        ["tail:1"],
        [],                                                          # last row empty
    ]
    assert rpw < len(rows)
    return tuple(tuple(r) for r in rows)


@functools.lru_cache(maxsize=None)
def _corpus_flat():
    rows = corpus()
    names = [_name(s) for r in rows for s in r]
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    return names, lens


_SEED_MIN: dict = {}


def _row_min(names, lens, seed: int) -> np.ndarray:
    """uint32 [n_rows]: the oracle for one seed."""
    out = np.zeros(len(lens), dtype=np.uint32)
    if not names:
        return out
    v = murmur3_batch(names, seed).view(np.uint32)
    starts = np.zeros(len(lens), dtype=np.int64)
    np.cumsum(lens[:-1], out=starts[1:])
    ne = lens > 0
    out[ne] = np.minimum.reduceat(v, starts[ne])
    return out


def oracle(rows, H: int, seed0: int) -> np.ndarray:
    names = [_name(s) for r in rows for s in (r or ())]
    lens = np.array([len(r or ()) for r in rows], dtype=np.int64)
    return np.stack([_row_min(names, lens, (seed0 + h) & 0xFFFFFFFF) for h in range(H)], axis=1) \
        if len(rows) else np.zeros((0, H), np.uint32)


def corpus_oracle(H: int, seed0: int) -> np.ndarray:
    names, lens = _corpus_flat()
    cols = []
    for h in range(H):
        s = (seed0 + h) & 0xFFFFFFFF
        if s not in _SEED_MIN:
            _SEED_MIN[s] = _row_min(names, lens, s)
        cols.append(_SEED_MIN[s])
    return np.stack(cols, axis=1)


@functools.lru_cache(maxsize=None)
def _packed_corpus():
    packed = _ops().pack_feature_column([list(r) for r in corpus()])
    assert packed is not None
    return packed


def _sig(packed, H, seed0, device):
    out = _ops().minhash_signatures(*(t.to(device) for t in packed), H, seed0)
    assert out.dtype == torch.int32 and out.device.type == device
    return out.cpu().numpy().view(np.uint32)


def _sig_rows(rows, H, seed0, device):
    packed = _ops().pack_feature_column([None if r is None else list(r) for r in rows])
    assert packed is not None
    return _sig(packed, H, seed0, device)


# ------------------------------------------------------------------ the oracle's own pin
def test_python_reference_matches_the_oracle():
    names = ["", "a", "ab", "abc", "abcd", "abcde", "日本語", "😀", "x" * 33]
    for seed in (0, 1, 0x9747B28C, 0xFFFFFFFF):
        want = murmur3_batch(names, seed).view(np.uint32)
        got = [murmurhash3_x86_32_py(n.encode("utf-8"), seed) for n in names]
        assert got == want.tolist()


def test_pack_feature_column_layout():
    buf, off, nlen, rowptr = _ops().pack_feature_column([["ab:1", "c"], None, [], [":2", "日:3"]])
    assert (buf.dtype, off.dtype, nlen.dtype, rowptr.dtype) == (torch.uint8, torch.int64, torch.int32,
                                                                torch.int64)
    assert bytes(buf.numpy()) == "ab:1c:2日:3".encode("utf-8")
    assert off.tolist() == [0, 4, 5, 7, 12]
    assert nlen.tolist() == [2, 1, 0, 3]
    assert rowptr.tolist() == [0, 2, 2, 2, 4]


def test_pack_feature_column_arrow_and_refusals():
    import pyarrow as pa

    m = _ops()
    rows = [["ab:1", "c"], None, [], [":2", "日:3"]]
    want = m.pack_feature_column(rows)
    for col in (pa.array(rows, type=pa.list_(pa.string())),
                pa.chunked_array([pa.array(rows[:2], type=pa.list_(pa.string())),
                                  pa.array(rows[2:], type=pa.list_(pa.string()))]),
                pa.array([["zz"]] + rows, type=pa.list_(pa.large_string())).slice(1),
                pd.Series(rows, dtype=object),
                pd.Series(pa.array(rows, type=pa.list_(pa.string())), dtype=pd.ArrowDtype(pa.list_(pa.string())))):
        got = m.pack_feature_column(col)
        assert got is not None
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    assert all(t.numel() == n for t, n in zip(m.pack_feature_column([]), (0, 1, 0, 1)))
    for bad in ([[1, 2, 3]], [{"a": 1.0}], [np.array([0.5, 1.5])], [["a:x"]], [["a:"]], [["a: 1"]],
                [["a:1", None]], [["a", 3]], ["abc"], 7, [["a:inf"]], [["a:1_0"]]):
        assert m.pack_feature_column(bad) is None, bad


# ------------------------------------------------------------------ 1. edge corpus
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("seed0", SEEDS)
@pytest.mark.parametrize("H", [1, 2, 10, 63, 64, 65, 128, 200, 255, 256, 257, 1024])
def test_edge_corpus(device, seed0, H):
    assert H in _hashes() and len(_hashes()) == 12           # HASHES_PER_PASS - 1 / = / + 1 are in
    got = _sig(_packed_corpus(), H, seed0, device)
    want = corpus_oracle(H, seed0)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"first mismatches (row, hash): {bad[:5].tolist()}"
    empty = [i for i, r in enumerate(corpus()) if not r]
    assert (got[empty] == 0).all()


@pytest.mark.parametrize("device", DEVICES)
def test_rows_per_workgroup_edges(device):
    rpw = _tiling()[0]
    rng = np.random.default_rng(5)
    rows = [[f"r{i}_{j}" for j in range(int(rng.integers(0, 6)))] for i in range(2 * rpw + 1)]
    for n in (1, rpw - 1, rpw, rpw + 1, 2 * rpw - 1, 2 * rpw, 2 * rpw + 1):
        got = _sig_rows(rows[:n], 10, 3, device)
        assert np.array_equal(got, oracle(rows[:n], 10, 3)), n


# ------------------------------------------------------------------ 2. grid stride
@pytest.mark.parametrize("device", DEVICES)
def test_grid_stride(device):
    rpw, _, _, _, max_grid = _tiling()
    n = max_grid * rpw + 4464                                # 70,000 with the present constants
    assert n > max_grid * rpw
    rng = np.random.default_rng(11)
    cnt = rng.integers(1, 4, size=n)
    ids = rng.integers(0, 50_000, size=int(cnt.sum()))
    flat = [f"k{v}" for v in ids.tolist()]
    ends = np.cumsum(cnt)
    rows = [flat[e - c:e] for c, e in zip(cnt.tolist(), ends.tolist())]
    got = _sig_rows(rows, 10, 0, device)
    want = np.stack([_row_min(flat, cnt.astype(np.int64), h) for h in range(10)], axis=1)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ 3. invariances
def _random_rows(n, seed):
    rng = np.random.default_rng(seed)
    vocab = [f"v{i}" if i % 3 else f"特{i}:0.{i}" for i in range(5000)]
    return [[vocab[j] for j in rng.integers(0, len(vocab), size=int(rng.integers(0, 61)))]
            for _ in range(n)]


@pytest.mark.parametrize("device", DEVICES)
def test_invariances(device):
    rows = [list(r) for r in corpus()]
    base = _sig(_packed_corpus(), 65, 7, device)
    assert np.array_equal(base, _sig(_packed_corpus(), 65, 7, device))          # a rerun
    rng = np.random.default_rng(3)
    shuffled = [[r[i] for i in rng.permutation(len(r))] for r in rows]
    assert np.array_equal(base, _sig_rows(shuffled, 65, 7, device))             # features shuffled
    perm = rng.permutation(len(rows))
    assert np.array_equal(base[perm], _sig_rows([rows[i] for i in perm], 65, 7, device))
    doubled = [r + r for r in rows]
    assert np.array_equal(base, _sig_rows(doubled, 65, 7, device))              # duplicates
    novalue = [[_name(s) for s in r] for r in rows]
    assert np.array_equal(base, _sig_rows(novalue, 65, 7, device))              # values ignored


@pytest.mark.gpu
def test_cuda_equals_twin_on_random_rows():
    packed = _ops().pack_feature_column(_random_rows(2000, 17))
    for H, seed0 in ((10, 0), (77, 0xFFFFFFF0), (300, 12345)):
        assert np.array_equal(_sig(packed, H, seed0, "cuda"), _sig(packed, H, seed0, "cpu"))


# ------------------------------------------------------------------ 4. today's functions
@functools.lru_cache(maxsize=None)
def _per_row_minhashes(n, k):
    return [knn.minhashes(list(r), False, n, k) for r in corpus()]


@functools.lru_cache(maxsize=None)
def _per_row_bbit(H, b):
    return [knn.bbit_minhash(list(r), H, b) for r in corpus()]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("n,k", [(5, 2), (1, 1), (16, 4)])
def test_minhashes_batch_equals_per_row(device, n, k):
    got = knn.minhashes_batch([list(r) for r in corpus()], n, k, device=device)
    assert got == _per_row_minhashes(n, k)
    assert all(type(v) is int for v in got[1])


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("H,b", [(128, 1), (64, 2), (10, 4)])
def test_bbit_minhash_batch_equals_per_row(device, H, b):
    got = knn.bbit_minhash_batch([list(r) for r in corpus()], H, b, device=device)
    assert got == _per_row_bbit(H, b)


@pytest.mark.parametrize("device", DEVICES)
def test_cluster_ids(device):
    m = _ops()
    sig = m.minhash_signatures(*(t.to(device) for t in _packed_corpus()), 12, 0)
    empty = [i for i, r in enumerate(corpus()) if not r]
    for kg in (1, 2, 3, 4, 12):
        ids = m.cluster_ids(sig, kg)
        assert ids.dtype == torch.int32 and tuple(ids.shape) == (len(corpus()), 12 // kg)
        assert (ids[empty] == 0).all()
        u = sig.cpu().numpy().view(np.uint32).tolist()
        for r in (1, 8, 11):
            want = []
            for g in range(12 // kg):
                h = 0
                for v in u[r][g * kg:(g + 1) * kg]:
                    h = (h * 31 + v) & 0x7FFFFFFF
                want.append(h)
            assert ids[r].tolist() == want
    with pytest.raises(ValueError, match="does not divide"):
        m.cluster_ids(sig, 5)
    s = knn.minhash_signatures([list(r) for r in corpus()], 12, device=device)
    assert torch.equal(s.cpu(), sig.cpu())
    with pytest.raises(ValueError):
        knn.minhash_signatures([[1, 2]], 4, device=device)


def test_bbit_pack_widths():
    m = _ops()
    sig = torch.tensor([[-1, 0x12345678, 5], [0, 0, 0]], dtype=torch.int32)
    for b in (1, 3, 8, 31, 32):
        want = []
        for row in sig.numpy().view(np.uint32).tolist():
            bits = 0
            for i, v in enumerate(row):
                bits |= (v & ((1 << b) - 1)) << (i * b)
            want.append(format(bits, "x"))
        assert m.bbit_pack(sig, b) == want


# ------------------------------------------------------------------ 5. SQL
def _sql_rows():
    rows = [list(r) for r in corpus()]
    keep = [rows[i] for i in (1, 2, 3, 0, 9, 11, 13, 14, 6, 24)]
    return keep + _random_rows(30, 23)


@pytest.fixture
def counted(monkeypatch):
    """Calls of ops.minhash.minhash_signatures."""
    m = _ops()
    calls = []
    real = m.minhash_signatures

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(m, "minhash_signatures", spy)
    return calls


def _session(device, feats, extra=None):
    from hivemall_amd.sql import Session

    s = Session(device=device)
    d = {"id": [f"row{i}" for i in range(len(feats))], "features": feats}
    d.update(extra or {})
    s.register("t", pd.DataFrame(d))
    return s


def _both(monkeypatch, counted, device, feats, query, extra=None):
    """(frame with HM_SQL_BATCH_UDTF=0, frame with the default, engine calls with the default)."""
    monkeypatch.setenv("HM_SQL_BATCH_UDTF", "0")
    per_row = _session(device, feats, extra).sql(query)
    assert not counted, "the batch path ran with HM_SQL_BATCH_UDTF=0"
    monkeypatch.delenv("HM_SQL_BATCH_UDTF")
    batch = _session(device, feats, extra).sql(query)
    return per_row, batch, len(counted)


QUERIES = [
    "SELECT minhash(id, features) AS (clusterid, id) FROM t",
    "SELECT minhash(id, features, '-n 3 -k 4') AS (clusterid, id) FROM t",
    "SELECT t.id, m.clusterid FROM t LATERAL VIEW minhash(id, features) m AS clusterid, item",
    "SELECT id, minhashes(features) AS sig FROM t",
    "SELECT id, minhashes(features, false, 4, 3) AS sig FROM t",
    "SELECT id, bbit_minhash(features) AS sig FROM t",
    "SELECT id, bbit_minhash(features, 16, 2) AS sig FROM t",
]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("query", QUERIES)
def test_sql_batch_equals_per_row(monkeypatch, counted, device, query):
    per_row, batch, calls = _both(monkeypatch, counted, device, _sql_rows(), query)
    assert calls == 1
    assert len(batch) >= len(_sql_rows())
    pd.testing.assert_frame_equal(batch, per_row)


@pytest.mark.parametrize("device", DEVICES)
def test_sql_null_feature_row(monkeypatch, counted, device):
    feats = [["a:1", "b"], None, ["c"]]
    for query, n_null in (("SELECT minhash(id, features) AS (clusterid, id) FROM t", 0),
                          ("SELECT id, minhashes(features) AS sig FROM t", 1),
                          ("SELECT id, bbit_minhash(features) AS sig FROM t", 1)):
        del counted[:]
        per_row, batch, calls = _both(monkeypatch, counted, device, feats, query)
        assert calls == 1
        pd.testing.assert_frame_equal(batch, per_row)
        if n_null:
            assert batch["sig"].isna().tolist() == [False, True, False]
        else:       # a NULL feature array hashes as an empty one: five clusters 0
            assert batch[batch["id"] == "row1"]["clusterid"].tolist() == [0] * 5


FALLBACKS = [
    ("int arrays", [[1, 2, 3], [4, 5]], None, "SELECT minhash(id, features) AS (clusterid, id) FROM t"),
    ("int arrays, udf", [[1, 2, 3], [4, 5]], None, "SELECT id, minhashes(features) AS sig FROM t"),
    ("varying options", [["a", "b:2"], ["c"]], {"opt": ["-n 2 -k 2", "-n 3 -k 1"]},
     "SELECT minhash(id, features, opt) AS (clusterid, id) FROM t"),
    ("varying options, lateral", [["a", "b:2"], ["c"]], {"opt": ["-n 2 -k 2", "-n 3 -k 1"]},
     "SELECT t.id, m.clusterid FROM t LATERAL VIEW minhash(id, features, opt) m AS clusterid, item"),
    ("-n 600 -k 2", [["a", "b:2"], ["c"]], None,
     "SELECT minhash(id, features, '-n 600 -k 2') AS (clusterid, id) FROM t"),
]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("case", FALLBACKS, ids=[c[0] for c in FALLBACKS])
def test_sql_fallbacks(monkeypatch, counted, device, case):
    _, feats, extra, query = case
    per_row, batch, calls = _both(monkeypatch, counted, device, feats, query, extra)
    assert calls == 0
    assert len(batch) > 0
    pd.testing.assert_frame_equal(batch, per_row)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("query", [QUERIES[0], QUERIES[2], QUERIES[3], QUERIES[5]])
def test_sql_unparsable_value_raises_as_per_row(monkeypatch, counted, device, query):
    feats = [["a:1"], ["a:x"]]
    monkeypatch.setenv("HM_SQL_BATCH_UDTF", "0")
    with pytest.raises(Exception) as per_row:
        _session(device, feats).sql(query)
    monkeypatch.delenv("HM_SQL_BATCH_UDTF")
    with pytest.raises(Exception) as batch:
        _session(device, feats).sql(query)
    assert type(batch.value) is type(per_row.value) and issubclass(type(batch.value), ValueError)
    assert not counted


def test_feature_pairs_select_keeps_its_path(monkeypatch):
    from hivemall_amd.ftvec.functions import feature_pairs

    calls = []
    monkeypatch.setattr(feature_pairs, "batch", lambda *a, **kw: calls.append(1))
    assert not getattr(feature_pairs, "batch_select", False)
    out = _session("cpu", [["1:0.5", "2:1.5"], ["3:2.0"]]).sql(
        "SELECT feature_pairs(features) AS (i, j, xi, xj) FROM t")
    assert len(out) == 4 and not calls


@pytest.mark.parametrize("device", DEVICES)
def test_dsl_goes_through_the_engine(counted, device):
    import hivemall_amd.dsl  # noqa: F401

    feats = _sql_rows()[:12] + [None]
    df = pd.DataFrame({"id": list(range(len(feats))), "features": feats})
    got = df.hivemall.on(device).minhashes("features")
    assert got.tolist() == [knn.minhashes(r) for r in feats]           # NULL rows are called too
    got = df.hivemall.on(device).bbit_minhash("features", 32, 2)
    assert got.tolist() == [knn.bbit_minhash(r, 32, 2) for r in feats]
    out = df.hivemall.on(device).minhash("id", "features")
    want = [(c, i) for i, r in zip(df["id"], feats) for c in knn.minhashes(r)]
    assert list(out.columns) == ["clusterid", "item"]
    assert list(zip(out["clusterid"].tolist(), out["item"].tolist())) == want
    assert len(counted) == 3


# ------------------------------------------------------------------ 6. validation
@pytest.mark.parametrize("device", DEVICES)
def test_validation(device):
    m = _ops()
    good = [t.to(device) for t in m.pack_feature_column([["ab:1", "c"], [], ["d"]])]
    buf, off, nlen, rowptr = good
    assert m.minhash_signatures(*good, 4).shape == (3, 4)

    def bad(match, *, buf=buf, off=off, nlen=nlen, rowptr=rowptr, H=4, seed0=0):
        with pytest.raises(ValueError, match=match):
            m.minhash_signatures(buf, off, nlen, rowptr, H, seed0)

    bad("buf must be torch.uint8", buf=buf.to(torch.int8))
    bad("off must be torch.int64", off=off.to(torch.int32))
    bad("nlen must be torch.int32", nlen=nlen.long())
    bad("rowptr must be torch.int64", rowptr=rowptr.to(torch.int32))
    bad("buf must be a torch tensor", buf=buf.cpu().numpy())
    bad("buf must have 1 dimension", buf=buf.reshape(1, -1))
    bad("off must have 1 dimension", off=off.reshape(1, -1))
    bad("nlen must have 1 dimension", nlen=nlen.reshape(1, -1))
    bad("rowptr must have 1 dimension", rowptr=rowptr.reshape(1, -1))
    bad("off must start at 0", off=off + 1)
    bad("rowptr must start at 0", rowptr=rowptr + 1)
    bad("off must be non-decreasing", off=torch.tensor([0, 5, 4, 6], device=device))
    bad("rowptr must be non-decreasing", rowptr=torch.tensor([0, 2, 1, 3], device=device))
    bad("off must hold at least one", off=off[:0])
    bad("rowptr must hold at least one", rowptr=rowptr[:0])
    bad("rowptr must end at nnz", rowptr=torch.tensor([0, 2, 2, 2], device=device))
    bad("rowptr must end at nnz", rowptr=torch.tensor([0, 2, 2, 4], device=device))
    bad("nlen must hold 3 lengths", nlen=nlen[:2])
    bad("off ends at", buf=buf[:-1])
    bad("nlen\\[s\\] must be in", nlen=torch.tensor([5, 1, 1], dtype=torch.int32, device=device))
    bad("nlen\\[s\\] must be in", nlen=torch.tensor([2, -1, 1], dtype=torch.int32, device=device))
    for H in (0, -1, 1025, 2.0, "4", None, True):
        bad("num_hashes must be", H=H)
    for seed0 in (-1, 2**32, 1.5, "0", None, False):
        bad("seed0 must be", seed0=seed0)
    m.minhash_signatures(*good, 1024, 2**32 - 1)
    # check=False skips only the passes over the arrays
    assert torch.equal(m.minhash_signatures(*good, 4, check=False), m.minhash_signatures(*good, 4))
    with pytest.raises(ValueError, match="num_hashes must be"):
        m.minhash_signatures(*good, 0, check=False)
    with pytest.raises(ValueError, match="off must be torch.int64"):
        m.minhash_signatures(buf, off.to(torch.int32), nlen, rowptr, 4, check=False)
    assert m.minhash_signatures(buf[:0], off[:1], nlen[:0], rowptr[:1], 4).shape == (0, 4)


@pytest.mark.gpu
def test_validation_mixed_devices():
    m = _ops()
    good = list(m.pack_feature_column([["ab:1", "c"], [], ["d"]]))
    for i, name in enumerate(("off", "nlen", "rowptr")):
        args = [t.to("cuda") for t in good]
        args[i + 1] = args[i + 1].cpu()
        with pytest.raises(ValueError, match=f"{name} is on cpu"):
            m.minhash_signatures(*args, 4)
