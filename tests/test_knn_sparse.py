"""The sparse cosine kNN engine (csrc/kernels/knn_sparse.hip, csrc/host/knn_sparse_cpu.cpp,
ops/knn_sparse.py, ``knn.topk_similar_csc``, ``SLIM.fit_csc(knn=K)``, the ``cosine_knn`` table
function) against a dense NumPy ``X.T @ X``.

Contract: candidates of column i are the columns j != i with dot(i, j) != 0; the result is the k
best under "score descending, then column id ascending", padded with -1 / 0.0.

Tolerances.  The shared case holds multiples of 0.5, so every product and partial sum of a dot is
exact in fp64 whatever the order of the additions; what is left of a score is a sqrt, a reciprocal
and two multiplies on each side, under 1e-14 relative, hence rtol 1e-12.  The oracle's smallest
relative gap between adjacent distinct scores is 1.9e-5 (k = 47; 1.0e-4 at k = 10, 1.0e-3 at
k = 1) and the tests assert on the oracle alone that it is above 1e-9 and that every exact tie is
the identical pair {4, 7}, so rtol 1e-12 cannot hide a wrong neighbour and index equality is
well defined.  For standard-normal values (test 4) reassociating at most 300 products costs at
most 300 * 2^-53 * |x_i| * |x_j|, times the norms at most 3.4e-14 on a score in [-1, 1]: atol
1e-12."""
import numpy as np
import pandas as pd
import pytest
import torch

from hivemall_amd.models.recommend import SLIM
from hivemall_amd.utils.matrix import CSCMatrix
from hivemall_amd.utils.options import UDFArgumentException

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
RTOL = 1e-12
ATOL = 1e-12


def _ops():
    from hivemall_amd.ops import knn_sparse

    return knn_sparse


def _half_steps(rng, shape):
    return rng.integers(1, 11, size=shape) * 0.5            # 0.5, 1.0, ..., 5.0


def _csc(X, device="cpu"):
    """Dense [users, C] -> (colptr, rows, vals) tensors; zeros are absent."""
    cols = [np.nonzero(X[:, c])[0] for c in range(X.shape[1])]
    colptr = np.zeros(X.shape[1] + 1, dtype=np.int64)
    np.cumsum([len(r) for r in cols], out=colptr[1:])
    rows = np.concatenate(cols).astype(np.int32)
    vals = np.concatenate([X[r, c] for c, r in enumerate(cols)]).astype(np.float64)
    return tuple(torch.from_numpy(a).to(device) for a in (colptr, rows, vals))


def _oracle(X, queries=None):
    """Per query: the full candidate list [(j, score)] in the contract's order, from dense
    products (``X.T @ X[:, queries]``: no C x C matrix when queries are given)."""
    C = X.shape[1]
    q = np.arange(C) if queries is None else np.asarray(queries)
    D = X.T @ X[:, q]                                        # [C, n]
    sq = (X * X).sum(0)
    rn = np.zeros(C)
    rn[sq > 0] = 1.0 / np.sqrt(sq[sq > 0])
    out = []
    for t, i in enumerate(q):
        d = D[:, t]
        cand = [j for j in np.flatnonzero(d) if j != i]
        s = {j: (d[j] * rn[i]) * rn[j] for j in cand}
        cand.sort(key=lambda j: (-s[j], j))
        out.append([(int(j), float(s[j])) for j in cand])
    return out


def _expect(full, k):
    idx = np.full((len(full), k), -1, dtype=np.int32)
    score = np.zeros((len(full), k))
    for t, cand in enumerate(full):
        for r, (j, s) in enumerate(cand[:k]):
            idx[t, r], score[t, r] = j, s
    return idx, score


_CASE: dict = {}


def _shared_case():
    """400 users, 48 columns of half-star values.  Columns 0..5 hold 0, 1, 63, 64, 65 and 300
    entries (around the wave width), the others 2..119; column 7 is identical to column 4;
    columns 8 (users 0..99) and 9 (users 200..279) have no common user.  Built once, with its
    oracle, and shared read-only."""
    if not _CASE:
        users, C = 400, 48
        rng = np.random.default_rng(11)
        lens = [0, 1, 63, 64, 65, 300]
        X = np.zeros((users, C))
        for c in range(C):
            m = lens[c] if c < len(lens) else int(rng.integers(2, 120))
            X[rng.choice(users, size=m, replace=False), c] = _half_steps(rng, m)
        X[:, 7] = X[:, 4]
        X[:, 8] = 0
        X[: users // 4, 8] = _half_steps(rng, users // 4)
        X[:, 9] = 0
        X[users // 2: users // 2 + users // 5, 9] = _half_steps(rng, users // 5)
        X.setflags(write=False)
        _CASE["X"] = X
        _CASE["full"] = _oracle(X)
    return _CASE["X"], _CASE["full"]


def _assert_oracle_is_decisive(full, k):
    """On the oracle alone: among each query's top-(k+1), adjacent distinct scores differ by more
    than 1e-9 relative, and every exact tie is the pair {4, 7}."""
    for cand in full:
        top = cand[:k + 1]
        for (a, sa), (b, sb) in zip(top[:-1], top[1:]):
            if sa == sb:
                assert {a, b} == {4, 7}, (a, b)
            else:
                assert (sa - sb) / abs(sa) > 1e-9, (a, b, sa, sb)


def _run(X, k, device, query=None, **kw):
    q = None if query is None else torch.as_tensor(np.asarray(query, dtype=np.int32)).to(device)
    idx, score = _ops().knn_cols(*_csc(X, device), k, q, n_rows=X.shape[0], **kw)
    n = X.shape[1] if query is None else len(query)
    assert idx.dtype == torch.int32 and score.dtype == torch.float64
    assert idx.device.type == device and tuple(idx.shape) == tuple(score.shape) == (n, k)
    return idx.cpu().numpy(), score.cpu().numpy()


# ---------------------------------------------------------------------------------- 1. oracle
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("k", [1, 10, 47])
def test_equals_dense_oracle(k, device):
    X, full = _shared_case()
    lens = (X != 0).sum(0)
    assert lens[:6].tolist() == [0, 1, 63, 64, 65, 300]
    assert not (X[:, 8] * X[:, 9]).any() and lens[8] and lens[9]
    _assert_oracle_is_decisive(full, k)
    idx, score = _run(X, k, device)
    ei, es = _expect(full, k)
    np.testing.assert_array_equal(idx, ei)
    np.testing.assert_allclose(score, es, rtol=RTOL, atol=0.0)
    assert (idx[0] == -1).all() and (score[0] == 0).all()               # empty column
    short = [t for t, c in enumerate(full) if len(c) < k]
    if k == 47:
        assert short                                                      # padding is exercised
    for t in short:
        assert (idx[t, len(full[t]):] == -1).all() and (score[t, len(full[t]):] == 0).all()
    assert not (idx == np.arange(X.shape[1])[:, None]).any()            # never itself
    assert 9 not in idx[8] and 8 not in idx[9]
    assert idx[4, 0] == 7 and idx[7, 0] == 4
    np.testing.assert_allclose(score[[4, 7], 0], 1.0, rtol=RTOL)
    both = 0
    for t in range(X.shape[1]):
        p4, p7 = np.flatnonzero(idx[t] == 4), np.flatnonzero(idx[t] == 7)
        if len(p4) and len(p7):
            both += 1
            assert p4[0] + 1 == p7[0] and score[t, p4[0]] == score[t, p7[0]]
    assert both or k == 1


# ------------------------------------------------------------------------- 2. tile invariance
@pytest.mark.parametrize("device", DEVICES)
def test_tile_size_does_not_change_the_result(device):
    X, full = _shared_case()
    ref_i, ref_s = _run(X, 10, device)
    np.testing.assert_array_equal(ref_i, _expect(full, 10)[0])
    for tile in (16, 17, 48):                                # 3, 3 and 1 passes over 48 columns
        idx, score = _run(X, 10, device, tile=tile)
        np.testing.assert_array_equal(idx, ref_i)
        np.testing.assert_array_equal(score, ref_s)


def _boundary_case():
    """C = 16384 + 70 columns of 1-3 half-star entries over 256 users.  The 105 columns from
    16384 - 35 on draw their users from the last 32 users, which no other column uses, so their
    neighbours lie among themselves: on both sides of column 16384, the edge of a full tile.
    64 queries: 60 of those columns and 4 from the front."""
    if "bX" not in _CASE:
        users, C, edge = 256, 16384 + 70, 16384 - 35
        rng = np.random.default_rng(12)
        X = np.zeros((users, C))
        m = rng.integers(1, 4, size=C)
        for e in range(3):
            sel = np.flatnonzero(m > e)
            u = np.where(sel < edge, rng.integers(0, 224, size=len(sel)), rng.integers(224, 256, size=len(sel)))
            X[u, sel] = _half_steps(rng, len(sel))
        q = np.concatenate([rng.permutation(np.arange(edge, C))[:60], [0, 1, 2, 3]])
        _CASE["bX"], _CASE["bq"] = X, rng.permutation(q)
        _CASE["bfull"] = _oracle(X, _CASE["bq"])
    return _CASE["bX"], _CASE["bq"], _CASE["bfull"]


@pytest.mark.parametrize("device", DEVICES)
def test_neighbours_on_both_sides_of_the_tile_boundary(device):
    X, q, full = _boundary_case()
    k = 20
    assert len(q) == 64
    # some queries' top-k holds columns below and columns at or above 16384: the running list
    # of the first tile is merged with the second tile's candidates
    straddle = [t for t, c in enumerate(full)
                if any(j < 16384 for j, _ in c[:k]) and any(j >= 16384 for j, _ in c[:k])]
    assert len(straddle) >= 5
    idx, score = _run(X, k, device, query=q)
    # values are multiples of 0.5 and a column has at most 3 entries: many exact ties, all of
    # them decided by the column id, in the oracle as in the engine
    ei, es = _expect(full, k)
    np.testing.assert_allclose(score, es, rtol=RTOL, atol=0.0)
    for t in range(len(q)):
        for r in range(k):
            if idx[t, r] != ei[t, r]:
                # the two sides may differ only where rounding of the norms splits or joins an
                # exact tie: the scores agree to rtol and the column is the oracle's candidate
                assert idx[t, r] >= 0 and ei[t, r] >= 0
                s = dict(full[t])
                np.testing.assert_allclose(score[t, r], s[int(idx[t, r])], rtol=RTOL, atol=0.0)
    i16, s16 = _run(X, k, device, query=q, tile=5000)       # 4 passes
    np.testing.assert_array_equal(i16, idx)
    np.testing.assert_array_equal(s16, score)


# --------------------------------------------------------------------------------- 3. queries
@pytest.mark.parametrize("device", DEVICES)
def test_query_subset_keeps_the_callers_order_and_pads(device):
    X, full = _shared_case()
    q = [5, 40, 0, 7, 5, 1, 23]                              # shuffled, 5 twice, the empty column
    idx, score = _run(X, 47, device, query=q)
    ei, es = _expect([full[i] for i in q], 47)
    np.testing.assert_array_equal(idx, ei)
    np.testing.assert_allclose(score, es, rtol=RTOL, atol=0.0)
    np.testing.assert_array_equal(idx[0], idx[4])
    n1 = len(full[1])                                        # column 1: one entry, few candidates
    assert 0 < n1 < 47 and (idx[5, :n1] >= 0).all() and (idx[5, n1:] == -1).all()
    assert (score[5, n1:] == 0).all()
    e_i, e_s = _run(X, 3, device, query=[])
    assert e_i.shape == (0, 3) and e_s.shape == (0, 3)


# -------------------------------------------------------------------------- 4. inexact values
@pytest.mark.parametrize("device", DEVICES)
def test_inexact_values_meet_the_order_free_contract(device):
    rng = np.random.default_rng(13)
    users, C, k = 400, 60, 10
    X = np.zeros((users, C))
    for c in range(C):
        m = 300 if c == 0 else int(rng.integers(1, 120))
        X[rng.choice(users, size=m, replace=False), c] = rng.standard_normal(m)
    assert (X < 0).any() and (X != 0).sum(0).max() == 300
    full = _oracle(X)
    idx, score = _run(X, k, device, tile=32)
    some_negative = False
    for t in range(C):
        s = dict(full[t])
        got = [(int(j), float(v)) for j, v in zip(idx[t], score[t]) if j >= 0]
        assert len(got) == min(k, len(s)) and len({j for j, _ in got}) == len(got)
        assert all(j != t and j in s for j, _ in got)
        vals = [v for _, v in got]
        assert all(a >= b for a, b in zip(vals[:-1], vals[1:]))
        for j, v in got:
            assert abs(v - s[j]) <= ATOL
        some_negative |= any(v < 0 for v in vals)
        if len(got) == k:
            taken = {j for j, _ in got}
            left = [v for j, v in s.items() if j not in taken]
            assert not left or max(left) <= vals[-1] + ATOL
        assert (idx[t, len(got):] == -1).all() and (score[t, len(got):] == 0).all()
    assert some_negative


# ---------------------------------------------------------------------------------- 5. reruns
@pytest.mark.parametrize("device", DEVICES)
def test_reruns_are_bit_identical_and_match_the_cpu_twin(device):
    X, _ = _shared_case()
    a_i, a_s = _run(X, 10, device)
    b_i, b_s = _run(X, 10, device)
    np.testing.assert_array_equal(a_i, b_i)
    np.testing.assert_array_equal(a_s, b_s)
    c_i, c_s = _run(X, 10, "cpu")
    np.testing.assert_array_equal(a_i, c_i)
    np.testing.assert_allclose(a_s, c_s, rtol=RTOL, atol=0.0)


def test_transpose_and_norms():
    X, _ = _shared_case()
    K = _ops()
    colptr, rows, vals = _csc(X)
    rowptr, cols, rvals = K.csc_transpose(colptr, rows, vals, X.shape[0])
    r, c = np.nonzero(X)                                     # row-major: columns ascending in a row
    np.testing.assert_array_equal(cols.numpy(), c)
    np.testing.assert_array_equal(rvals.numpy(), X[r, c])
    np.testing.assert_array_equal(np.diff(rowptr.numpy()), (X != 0).sum(1))
    rn = K.col_rnorm(colptr, vals).numpy()
    assert rn[0] == 0 and rn[4] == rn[7]
    np.testing.assert_allclose(rn[1:], 1 / np.sqrt((X * X).sum(0)[1:]), rtol=RTOL)


# ------------------------------------------------------------------------------ 6. validation
@pytest.mark.parametrize("device", DEVICES)
def test_rejects_bad_arguments(device):
    K = _ops()
    X, _ = _shared_case()
    colptr, rows, vals = _csc(X, device)
    q = torch.tensor([1, 2], dtype=torch.int32, device=device)
    for bad in ((colptr.int(), rows, vals), (colptr, rows.long(), vals), (colptr, rows, vals.float()),
                (colptr.numpy(force=True), rows, vals), (colptr[None], rows, vals), (colptr, rows, vals[:-1])):
        with pytest.raises(ValueError):
            K.knn_cols(*bad, 3)
    s = int(colptr[3])
    swapped = rows.clone()
    swapped[s], swapped[s + 1] = rows[s + 1], rows[s]
    with pytest.raises(ValueError, match="increasing"):
        K.knn_cols(colptr, swapped, vals, 3)
    with pytest.raises(ValueError, match="n_rows"):
        K.knn_cols(colptr, rows, vals, 3, n_rows=int(rows.max()))          # one id too large
    neg = rows.clone()
    neg[int(colptr[1])] = -1                                                # column 1's only entry
    with pytest.raises(ValueError, match="rows"):
        K.knn_cols(colptr, neg, vals, 3, n_rows=400)
    for k in (0, 129, -1, 2.5, None):
        with pytest.raises(ValueError, match="k must"):
            K.knn_cols(colptr, rows, vals, k)
    for tile in (0, 16385, -4, 1.5):
        with pytest.raises(ValueError, match="tile must"):
            K.knn_cols(colptr, rows, vals, 3, tile=tile)
    for bad_q in (q.long(), q[None], q.tolist()):
        with pytest.raises(ValueError, match="query"):
            K.knn_cols(colptr, rows, vals, 3, bad_q)
    for ids in ([0, 48], [-1, 3]):
        with pytest.raises(ValueError, match="query column ids"):
            K.knn_cols(colptr, rows, vals, 3, torch.tensor(ids, dtype=torch.int32, device=device))
    idx, _ = K.knn_cols(colptr, rows, vals, 128, q, tile=16384)             # the limits are allowed
    assert tuple(idx.shape) == (2, 128)


@pytest.mark.gpu
def test_rejects_a_mix_of_devices():
    K = _ops()
    X, _ = _shared_case()
    colptr, rows, vals = _csc(X, "cuda")
    q = torch.tensor([1, 2], dtype=torch.int32)
    with pytest.raises(ValueError, match="rows is on"):
        K.knn_cols(colptr, rows.cpu(), vals, 3)
    with pytest.raises(ValueError, match="vals is on"):
        K.knn_cols(colptr, rows, vals.cpu(), 3)
    with pytest.raises(ValueError, match="query is on"):
        K.knn_cols(colptr, rows, vals, 3, q)
    with pytest.raises(ValueError, match="query is on"):
        K.knn_cols(colptr.cpu(), rows.cpu(), vals.cpu(), 3, q.cuda())


# ----------------------------------------------------------------------------- 7. fit_csc(knn)
def _ratings(seed, n_users, n_items, density):
    rng = np.random.default_rng(seed)
    return _half_steps(rng, (n_users, n_items)) * (rng.random((n_users, n_items)) < density)


@pytest.mark.parametrize("device", DEVICES)
def test_fit_csc_computes_its_neighbours(device):
    Rm = _ratings(51, 80, 30, 0.15)
    full = _oracle(Rm)
    _assert_oracle_is_decisive_or_tied_by_id(full, 5)
    targets = [3, 0, 17, 29, 8, 11]
    nbr = [[j for j, _ in full[i][:5]] for i in targets]
    assert all(len(n) == 5 for n in nbr)
    colptr, rows, vals = (t.numpy() for t in _csc(Rm))
    R = CSCMatrix(colptr, rows, vals, Rm.shape[0])
    opts = "-engine native -l1 0.01 -l2 0.05 -iters 20 -eps 0"
    by_knn = SLIM(opts, device=device).fit_csc(R, targets, knn=5).model_table()
    by_nbr = SLIM(opts, device=device).fit_csc(R, targets, nbr).model_table()
    assert len(by_nbr) > len(targets)
    pd.testing.assert_frame_equal(by_knn, by_nbr)
    by_triple = SLIM(opts, device=device).fit_csc((colptr, rows, vals), targets, knn=5).model_table()
    pd.testing.assert_frame_equal(by_triple, by_nbr)
    with pytest.raises(ValueError, match="knn"):
        SLIM(opts, device=device).fit_csc(R, targets)
    # nbr alone, positionally as before
    again = SLIM(opts, device=device).fit_csc(R, targets, nbr, None).model_table()
    pd.testing.assert_frame_equal(again, by_nbr)


def _assert_oracle_is_decisive_or_tied_by_id(full, k):
    """Adjacent distinct scores in every top-(k+1) are more than 1e-9 apart (relative): the
    neighbour sets do not hang on rounding.  Exact ties fall to the smaller id on both sides."""
    for cand in full:
        top = cand[:k + 1]
        for (a, sa), (b, sb) in zip(top[:-1], top[1:]):
            assert sa == sb or (sa - sb) / abs(sa) > 1e-9, (a, b, sa, sb)


# ------------------------------------------------------------------------ 8. topk_similar_csc
@pytest.mark.parametrize("device", DEVICES)
def test_topk_similar_csc_agrees_with_the_cosine_similarity_udf(device):
    from hivemall_amd.knn import cosine_similarity, topk_similar_csc

    Rm = _ratings(61, 70, 25, 0.2)
    colptr, rows, vals = (t.numpy() for t in _csc(Rm))
    feats = [[f"{u}:{Rm[u, j]}" for u in np.flatnonzero(Rm[:, j])] for j in range(Rm.shape[1])]
    queries = [7, 0, 24, 13]
    for R in (CSCMatrix(colptr, rows, vals, Rm.shape[0]), (colptr, rows, vals)):
        scores, indices = topk_similar_csc(R, 6, queries=queries, device=device)
        assert scores.device.type == device and tuple(scores.shape) == tuple(indices.shape) == (4, 6)
        scores, indices = scores.cpu().numpy(), indices.cpu().numpy()
        assert (indices >= 0).sum() > 12
        for t, i in enumerate(queries):
            for j, s in zip(indices[t], scores[t]):
                if j >= 0:
                    assert abs(s - cosine_similarity(feats[i], feats[j])) <= 1e-12
    every = topk_similar_csc((colptr, rows, vals), 2, device=device)[1]
    assert tuple(every.shape) == (25, 2)


# ------------------------------------------------------------------------------------- 9. SQL
@pytest.mark.parametrize("device", DEVICES)
def test_cosine_knn_table_function(device):
    from hivemall_amd.sql import Session

    Rm = _ratings(71, 40, 12, 0.3)
    full = _oracle(Rm)
    _assert_oracle_is_decisive_or_tied_by_id(full, 3)
    names = [f"item-{chr(ord('a') + (5 * j) % 12)}" for j in range(12)]     # not in sorted order
    assert len(set(names)) == 12
    u, j = np.nonzero(Rm)
    o = np.lexsort((u, j))                                   # items appear in column order
    u, j = u[o], j[o]
    tab = pd.DataFrame({"item": [names[c] for c in j], "user": [f"u{x}" for x in u],
                        "rating": Rm[u, j]})
    s = Session(device=device)
    s.register("r", tab)
    got = s.sql("SELECT cosine_knn(3, item, user, rating) AS (item, rank, other, similarity) FROM r")
    assert list(got.columns) == ["item", "rank", "other", "similarity"]
    want = [(names[i], r + 1, names[c], sc) for i in range(12) for r, (c, sc) in enumerate(full[i][:3])]
    assert len(want) > 24
    assert list(got["item"]) == [w[0] for w in want]
    assert [int(x) for x in got["rank"]] == [w[1] for w in want]
    assert list(got["other"]) == [w[2] for w in want]
    np.testing.assert_allclose(got["similarity"].to_numpy(dtype=np.float64), [w[3] for w in want],
                               rtol=RTOL, atol=0.0)
    s.register("d", pd.concat([tab, tab.iloc[[4]]], ignore_index=True))
    with pytest.raises(UDFArgumentException, match="duplicate"):
        s.sql("SELECT cosine_knn(3, item, user, rating) AS (item, rank, other, similarity) FROM d")
