"""The native SLIM engine (csrc/kernels/slim.hip, csrc/host/slim_cpu.cpp, ops/slim.py, and
``train_slim -engine native`` / ``SLIM.fit_csc``) against NumPy's dense Gram build and the fp64
torch descent ``slim_cd_batched`` on the CPU.

Tolerances: ratings are multiples of 0.5, so every product and partial sum of a Gram entry is
exact in fp64 and G, b must equal the dense build exactly.  The descent is compared at the bound
the project already uses between its CD implementations (rtol 1e-9, atol 1e-12); fp64
reassociation can only exceed it when an item's sweep-end ``dmax`` sits within rounding of
``eps`` (it would stop a sweep earlier or later), so the tests with ``eps > 0`` assert that the
reference's per-sweep ``dmax`` stays clear of ``eps`` for their seeds."""
import numpy as np
import pandas as pd
import pytest
import torch

from hivemall_amd.models import recommend as R
from hivemall_amd.models.recommend import SLIM, slim_cd_batched
from hivemall_amd.utils.matrix import CSCMatrix
from hivemall_amd.utils.options import UDFArgumentException

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
RTOL, ATOL = 1e-9, 1e-12


def _ops():
    from hivemall_amd.ops import slim

    return slim


def _half_steps(rng, shape):
    return rng.integers(1, 11, size=shape) * 0.5            # 0.5, 1.0, ..., 5.0


def _csc(X, device):
    """Dense [users, C] -> (colptr, rows, vals) tensors; zeros are absent."""
    cols = [np.nonzero(X[:, c])[0] for c in range(X.shape[1])]
    colptr = np.zeros(X.shape[1] + 1, dtype=np.int64)
    np.cumsum([len(r) for r in cols], out=colptr[1:])
    rows = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    vals = np.concatenate([X[r, c] for c, r in enumerate(cols)]).astype(np.float64)
    return tuple(torch.from_numpy(a).to(device) for a in (colptr, rows, vals))


def _dense_gram(X, target, nbr):
    n, K = nbr.shape
    G, b = np.zeros((n, K, K)), np.zeros((n, K))
    for t in range(n):
        Xt = np.where(nbr[t] >= 0, X[:, np.maximum(nbr[t], 0)], 0.0)
        G[t] = Xt.T @ Xt
        b[t] = Xt.T @ X[:, target[t]]
    return G, b


def _gram_case(users):
    """10 rating vectors; n = 5 items, K = 7 with -1 padding; a pair without a common user
    (columns 8, 9) and two identical columns (4, 7)."""
    rng = np.random.default_rng(11)
    lens = [0, 1, 63, 64, 65, 300] if users == 400 else [0, 1, 7, 39, 40, 20]
    X = np.zeros((users, 10))
    for c, m in enumerate(lens):
        X[rng.choice(users, size=m, replace=False), c] = _half_steps(rng, m)
    X[:, 6] = _half_steps(rng, users) * (rng.random(users) < 0.5)
    X[:, 7] = X[:, 4]
    X[: users // 4, 8] = _half_steps(rng, users // 4)
    X[users // 2: users // 2 + users // 5, 9] = _half_steps(rng, users // 5)
    target = np.array([6, 5, 2, 0, 9], dtype=np.int32)
    nbr = np.array([[0, 1, 2, 3, 4, 5, 7],
                    [4, 7, 8, 9, -1, -1, -1],
                    [5, -1, 3, -1, 6, 4, -1],
                    [-1, -1, -1, -1, -1, -1, -1],
                    [8, 6, 3, 3, 1, 0, 5]], dtype=np.int32)
    return X, target, nbr


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("users", [40, 400])
def test_gram_equals_dense_build_exactly(users, device):
    X, target, nbr = _gram_case(users)
    lens = (X != 0).sum(0)
    if users == 400:
        assert {0, 1, 63, 64, 65, 300} <= set(lens.tolist())
    assert not (X[:, 8] * X[:, 9]).any() and lens[8] and lens[9]
    G, b = _ops().slim_gram(*_csc(X, device), torch.from_numpy(target).to(device),
                            torch.from_numpy(nbr).to(device))
    G, b = G.cpu().numpy(), b.cpu().numpy()
    Ge, be = _dense_gram(X, target, nbr)
    np.testing.assert_array_equal(G, Ge)
    np.testing.assert_array_equal(b, be)
    np.testing.assert_array_equal(G, G.transpose(0, 2, 1))
    pad = nbr < 0
    assert (G[pad] == 0).all() and (G.transpose(0, 2, 1)[pad] == 0).all() and (b[pad] == 0).all()
    assert G[1, 0, 1] == G[1, 0, 0] > 0                       # identical columns 4 and 7
    assert G[1, 2, 3] == 0 and G[1, 2, 2] > 0 and G[1, 3, 3] > 0   # no common user


@pytest.mark.parametrize("device", DEVICES)
def test_gram_rejects_unsorted_rows_and_wrong_dtypes(device):
    S = _ops()
    X, target, nbr = _gram_case(40)
    colptr, rows, vals = _csc(X, device)
    t, nb = torch.from_numpy(target).to(device), torch.from_numpy(nbr).to(device)
    s = int(colptr[3])                                       # column 3 holds 39 rows
    swapped = rows.clone()
    swapped[s], swapped[s + 1] = rows[s + 1], rows[s]
    with pytest.raises(ValueError, match="increasing"):
        S.slim_gram(colptr, swapped, vals, t, nb)
    dup = rows.clone()
    dup[s + 1] = rows[s]
    with pytest.raises(ValueError, match="increasing"):
        S.slim_gram(colptr, dup, vals, t, nb)
    for bad in ((colptr.int(), rows, vals, t, nb), (colptr, rows.long(), vals, t, nb),
                (colptr, rows, vals.float(), t, nb), (colptr, rows, vals, t.long(), nb),
                (colptr, rows, vals, t, nb.long()), (colptr.numpy(force=True), rows, vals, t, nb)):
        with pytest.raises(ValueError):
            S.slim_gram(*bad)
    with pytest.raises(ValueError, match="column ids"):
        S.slim_gram(colptr, rows, vals, t, nb + 4)
    with pytest.raises(ValueError):
        S.slim_cd(torch.zeros(2, 3, 3, device=device), torch.zeros(2, 3, dtype=torch.float64, device=device),
                  0.1, 0.1, 3, 0.0)


# ---------------------------------------------------------------------------------- descent
def _cd_problem(K, n, seed):
    rng = np.random.default_rng(seed)
    U = 2 * K + 5
    G, b = np.zeros((n, K, K)), np.zeros((n, K))
    for t in range(n):
        X = rng.random((U, K)) * (rng.random((U, K)) < 0.4)
        G[t] = X.T @ X
        b[t] = X.T @ (rng.random(U) * (rng.random(U) < 0.5))
    return G, b


_REF: dict = {}


def _reference(key, G, b, l1, l2, iters, eps):
    """slim_cd_batched on the CPU, computed once per problem and shared by the device variants."""
    if key not in _REF:
        W = slim_cd_batched(list(G), list(b), l1, l2, iters, eps)
        W.setflags(write=False)
        _REF[key] = W
    return _REF[key]


def _native_cd(G, b, l1, l2, iters, eps, device):
    W = _ops().slim_cd(torch.from_numpy(G).to(device), torch.from_numpy(b).to(device), l1, l2, iters, eps)
    assert W.dtype == torch.float64 and W.device.type == device
    return W.cpu().numpy()


def _sweep_dmax(G, b, l1, l2, iters, eps):
    """The scalar loop again, returning every sweep's dmax up to the stop."""
    w, out = np.zeros(len(b)), []
    for _ in range(iters):
        dmax = 0.0
        for k in range(len(b)):
            if G[k, k] <= 0:
                continue
            nw = max(0.0, b[k] - G[k] @ w + G[k, k] * w[k] - l1) / (G[k, k] + l2)
            dmax = max(dmax, abs(nw - w[k]))
            w[k] = nw
        out.append(dmax)
        if dmax < eps:
            break
    return out


def _assert_clear_of_eps(Gs, bs, l1, l2, iters, eps):
    """No item's sweep-end dmax within 1e-9 (relative) of eps: the stop sweep is not a matter of
    rounding.  Returns the number of sweeps each item ran."""
    sweeps = []
    for G, b in zip(Gs, bs):
        d = _sweep_dmax(np.asarray(G), np.asarray(b), l1, l2, iters, eps)
        assert all(abs(x - eps) > 1e-9 * eps for x in d), d
        sweeps.append(len(d))
    return sweeps


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("K", [1, 31, 32, 33, 63, 64, 65, 127, 128])
def test_cd_matches_torch_reference(K, n, device):
    G, b = _cd_problem(K, n, seed=100 + K)
    args = (0.01, 0.05, 50, 0.0)
    W = _native_cd(G, b, *args, device)
    np.testing.assert_allclose(W, _reference(("full", K, n), G, b, *args), rtol=RTOL, atol=ATOL)
    assert (W >= 0).all() and W.any()


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("K", [33, 65])
def test_cd_early_stop_matches_torch_reference(K, device):
    G, b = _cd_problem(K, 5, seed=100 + K)
    args = (0.01, 0.05, 30, 1e-4)
    sweeps = _assert_clear_of_eps(G, b, *args)
    if K == 33:                     # at K = 65 these inputs need more than 30 sweeps
        assert max(sweeps) < 30 and len(set(sweeps)) > 1      # items stop, on different sweeps
    W = _native_cd(G, b, *args, device)
    np.testing.assert_allclose(W, _reference(("eps", K), G, b, *args), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("device", DEVICES)
def test_cd_item_stops_alone_inside_a_workgroup(device):
    """Item 0 (diagonal G) is exact after sweep 1 and stops after sweep 2; items 1..3, in the same
    workgroup, go on."""
    G, b = _cd_problem(8, 4, seed=7)
    G[0] = np.diag(np.diag(G[0]))
    args = (0.01, 0.05, 30, 1e-6)
    sweeps = _assert_clear_of_eps(G, b, *args)
    assert sweeps[0] == 2 and min(sweeps[1:]) > 2
    W = _native_cd(G, b, *args, device)
    np.testing.assert_allclose(W[0], np.maximum(0.0, b[0] - 0.01) / (np.diag(G[0]) + 0.05),
                               rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(W, _reference(("diag",), G, b, *args), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("device", DEVICES)
def test_cd_dead_coordinates_zero_iters_and_large_l1(device):
    G, b = _cd_problem(9, 3, seed=9)
    G[1, 4, :] = 0
    G[1, :, 4] = 0
    b[1, 4] = 3.0                                            # would move if it were visited
    args = (0.01, 0.05, 50, 0.0)
    W = _native_cd(G, b, *args, device)
    assert (W[1, 4] == 0) and W[1].any()
    np.testing.assert_allclose(W, _reference(("dead",), G, b, *args), rtol=RTOL, atol=ATOL)
    assert not _native_cd(G, b, 0.01, 0.05, 0, 0.0, device).any()
    assert not _native_cd(G, b, float(b.max()) + 1.0, 0.05, 20, 0.0, device).any()


@pytest.mark.parametrize("device", DEVICES)
def test_cd_rejects_more_than_128_neighbours(device):
    G = torch.zeros(1, 129, 129, dtype=torch.float64, device=device)
    with pytest.raises(ValueError, match="128"):
        _ops().slim_cd(G, G[:, 0], 0.01, 0.05, 1, 0.0)


# ---------------------------------------------------------------------------------- learner
def _ratings(seed, n_users, n_items, density=0.35):
    rng = np.random.default_rng(seed)
    return _half_steps(rng, (n_users, n_items)) * (rng.random((n_users, n_items)) < density)


def _vec(Rm, j):
    return {int(u) * 3 + 100: float(Rm[u, j]) for u in np.nonzero(Rm[:, j])[0]}


def _sql_rows(Rm, nbrs, unrated=(), self_row=()):
    """train_slim's input rows: the first half of an item's neighbours as (j, r_j) rows, the
    rest through topKRatesOfI on its last row (so the neighbour order is ``nbrs[i]``'s)."""
    out = []
    for i, nbs in nbrs.items():
        ri = None if i in unrated else _vec(Rm, i)
        explicit = list(nbs[: (len(nbs) + 1) // 2]) + ([i] if i in self_row else [])
        knn = {j: _vec(Rm, j) for j in nbs[(len(nbs) + 1) // 2:]}
        for q, j in enumerate(explicit):
            out.append((i, ri, knn if q == len(explicit) - 1 and knn else None, j, _vec(Rm, j)))
    return [list(c) for c in zip(*out)]


def _small_case():
    """12 items, 60 users, 1-9 neighbours each; item 3 also names itself, item 7 has no ratings."""
    Rm = _ratings(21, 60, 12)
    rng = np.random.default_rng(22)
    nbrs = {}
    for i in range(12):
        others = [j for j in range(12) if j != i]
        nbrs[i] = [int(j) for j in rng.choice(others, size=1 + i % 9, replace=False)]
    return Rm, nbrs


def _problems(Rm, nbrs, skip=()):
    items = [i for i in nbrs if i not in skip]
    return ([Rm[:, nbrs[i]].T @ Rm[:, nbrs[i]] for i in items], [Rm[:, nbrs[i]].T @ Rm[:, i] for i in items])


def _model(learner):
    tab = learner.model_table()
    assert list(tab.columns) == ["i", "nn", "w"]
    return {(int(a), int(b)): float(v) for a, b, v in tab.itertuples(index=False)}


def _assert_same_model(a, b, rtol=RTOL, atol=ATOL):
    keys = sorted(set(a) | set(b))
    assert keys
    np.testing.assert_allclose([a.get(k, 0.0) for k in keys], [b.get(k, 0.0) for k in keys],
                               rtol=rtol, atol=atol)


@pytest.mark.parametrize("device", DEVICES)
def test_fit_native_matches_torch_engine(device):
    Rm, nbrs = _small_case()
    _assert_clear_of_eps(*_problems(Rm, nbrs, skip=(7,)), 0.001, 0.0005, 30, 1e-4)
    rows = _sql_rows(Rm, nbrs, unrated=(7,), self_row=(3,))
    native = _model(SLIM("-engine native", device=device).fit(*rows))
    ref = _model(SLIM("-engine torch", device="cpu").fit(*rows))
    _assert_same_model(native, ref)
    assert not any(i == 7 or i == nn for i, nn in native) and len(native) > 12
    assert SLIM("", device=device).engine() == "native"      # auto: the library is there


def _csc_of(Rm):
    colptr, rows, vals = (t.numpy() for t in _csc(Rm, "cpu"))
    return CSCMatrix(colptr, rows, vals, Rm.shape[0])


def test_fit_csc_matches_fit_and_takes_torch_cd_above_128_neighbours():
    Rm = _ratings(31, 60, 140, density=0.2)
    rng = np.random.default_rng(32)
    nbrs = {0: list(range(1, 131))}
    for i in range(1, 9):
        nbrs[i] = [int(j) for j in rng.choice([j for j in range(140) if j != i], size=i, replace=False)]
    opts = " -iters 10 -eps 0"
    rows = _sql_rows(Rm, nbrs)
    by_rows = SLIM("-engine native" + opts, device="cpu").fit(*rows)
    items = list(nbrs)
    by_csc = SLIM("-engine native" + opts, device="cpu").fit_csc(_csc_of(Rm), items, [nbrs[i] for i in items])
    triple = _csc_of(Rm)
    padded = np.full((len(items), 131), -1, dtype=np.int64)
    for t, i in enumerate(items):
        padded[t, 1:1 + len(nbrs[i])] = nbrs[i]               # padding in front: order is kept
    by_triple = SLIM("-engine native" + opts, device="cpu").fit_csc(
        (triple.indptr, triple.indices, triple.values), np.asarray(items), padded)
    ref = _model(SLIM("-engine torch" + opts, device="cpu").fit(*rows))
    assert sum(1 for i, _ in ref if i == 0) > 5
    # ratings are multiples of 0.5: both native routes see the same exact G and b
    pd.testing.assert_frame_equal(by_csc.model_table(), by_rows.model_table())
    pd.testing.assert_frame_equal(by_triple.model_table(), by_csc.model_table())
    _assert_same_model(_model(by_csc), ref)
    assert [nn for i, nn in _model(by_csc) if i == 0] == [nn for i, nn in ref if i == 0]


def test_fit_csc_chunked_equals_one_shot(monkeypatch):
    Rm = _ratings(41, 50, 45, density=0.3)
    rng = np.random.default_rng(42)
    sizes = list(rng.integers(1, 6, size=40)) + [30]
    items = list(range(len(sizes)))
    nbr = [[int(j) for j in rng.choice([j for j in range(45) if j != i], size=m, replace=False)]
           for i, m in zip(items, sizes)]
    opts = "-engine native -l1 0.01 -l2 0.05 -iters 40 -eps 1e-8"
    full = _model(SLIM(opts, device="cpu").fit_csc(_csc_of(Rm), items, nbr))
    calls = []
    S = _ops()
    monkeypatch.setattr(R, "_SLIM_CHUNK_BYTES", 4 * 6 * 6 * 8)      # <= 4 small items per chunk
    monkeypatch.setattr(S, "slim_cd", lambda G, *a, _f=S.slim_cd: calls.append(G.shape) or _f(G, *a))
    chunked = _model(SLIM(opts, device="cpu").fit_csc(_csc_of(Rm), items, nbr))
    assert len(calls) > 2 and calls[-1] == (1, 30, 30)
    assert set(chunked) == set(full)
    _assert_same_model(chunked, full, rtol=1e-12, atol=0.0)


def test_train_slim_sql_engine_option():
    from hivemall_amd.sql import Session

    Rm, nbrs = _small_case()
    _assert_clear_of_eps(*_problems(Rm, nbrs), 0.001, 0.0005, 30, 1e-4)
    i, r_i, knn_i, j, r_j = _sql_rows(Rm, nbrs)
    s = Session(device="cpu")
    s.register("t", pd.DataFrame({"i": i, "r_i": r_i, "knn_i": knn_i, "j": j, "r_j": r_j}))
    q = "SELECT train_slim(i, r_i, knn_i, j, r_j, '-engine {} -l1 0.001 -l2 0.0005') AS (i, nn, w) FROM t"
    tabs = {e: s.sql(q.format(e)) for e in ("native", "torch")}
    models = {e: {(int(a), int(b)): float(v) for a, b, v in t[["i", "nn", "w"]].itertuples(index=False)}
              for e, t in tabs.items()}
    assert len(models["torch"]) > 12
    _assert_same_model(models["native"], models["torch"])
    with pytest.raises(UDFArgumentException, match="engine"):
        s.sql(q.format("fast"))
