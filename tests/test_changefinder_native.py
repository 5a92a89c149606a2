"""The native changefinder engine (csrc/kernels/changefinder.hip, csrc/host/changefinder_cpu.cpp,
ops/changefinder.py, ``changefinder -engine native``) against the Python path of ``changefinder``
(``-engine python``), which is the definition.

Tolerance.  The unit is ``u = |got - ref| / (eps * max(1, |ref|))``, over both output columns and
every point; no point is left out.  ``C_TOL`` was fixed once from ``_model`` below, a NumPy model
of the kernel's formulation (chunk-local scans from zero plus carries, Levinson per point) that
shares no code with the engine: over every series and option set of this file at chunk lengths
1, 64, ``CHUNK`` and N its largest distance from the Python path was 4.02e3 units (8.9e-13; sine,
k = 16, r = 0.1, T = 20, logloss, chunk length 64), and ``C_TOL`` is 8 times that rounded up to a
power of two.  The factor 8 is the margin of the sst tests: it covers the kernel's different order
of additions inside a wave scan and FMA contraction.  The twin and the kernel are both held to it.
Largest seen: twin 40 units (sine, k = 16, r = 0.1, T = 20, logloss; it follows the Python path's
operation order, what is left is libm against numpy in the last bit, and most cases are 0), kernel
7155 units (1.6e-12; noise, k = 32, hellinger) on the MI355X.

Kernel against twin: both are within ``C_TOL`` of the reference, so they are compared at
``2 * C_TOL`` units of ``max(1, |twin|)``.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from hivemall_amd.anomaly import changefinder
from hivemall_amd.utils.options import UDFArgumentException

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
EPS = float(np.finfo(np.float64).eps)
MODEL_UNITS = 4.02e3       # sine at (16, 0.1, 20, logloss), chunk length 64
C_TOL = 32768.0            # 8 * 4.02e3 = 3.22e4, rounded up to a power of two (7.3e-12)
N_SERIES = 600

# (k, r1, r2, T1, T2, loss1, loss2)
OPTION_SETS = [
    (7, .02, .02, 7, 7, "hellinger", "hellinger"),
    (7, .02, .02, 7, 7, "logloss", "logloss"),
    (1, .5, .5, 1, 1, "hellinger", "hellinger"),
    (3, .005, .005, 5, 5, "hellinger", "hellinger"),
    (32, .02, .02, 7, 7, "hellinger", "hellinger"),
    (16, .1, .1, 20, 20, "logloss", "logloss"),
    (5, .05, .01, 3, 11, "logloss", "hellinger"),
    (8, .02, .02, 7, 7, "hellinger", "hellinger"),
    (9, .02, .02, 7, 7, "hellinger", "hellinger"),
]
SERIES = ["sine", "walk", "noise", "shift", "vec3"]

_CACHE: dict = {}


def _ops():
    from hivemall_amd.ops import changefinder as ops_cf

    return ops_cf


def _series():
    if "series" not in _CACHE:
        rng = np.random.default_rng(0)
        N = N_SERIES
        t = np.arange(N)
        s = {"sine": np.where(t < N // 2, np.sin(t / 3), np.sin(t / 1.2)) + rng.normal(0, 0.1, N),
             "walk": np.cumsum(rng.normal(0, 1, N)),
             "noise": rng.normal(0, 1, N),
             "shift": np.where(t < N // 2, 0.0, 5.0) + rng.normal(0, 0.5, N),
             "vec3": np.stack([np.sin(t / 5), np.cumsum(rng.normal(0, 1, N)), rng.normal(0, 1, N)], 1)
             + rng.normal(0, .1, (N, 3))}
        # the seams need 5 * CHUNK + 17 points
        s["long"] = np.random.default_rng(1).normal(0, 1, 5 * _ops().CHUNK + 17)
        for a in s.values():
            a.setflags(write=False)
        _CACHE["series"] = s
    return _CACHE["series"]


def _opts(o, extra=""):
    k, r1, r2, T1, T2, l1, l2 = o
    return (f"-k {k} -r1 {r1} -r2 {r2} -T1 {T1} -T2 {T2} -loss_function1 {l1} "
            f"-loss_function2 {l2}{extra}")


def _reference(name, o):
    """[N, 2] of the Python path for a series and an option set, computed once.  The path is
    causal, so its first n rows are the reference of the series' first n points."""
    key = (name, o)
    if key not in _CACHE:
        ref = np.array(changefinder(list(_series()[name]), _opts(o, " -engine python")), dtype=np.float64)
        ref.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def _native(x, o, device):
    """[N, 2] (or [S, N, 2]) of the engine for x [N], [N, D] (one series) or a 3-d batch."""
    x = np.array(x, dtype=np.float64)
    xt = torch.from_numpy(x[None] if x.ndim == 2 else x).to(device)
    out, cp = _ops().changefinder_scores(xt, *o)
    want = tuple(x.shape[:2]) if x.ndim == 3 else (len(x),)
    for r in (out, cp):
        assert r.device.type == device and r.dtype == torch.float64
    if x.ndim == 2:
        assert tuple(out.shape) == (1, len(x)) == tuple(cp.shape)
        out, cp = out[0], cp[0]
    assert tuple(out.shape) == want == tuple(cp.shape)
    return np.stack([out.cpu().numpy(), cp.cpu().numpy()], -1)


def _units(got, ref):
    assert got.shape == ref.shape and np.isfinite(got).all()
    return np.abs(got - ref) / (EPS * np.maximum(1.0, np.abs(ref)))


# ----------------------------------------------------------------------- the model behind C_TOL
def _ew_scan(v, a, init, L):
    """y_t = a y_(t-1) + v_t with y_(-1) = init, as chunk-local scans from zero plus carries;
    v [N] or [N, J] (J scans side by side)."""
    N = len(v)
    y = np.empty_like(v)
    carry = np.broadcast_to(np.float64(init), v.shape[1:]).copy()
    for c0 in range(0, N, L):
        n = min(L, N - c0)
        loc = np.zeros(v.shape[1:])
        for i in range(n):
            loc = a * loc + v[c0 + i]
            y[c0 + i] = loc
        pw = a ** np.arange(1, n + 1)
        y[c0:c0 + n] += pw.reshape((n,) + (1,) * (v.ndim - 1)) * carry
        carry = y[c0 + n - 1].copy()
    return y


def _model_sdar(x, r, k, loss, L):
    N = len(x)
    a = 1 - r
    mu = _ew_scan(r * x, a, x[0], L)
    lag = np.zeros((N, k + 1))                      # x_(t-j) - mu_t, 0 where t - j < 0
    for j in range(k + 1):
        lag[j:, j] = x[:N - j] - mu[j:]
    C = _ew_scan(r * (x - mu)[:, None] * lag, a, 0.0, L)
    # Levinson-Durbin, every point at once
    w = np.zeros((N, k))
    ok = C[:, 0] > 0
    e = C[:, 0].copy()
    for i in range(k):
        acc = C[:, i + 1].copy()
        s = np.zeros(N)
        for j in range(i):
            s = s + w[:, j] * C[:, i - j]
        acc = acc - s
        with np.errstate(divide="ignore", invalid="ignore"):
            kap = np.where(ok & (e > 0), acc / e, 0.0)
        kap = np.maximum(-0.999, np.minimum(0.999, kap))
        new = w.copy()
        new[:, i] = kap
        for j in range(i):
            new[:, j] = w[:, j] - kap * w[:, i - 1 - j]
        w = new
        e = e * (1 - kap * kap)
    s = np.zeros(N)
    for i in range(k):
        s = s + w[:, i] * lag[:, i + 1]
    xhat = mu + s
    e2 = (x - xhat) ** 2
    sig = _ew_scan(r * e2, a, 1e-6, L)
    prev = np.concatenate([[1e-6], sig[:-1]])
    s2, s1 = np.maximum(sig, 1e-12), np.maximum(prev, 1e-12)
    if loss == "logloss":
        return 0.5 * np.log(2 * np.pi * s2) + e2 / (2 * s2)
    bc = np.sqrt(2 * np.sqrt(s1 * s2) / (s1 + s2))
    return np.maximum(0.0, 2 - 2 * bc * np.exp(-e2 / (4 * (s1 + s2))))


def _wmean(s, T):
    return np.array([np.mean(s[max(0, t - T + 1):t + 1]) for t in range(len(s))])


def _model(x, o, L):
    """[N, 2] of the scan formulation at chunk length L."""
    k, r1, r2, T1, T2, l1, l2 = o
    x = x[:, None] if x.ndim == 1 else x
    out = sum(_model_sdar(np.ascontiguousarray(x[:, d]), r1, k, l1, L) for d in range(x.shape[1]))
    c = _model_sdar(_wmean(out, T1), r2, k, l2, L)
    return np.stack([out, _wmean(c, T2)], -1)


@pytest.mark.parametrize("name,o,L", [("sine", OPTION_SETS[5], 1), ("sine", OPTION_SETS[5], 64),
                                      ("vec3", OPTION_SETS[0], 64), ("walk", OPTION_SETS[6], 600),
                                      ("shift", OPTION_SETS[8], 256)],
                         ids=lambda v: str(v) if not isinstance(v, tuple) else "-".join(map(str, v[:5])))
def test_the_model_behind_the_constant(name, o, L):
    """The constant stays honest: the model is within C_TOL of the Python path, and C_TOL is what
    the docstring says it is."""
    u = _units(_model(_series()[name], o, L), _reference(name, o))
    print(f"model {name} {o} L={L}: max {u.max():.4g} units")
    assert u.max() <= C_TOL
    assert C_TOL == 2.0 ** np.ceil(np.log2(8 * MODEL_UNITS))


# --------------------------------------------------------------------------- 1. the Python path
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("o", OPTION_SETS, ids=lambda o: "-".join(map(str, o)))
@pytest.mark.parametrize("name", SERIES)
def test_equals_the_python_path(name, o, device):
    ref = _reference(name, o)
    got = _native(_series()[name], o, device)
    u = _units(got, ref)
    print(f"{name} {o} {device}: max {u[:, 0].max():.4g} / {u[:, 1].max():.4g} units")
    assert u.max() <= C_TOL


# -------------------------------------------------------------------------------- 2. chunk seams
def _seam_lengths(k):
    ch = _ops().CHUNK
    return [1, 2, k, k + 1, ch - 1, ch, ch + 1, 2 * ch + 3, 5 * ch + 17]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("T", [7, 20])
@pytest.mark.parametrize("k", [7, 32])
def test_chunk_seams(k, T, device):
    """Every length around a chunk seam, with the sample halo (k) and the window halo (T) crossing
    it, and lengths below k and below T."""
    o = (k, .02, .02, T, T, "hellinger", "logloss")
    ref = _reference("long", o)
    x = _series()["long"]
    assert len(x) == _seam_lengths(k)[-1]
    for n in _seam_lengths(k):
        u = _units(_native(x[:n], o, device), ref[:n])
        print(f"k={k} T={T} N={n} {device}: max {u.max():.4g} units")
        assert u.max() <= C_TOL, n


@pytest.mark.parametrize("device", DEVICES)
def test_more_chunks_than_one_round_of_the_carry_walk(device):
    """The carry walk takes CHUNK chunk sums per round: CHUNK * CHUNK + 300 points are the
    smallest series whose walk has a second round (k = 1 keeps the Python reference short)."""
    ch = _ops().CHUNK
    if "carry" not in _CACHE:
        x = np.random.default_rng(2).normal(0, 1, ch * ch + 300)
        x.setflags(write=False)
        _series()["carry"] = x
        _CACHE["carry"] = True
    o = (1, .02, .01, 1, 3, "hellinger", "logloss")
    u = _units(_native(_series()["carry"], o, device), _reference("carry", o))
    print(f"N={ch * ch + 300} {device}: max {u[:, 0].max():.4g} / {u[:, 1].max():.4g} units, "
          f"in the second round {u[ch * ch:].max():.4g}")
    assert u.max() <= C_TOL


# ----------------------------------------------------------------------------------- 3. batching
@pytest.mark.parametrize("device", DEVICES)
def test_a_batch_equals_its_series(device):
    o = OPTION_SETS[0]
    n = _ops().CHUNK + 44
    ser = _series()
    X = np.stack([np.stack([ser["sine"][:n], ser["noise"][:n]], 1),
                  np.stack([ser["walk"][:n], ser["shift"][:n]], 1),
                  ser["vec3"][:n, :2]])                                     # [3, n, 2]
    batch = _native(X, o, device)
    assert batch.shape == (3, n, 2)
    for s in range(3):
        # the series on its own: bit for bit, on either engine (a row's chunks do not depend on
        # what else is in the batch)
        np.testing.assert_array_equal(_native(X[s], o, device), batch[s])
        # the outlier score is the sum of the two dimensions' scalar-series scores
        dims = [_native(X[s, :, d], o, device)[:, 0] for d in range(2)]
        np.testing.assert_array_equal(dims[0] + dims[1], batch[s, :, 0])
    np.testing.assert_array_equal(_native(X, o, device), batch)             # a rerun
    # a non-contiguous view is the same batch
    xt = torch.from_numpy(X).to(device).permute(2, 0, 1).contiguous().permute(1, 2, 0)
    assert not xt.is_contiguous()
    out, cp = _ops().changefinder_scores(xt, *o)
    np.testing.assert_array_equal(np.stack([out.cpu().numpy(), cp.cpu().numpy()], -1), batch)
    if device != "cpu":
        twin = _native(X, o, "cpu")
        u = np.abs(batch - twin) / (EPS * np.maximum(1.0, np.abs(twin)))
        print(f"kernel against twin: max {u.max():.4g} units")
        assert u.max() <= 2 * C_TOL
    # [N], [1, N] and [1, N, 1]
    x = ser["sine"]
    f = _ops().changefinder_scores
    a = f(torch.from_numpy(x.copy()).to(device), *o)
    b = f(torch.from_numpy(x.copy()).to(device)[None], *o)
    c = f(torch.from_numpy(x.copy()).to(device)[None, :, None], *o)
    for i in range(2):
        assert a[i].shape == (len(x),) and b[i].shape == (1, len(x)) == c[i].shape
        assert torch.equal(a[i], b[i][0]) and torch.equal(b[i], c[i])
    # nothing to do
    for shape in ((0,), (0, 5), (3, 0), (3, 0, 2), (3, 5, 0), (0, 5, 2)):
        a = f(torch.zeros(shape, dtype=torch.float64, device=device), *o)
        for r in a:
            assert tuple(r.shape) == shape[:2] and r.device.type == device and not r.any()


# --------------------------------------------------------------------------------- 4. validation
@pytest.mark.parametrize("device", DEVICES)
def test_rejects_bad_arguments(device):
    ops_cf = _ops()
    f = ops_cf.changefinder_scores
    x = torch.from_numpy(_series()["noise"][:50].copy()).to(device)
    for bad in (x.cpu().numpy(), x.tolist(), x.float(), x.long(), x[None, None, None], x.sum()):
        with pytest.raises(ValueError, match="x must"):
            f(bad)
    for k in (0, 33, -3, 2.5, None, True, "7"):
        with pytest.raises(ValueError, match="k must"):
            f(x, k)
        assert not ops_cf.supports(k, .02, .02, 7, 7, "hellinger", "hellinger")
    for r in (0, 1, 0.0, 1.0, -0.1, 1.5, None, True, "0.1", float("nan")):
        with pytest.raises(ValueError, match="r1 must"):
            f(x, r1=r)
        with pytest.raises(ValueError, match="r2 must"):
            f(x, r2=r)
        assert not ops_cf.supports(7, r, .02, 7, 7, "hellinger", "hellinger")
        assert not ops_cf.supports(7, .02, r, 7, 7, "hellinger", "hellinger")
    for T in (0, 1025, -1, 1.5, None, False):
        with pytest.raises(ValueError, match="T1 must"):
            f(x, T1=T)
        with pytest.raises(ValueError, match="T2 must"):
            f(x, T2=T)
        assert not ops_cf.supports(7, .02, .02, T, 7, "hellinger", "hellinger")
        assert not ops_cf.supports(7, .02, .02, 7, T, "hellinger", "hellinger")
    for loss in ("bogus", "Hellinger", None, 0):
        with pytest.raises(ValueError, match="loss1 must"):
            f(x, loss1=loss)
        with pytest.raises(ValueError, match="loss2 must"):
            f(x, loss2=loss)
        assert not ops_cf.supports(7, .02, .02, 7, 7, loss, "hellinger")
        assert not ops_cf.supports(7, .02, .02, 7, 7, "logloss", loss)
    for v in (float("nan"), float("inf"), -float("inf")):
        y = x.clone()
        y[7] = y[31] = v
        with pytest.raises(ValueError, match=r"x\[7\] is not finite"):
            f(y)
        with pytest.raises(ValueError, match=r"x\[\(1, 7\)\] is not finite"):
            f(torch.stack([x, y]))
        with pytest.raises(ValueError, match=r"x\[\(0, 7, 1\)\] is not finite"):
            f(torch.stack([x, y], 1)[None])
    # the limits are allowed
    assert ops_cf.K_MAX == 32 and ops_cf.supports(32, 1e-9, 1 - 1e-9, 1024, 1, "logloss", "hellinger")
    out, cp = f(x, 32, 1e-9, 1 - 1e-9, 1024, 1, "logloss", "hellinger")
    assert out.shape == x.shape == cp.shape and bool(torch.isfinite(out).all() & torch.isfinite(cp).all())
    out, cp = f(x, 1, .5, .5, 1, 1024)
    assert out.shape == x.shape == cp.shape


@pytest.mark.gpu
def test_the_result_follows_the_device_of_x():
    f = _ops().changefinder_scores
    x = torch.from_numpy(_series()["noise"].copy())
    a, b = f(x.cuda()), f(x)
    assert a[0].is_cuda and a[1].is_cuda and not b[0].is_cuda and not b[1].is_cuda
    with pytest.raises(ValueError, match="x must"):
        f(x.cuda().float())
    with pytest.raises(ValueError, match="is not finite"):
        f(torch.full((40,), float("nan"), dtype=torch.float64, device="cuda"))


# ----------------------------------------------------------------------------------- 5. surfaces
def _count_calls(monkeypatch):
    ops_cf = _ops()
    calls = []
    real = ops_cf.changefinder_scores

    def counted(x, *a, **kw):
        calls.append(x.device.type)
        return real(x, *a, **kw)

    monkeypatch.setattr(ops_cf, "changefinder_scores", counted)
    return calls


def _check_rows(rows, ref_rows):
    """The engine's rows against the Python path's: the same row lengths (flags exactly where the
    Python path has them), scores within C_TOL, flags equal wherever C_TOL decides them."""
    rows, ref_rows = list(rows), list(ref_rows)
    assert len(rows) == len(ref_rows) and [len(r) for r in rows] == [len(r) for r in ref_rows]
    got = np.array([r[:2] for r in rows], dtype=np.float64)
    ref = np.array([r[:2] for r in ref_rows], dtype=np.float64)
    assert _units(got, ref).max() <= C_TOL
    return got


@pytest.mark.parametrize("device", DEVICES)
def test_the_three_surfaces(device, monkeypatch):
    import hivemall_amd.dsl  # noqa: F401
    from hivemall_amd.sql import Session

    x = _series()["sine"]
    o = "-k 5 -T1 3"
    want = changefinder(list(x), o + " -engine python")
    calls = _count_calls(monkeypatch)
    monkeypatch.setenv("HM_DEVICE", device)
    direct = _check_rows(changefinder(list(x), o + " -engine native"), want)
    assert calls == [device]
    monkeypatch.delenv("HM_DEVICE")
    tab = pd.DataFrame({"i": np.arange(len(x)), "x": x})
    s = Session(device)
    s.register("t", tab)
    got = s.sql(f"SELECT changefinder(x, '{o} -engine native') AS s FROM t")
    np.testing.assert_array_equal(_check_rows(got["s"], want), direct)
    np.testing.assert_array_equal(
        _check_rows(tab.hivemall.on(device).changefinder("x", o + " -engine native"), want), direct)
    assert calls == [device] * 3
    # the flags: present exactly when the Python path emits them, equal wherever decided
    for th, col in (("-outlier_threshold 0.05", 0), ("-changepoint_threshold 0.02", 1),
                    ("-outlier_threshold 0.05 -changepoint_threshold 0.02", None)):
        ref_rows = changefinder(list(x), f"{o} {th} -engine python")
        rows = list(s.sql(f"SELECT changefinder(x, '{o} {th} -engine native') AS s FROM t")["s"])
        _check_rows(rows, ref_rows)
        assert len(ref_rows[0]) == 4
        ths = (0.05 if col in (0, None) else -1.0, 0.02 if col in (1, None) else -1.0)
        n_true = 0
        for row, ref in zip(rows, ref_rows):
            for c in range(2):
                if abs(ref[c] - ths[c]) > C_TOL * EPS * max(1.0, abs(ref[c])):
                    assert bool(row[2 + c]) == bool(ref[2 + c])
                    n_true += bool(row[2 + c])
        assert n_true > 0
    # a series of vectors, through a column of arrays
    v = _series()["vec3"]
    want = changefinder(list(v), o + " -engine python")
    vtab = pd.DataFrame({"x": list(v)})
    s.register("v", vtab)
    _check_rows(s.sql(f"SELECT changefinder(x, '{o} -engine native') AS s FROM v")["s"], want)
    _check_rows(vtab.hivemall.on(device).changefinder("x", o + " -engine native"), want)
    n_calls = len(calls)
    for call in (lambda: changefinder(list(x), "-engine bogus"),
                 lambda: s.sql("SELECT changefinder(x, '-engine bogus') AS s FROM t"),
                 lambda: tab.hivemall.changefinder("x", "-engine bogus")):
        with pytest.raises(UDFArgumentException, match="engine"):
            call()
    assert len(calls) == n_calls
    assert changefinder([], "-engine native") == []


@pytest.mark.parametrize("device", DEVICES)
def test_auto_is_native_on_a_cuda_session_only(device, monkeypatch):
    import hivemall_amd.dsl  # noqa: F401
    from hivemall_amd.sql import Session

    x = _series()["sine"][:300]
    python_rows = changefinder(list(x), "-engine python")
    calls = _count_calls(monkeypatch)
    # a direct call without a session never leaves the Python path, whatever the default device
    assert changefinder(list(x)) == python_rows and changefinder(list(x), "-engine auto") == python_rows
    assert (changefinder(list(x), "-outlier_threshold 0.1 -engine auto")
            == changefinder(list(x), "-outlier_threshold 0.1 -engine python"))
    assert calls == []
    tab = pd.DataFrame({"x": x})
    s = Session(device)
    s.register("t", tab)
    for q in ("SELECT changefinder(x) AS s FROM t", "SELECT changefinder(x, '-engine auto') AS s FROM t"):
        got = list(s.sql(q)["s"])
        if device == "cpu":
            assert got == python_rows and calls == []
        else:
            assert calls == ["cuda"]
            calls.clear()
            _check_rows(got, python_rows)
    got = list(tab.hivemall.on(device).changefinder("x"))
    assert calls == ([] if device == "cpu" else ["cuda"])
    if device == "cpu":
        assert got == python_rows
    else:
        _check_rows(got, python_rows)
    # outside the engine's limits or its input contract: auto runs the Python path with bit-equal
    # rows on every session, only an explicit -engine native raises
    calls.clear()
    nan = x.copy()
    nan[150] = np.nan
    ragged = [[a, a + 1.0] for a in x[:100]] + [[a] for a in x[100:200]] + [[a, 2.0, 3.0] for a in x[200:]]
    mixed = [a if i % 2 else [a] for i, a in enumerate(x)]
    for xs, o in ((list(x), "-k 33"), (list(x), "-T1 1025"), (list(nan), ""), (ragged, ""), (mixed, "")):
        want = np.array(changefinder(xs, o + " -engine python"), dtype=np.float64)
        for got in (changefinder(xs, o, session=s), changefinder(xs, o + " -engine auto", session=s)):
            np.testing.assert_array_equal(np.array(got, dtype=np.float64), want)
        assert calls == []
        with pytest.raises(UDFArgumentException, match="changefinder"):
            changefinder(xs, o + " -engine native", session=s)
        calls.clear()
    s.register("u", pd.DataFrame({"x": nan}))
    want = np.array(changefinder(list(nan), "-k 33 -engine python"), dtype=np.float64)
    got = list(s.sql("SELECT changefinder(x, '-k 33') AS s FROM u")["s"])
    np.testing.assert_array_equal(np.array(got, dtype=np.float64), want)
    with pytest.raises(UDFArgumentException, match="k must"):
        s.sql("SELECT changefinder(x, '-k 33 -engine native') AS s FROM t")
    # no device chosen: the Python path
    calls.clear()
    plain = Session()
    plain.register("t", tab)
    assert list(plain.sql("SELECT changefinder(x) AS s FROM t")["s"]) == python_rows
    assert list(pd.DataFrame({"x": x}).hivemall.changefinder("x")) == python_rows
    assert list(s.sql("SELECT changefinder(x, '-engine python') AS s FROM t")["s"]) == python_rows
    assert calls == []


@pytest.mark.gpu
def test_auto_on_a_cuda_session_takes_the_engine(monkeypatch):
    from hivemall_amd.sql import Session

    calls = _count_calls(monkeypatch)
    v = _series()["vec3"]
    s = Session("cuda")
    s.register("v", pd.DataFrame({"x": list(v)}))
    got = list(s.sql("SELECT changefinder(x, '-k 9') AS s FROM v")["s"])
    assert calls == ["cuda"]
    _check_rows(got, changefinder(list(v), "-k 9 -engine python"))
