"""Anomaly / change-point detection (upstream core/src/main/java/hivemall/
anomaly/{ChangeFinderUDF,ChangeFinder1D,ChangeFinder2D,SDAR1D,SDAR2D,
SingularSpectrumTransformUDF,SingularSpectrumTransform}.java).

Both are streaming functions over an ordered series; they are registered as *vectorised* UDFs
(the executor hands over the whole ordered column) so the SDAR / SST state lives in one
object per call.
"""
from __future__ import annotations

import math

import numpy as np

from ..registry import udf
from ..utils.options import Options, UDFArgumentException, flag, opt

_CF_OPTS = Options([
    opt("k", None, 7, int, "Order of the AR model"),
    opt("r1", None, 0.02, float, "Discounting rate of the outlier stage"),
    opt("r2", None, 0.02, float, "Discounting rate of the change-point stage"),
    opt("T1", None, 7, int, "Smoothing window of the outlier scores"),
    opt("T2", None, 7, int, "Smoothing window of the change-point scores"),
    opt("outlier_threshold", None, -1.0, float, "Outlier threshold (emit is_outlier)"),
    opt("changepoint_threshold", None, -1.0, float, "Change-point threshold"),
    opt("loss_function", None, "hellinger", str, "hellinger | logloss"),
    opt("loss_function1", None, None, str, "Loss of stage 1"),
    opt("loss_function2", None, None, str, "Loss of stage 2"),
    opt("engine", None, "auto", str, "auto | native | python: native = the time-parallel SDAR scan "
        "engine (ops/changefinder.py); auto = native on a cuda session for options inside its "
        "limits and a finite rectangular input, python otherwise")], "changefinder")


class SDAR1D:
    """Sequentially discounting AR model (Yamanishi & Takeuchi 2002)."""

    def __init__(self, r: float, k: int):
        self.r, self.k = r, k
        self.mu = 0.0
        self.C = np.zeros(k + 1)
        self.sigma = 0.0
        self.hist: list[float] = []
        self.n = 0

    def update(self, x: float, loss: str) -> float:
        r, k = self.r, self.k
        if self.n == 0:
            self.mu = x
            self.sigma = 1e-6
        self.mu = (1 - r) * self.mu + r * x
        past = self.hist[::-1]  # x_{t-1}, x_{t-2}, ...
        for j in range(k + 1):
            xj = x if j == 0 else (past[j - 1] if j - 1 < len(past) else self.mu)
            self.C[j] = (1 - r) * self.C[j] + r * (x - self.mu) * (xj - self.mu)
        w = _levinson(self.C)
        xhat = self.mu + sum(w[i] * ((past[i] if i < len(past) else self.mu) - self.mu)
                             for i in range(k))
        prev_sigma = self.sigma
        self.sigma = (1 - r) * self.sigma + r * (x - xhat) ** 2
        self.hist.append(x)
        if len(self.hist) > k:
            self.hist.pop(0)
        self.n += 1
        s2 = max(self.sigma, 1e-12)
        if loss == "logloss":
            return 0.5 * math.log(2 * math.pi * s2) + (x - xhat) ** 2 / (2 * s2)
        # Hellinger distance between the predictive distributions before / after the update
        s1 = max(prev_sigma, 1e-12)
        bc = math.sqrt(2 * math.sqrt(s1 * s2) / (s1 + s2))
        return max(0.0, 2.0 - 2.0 * bc * math.exp(-(x - xhat) ** 2 / (4 * (s1 + s2))))


def _levinson(C: np.ndarray) -> np.ndarray:
    """Solve the Yule-Walker equations Σ_j w_j C_|i-j| = C_{i+1} (Levinson-Durbin)."""
    k = len(C) - 1
    if C[0] <= 0:
        return np.zeros(k)
    a = np.zeros(k)
    e = C[0]
    for i in range(k):
        acc = C[i + 1] - sum(a[j] * C[i - j] for j in range(i))
        kappa = acc / e if e > 0 else 0.0
        kappa = max(-0.999, min(0.999, kappa))
        new = a.copy()
        new[i] = kappa
        for j in range(i):
            new[j] = a[j] - kappa * a[i - 1 - j]
        a = new
        e *= (1 - kappa * kappa)
    return a


class ChangeFinder:
    def __init__(self, options: str | None):
        c = _CF_OPTS.parse(options)
        self.c = c
        l1 = c["loss_function1"] or c["loss_function"]
        l2 = c["loss_function2"] or c["loss_function"]
        self.l1, self.l2 = l1, l2
        self.s1: list = []
        self.s2: list = []
        self.m1 = None
        self.m2 = None

    def _mk(self, dim, r):
        return [SDAR1D(r, self.c["k"]) for _ in range(dim)]

    def step(self, x):
        xs = np.atleast_1d(np.asarray(x, dtype=np.float64))
        if self.m1 is None:
            self.m1 = self._mk(len(xs), self.c["r1"])
            self.m2 = SDAR1D(self.c["r2"], self.c["k"])
        o = float(sum(m.update(float(v), self.l1) for m, v in zip(self.m1, xs)))
        self.s1.append(o)
        y = float(np.mean(self.s1[-self.c["T1"]:]))
        cp_raw = self.m2.update(y, self.l2)
        self.s2.append(cp_raw)
        cp = float(np.mean(self.s2[-self.c["T2"]:]))
        out = [o, cp]
        if self.c["outlier_threshold"] >= 0 or self.c["changepoint_threshold"] >= 0:
            out += [o > self.c["outlier_threshold"] >= 0, cp > self.c["changepoint_threshold"] >= 0]
        return out


def _cf_rectangular(xs):
    """The input as fp64 [N, D] if it is all scalars or all vectors of one length, else None."""
    try:
        rows = [np.asarray(x, dtype=np.float64) for x in xs]
    except (TypeError, ValueError):
        return None
    if not rows or any(r.ndim != rows[0].ndim or r.shape != rows[0].shape for r in rows):
        return None
    if rows[0].ndim > 1:
        return None
    return np.stack(rows).reshape(len(rows), -1)


def _cf_native(x: np.ndarray, c, l1, l2, device):
    """The rows of ``changefinder`` from ``ops.changefinder.changefinder_scores`` on ``device``."""
    import torch

    from ..ops import changefinder as ops_cf

    try:
        o, cp = ops_cf.changefinder_scores(torch.from_numpy(x[None]).to(device), c["k"], c["r1"],
                                           c["r2"], c["T1"], c["T2"], l1, l2)
    except ValueError as ex:
        raise UDFArgumentException(str(ex)) from None
    ot, ct = c["outlier_threshold"], c["changepoint_threshold"]
    rows = zip(o[0].cpu().tolist(), cp[0].cpu().tolist())
    if ot >= 0 or ct >= 0:
        return [[a, b, a > ot >= 0, b > ct >= 0] for a, b in rows]
    return [[a, b] for a, b in rows]


@udf("changefinder", vectorized=True)
def changefinder(xs, options=None, session=None):
    """Per ordered input: [outlier_score, changepoint_score(, is_outlier, is_changepoint)].
    `-engine native` runs the time-parallel SDAR scan engine (ops/changefinder.py: the gfx950
    kernels on a cuda device, the OpenMP twin on the CPU); `-engine auto` (default) picks it on a
    cuda session when the options are inside its limits (k <= 32, T1, T2 <= 1024) and the input is
    finite and rectangular, and the per-point Python loop otherwise."""
    o = options[0] if isinstance(options, (list, tuple, np.ndarray)) else options
    cf = ChangeFinder(o)
    engine = cf.c["engine"]
    if engine not in ("auto", "native", "python"):
        raise UDFArgumentException(f"changefinder: -engine must be auto, native or python, got {engine!r}")
    if engine != "python":
        from ..models.base import resolve_device

        dev = None if session is None or session.device is None else resolve_device(session.device)
        if engine == "native" or (dev is not None and dev.type == "cuda"):
            from ..ops.changefinder import supports

            xs = list(xs)
            x = _cf_rectangular(xs)
            c = cf.c
            if engine == "native":
                if not xs:
                    return []
                if x is None:
                    raise UDFArgumentException("changefinder: -engine native needs all scalars or all "
                                               "vectors of one length")
                return _cf_native(x, c, cf.l1, cf.l2, dev or resolve_device(None))
            # auto: the native engine on a cuda session, for options inside its limits and a finite
            # rectangular input; everything else runs below as it always did
            if (x is not None and x.size and bool(np.isfinite(x).all())
                    and supports(c["k"], c["r1"], c["r2"], c["T1"], c["T2"], cf.l1, cf.l2)):
                return _cf_native(x, c, cf.l1, cf.l2, dev)
    return [cf.step(x) for x in xs]


changefinder.wants_session = True


_SST_OPTS = Options([
    opt("w", "window", 30, int, "Window size"),
    opt("n", "n_past", None, int, "Number of past windows"),
    opt("m", "n_current", None, int, "Number of current windows"),
    opt("g", "current_offset", None, int, "Offset of the current windows"),
    opt("r", "n_component", 3, int, "Rank of the past subspace"),
    opt("k", "n_dim", 5, int, "Rank of the current subspace"),
    opt("th", "threshold", -1.0, float, "Change-point threshold"),
    opt("engine", None, "auto", str, "auto | native | numpy: native = the batched Jacobi SVD "
        "engine (ops/sst.py); auto = native on a cuda session for a shape inside its limits, "
        "numpy otherwise"),
    flag("ika", None, "Use the implicit Krylov approximation",
         inert="SST uses an exact (batched) SVD")], "sst")


def _sst_native(x: np.ndarray, w, n, m, g, r, k, th, device):
    """The rows of ``sst`` from ``ops.sst.sst_scores`` on ``device``."""
    import torch

    from ..ops import sst as ops_sst

    try:
        score = ops_sst.sst_scores(torch.from_numpy(x).to(device), w, n, m, g, r, k)
    except ValueError as ex:
        raise UDFArgumentException(str(ex)) from None
    score = score.cpu().tolist()
    return [[v] for v in score] if th < 0 else [[v, v > th] for v in score]


@udf("sst", vectorized=True)
def sst(xs, options=None, session=None):
    """Singular spectrum transformation score per point: 1 - (largest singular value of
    U_pastᵀ U_current)² between the top-r past and top-k current subspaces. `-engine native`
    runs the batched Jacobi SVD engine (ops/sst.py: the gfx950 kernel on a cuda device, its
    OpenMP twin on the CPU); `-engine auto` (default) picks it on a cuda session when the shape is
    inside its limits (w, n, m <= 64) and the per-point LAPACK loop otherwise."""
    o = options[0] if isinstance(options, (list, tuple, np.ndarray)) else options
    c = _SST_OPTS.parse(o)
    w = c["w"]
    n = c["n"] or w
    m = c["m"] or w
    g = c["g"] if c["g"] is not None else -w
    r, k = c["r"], c["k"]
    engine = c["engine"]
    if engine not in ("auto", "native", "numpy"):
        raise UDFArgumentException(f"sst: -engine must be auto, native or numpy, got {engine!r}")
    x = np.asarray(list(xs), dtype=np.float64)
    if engine != "numpy":
        from ..models.base import resolve_device
        from ..ops.sst import supports

        dev = None if session is None or session.device is None else resolve_device(session.device)
        if engine == "native":
            return _sst_native(x, w, n, m, g, r, k, c["th"], dev or resolve_device(None))
        # auto: the native engine on a cuda session, for a shape inside its limits and finite
        # samples; everything else runs below as it always did
        if (dev is not None and dev.type == "cuda" and supports(w, n, m, g, r, k)
                and bool(np.isfinite(x).all())):
            return _sst_native(x, w, n, m, g, r, k, c["th"], dev)
    out = []
    need = w + n + max(0, -g) + m
    for t in range(len(x)):
        if t + 1 < need:
            out.append([0.0] if c["th"] < 0 else [0.0, False])
            continue
        end = t + 1
        past = np.stack([x[end + g - m - n + i - w + 1: end + g - m - n + i + 1] for i in range(n)], 1)
        cur = np.stack([x[end - m + i - w + 1: end - m + i + 1] for i in range(m)], 1)
        U, _, _ = np.linalg.svd(past, full_matrices=False)
        Q, _, _ = np.linalg.svd(cur, full_matrices=False)
        s = np.linalg.svd(U[:, :r].T @ Q[:, :k], compute_uv=False)
        score = float(1.0 - (s[0] ** 2 if s.size else 0.0))
        out.append([score] if c["th"] < 0 else [score, score > c["th"]])
    return out


sst.wants_session = True
