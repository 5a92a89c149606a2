"""Per-row numpy FM oracle (Rendle SGD, the pinned train_fm rule, docs/compat.md)."""
import math

import numpy as np


def fm_train(rows, y, dims, V0, eta0=0.05, power_t=0.1, l0=0.01, lw=0.01, lv=0.01, cls=True):
    w0 = 0.0
    w = np.zeros(dims)
    V = V0.astype(np.float64).copy()
    losses = []
    for t, (feats, yy) in enumerate(zip(rows, y), start=1):
        i = np.asarray(feats)
        x = np.ones(len(i))
        S = (V[i] * x[:, None]).sum(0)
        p = w0 + (w[i] * x).sum() + 0.5 * float((S * S).sum() - ((V[i] * x[:, None]) ** 2).sum())
        if cls:
            d = -yy / (1 + math.exp(yy * p))
            losses.append(math.log1p(math.exp(-yy * p)))
        else:
            d = p - yy
        eta = eta0 / (t ** power_t)
        for j, xi in zip(i, x):
            w[j] -= eta * (d * xi + 2 * lw * w[j])
            g = d * xi * (S - V[j] * xi) + 2 * lv * V[j]
            V[j] -= eta * g
        w0 -= eta * (d + 2 * l0 * w0)
    return w0, w, V, np.array(losses)


def fm_eta(h, t0, row):
    """Learning rate of stream row ``t0 + row`` (0-based): the engines count t = t0 + row + 1 in
    float32.  h.eta_kind: 0 fixed, 1 simple, 2 inverse."""
    f = lambda v: float(np.float32(v))
    t = f(t0 + row + 1)
    if h.eta_kind == 0:
        return f(h.eta0)
    if h.eta_kind == 1:
        return f(h.eta0) / (1.0 + t / f(h.total_steps)) if f(h.total_steps) > 0 else f(h.eta0)
    return f(h.eta0) / max(t, 1.0) ** f(h.power_t)


def fm_run(indptr, idx, val, y, dims, k, V0, w_init, w0_init, hyper, t0=0, train=True, mag=None):
    """The rule at the top of csrc/kernels/fm.hip in float64, rows strictly in order.

    CSR rows ``indptr`` (absolute offsets into ``idx`` / ``val``; indptr[0] may be non-zero),
    ``val`` None = every x is 1, ``y`` None = every label is 0.  Ids outside [0, dims) contribute
    nothing and are not updated; the ids of one row must be distinct.  Only columns [0, k) of V
    take part; the others are returned as given.  ``hyper`` carries eta0, power_t, total_steps,
    eta_kind, lambda0, lambda_w, lambda_v, min_target, max_target, classification and use_w0
    (ops.fm.FMHyper); its floats are taken at float32, as the engines receive them.
    Returns (w0, w, V, pred, loss): classification pred = p, loss = log(1 + exp(-y p));
    regression pred = clip(p), loss = (clip(p) - y)^2 / 2.
    ``mag`` (a list) receives, per row, the size of what p is summed from:
    |w0| + sum |w_i x_i| + 1/2 sum_f [(sum_i |v_if x_i|)^2 + sum_i (v_if x_i)^2]; the rounding
    error of an engine's p is proportional to it, not to |p| (the pair terms cancel)."""
    h = hyper
    f = lambda v: float(np.float32(v))
    l0, lw, lv = f(h.lambda0), f(h.lambda_w), f(h.lambda_v)
    lo, hi = f(h.min_target), f(h.max_target)
    indptr = np.asarray(indptr, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    V = np.array(V0, dtype=np.float64)
    w = np.array(w_init, dtype=np.float64)
    w0 = float(w0_init)
    n = len(indptr) - 1
    pred, loss = np.zeros(n), np.zeros(n)
    for r in range(n):
        s, e = int(indptr[r]), int(indptr[r + 1])
        i = idx[s:e]
        x = np.ones(e - s) if val is None else np.asarray(val[s:e], dtype=np.float64)
        ok = (i >= 0) & (i < dims)
        i, x = i[ok], x[ok]
        assert len(np.unique(i)) == len(i), "the ids of one row must be distinct"
        Vx = V[i, :k] * x[:, None]
        S = Vx.sum(0)
        p = float((w[i] * x).sum() + 0.5 * ((S * S).sum() - (Vx * Vx).sum()))
        if h.use_w0:
            p += w0
        if mag is not None:
            mag.append((abs(w0) if h.use_w0 else 0.0) + float(np.abs(w[i] * x).sum())
                       + 0.5 * float((np.abs(Vx).sum(0) ** 2).sum() + (Vx * Vx).sum()))
        yy = 0.0 if y is None else float(y[r])
        if h.classification:
            z = yy * p
            d = -yy / (1.0 + math.exp(min(z, 700.0)))
            pred[r] = p
            loss[r] = np.logaddexp(0.0, -z)
        else:
            pc = min(max(p, lo), hi)
            d = pc - yy
            pred[r] = pc
            loss[r] = 0.5 * d * d
        if not train:
            continue
        eta = fm_eta(h, t0, r)
        w[i] -= eta * (d * x + 2 * lw * w[i])
        V[i, :k] -= eta * (d * x[:, None] * (S - Vx) + 2 * lv * V[i, :k])
        if h.use_w0:
            w0 -= eta * (d + 2 * l0 * w0)
    return w0, w, V, pred, loss
