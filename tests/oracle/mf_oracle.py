"""Sequential numpy / float64 restatement of the MF and BPR-MF rules (csrc/kernels/mf.hip header;
upstream hivemall.mf.{MatrixFactorizationSGDUDTF,MatrixFactorizationAdaGradUDTF,
BPRMatrixFactorizationUDTF}) and of the kernels' counter-based negative sampler.

  * ``mf_seq``        biased MF, SGD or AdaGrad, one rating at a time, in order;
  * ``bpr_seq``       BPR-MF, one triple at a time, in order;
  * ``bpr_pipelined`` the documented order of bpr_pf3_kernel: per slot chain (the triples
                      r, r + stride, r + 2 stride, ... one group of lanes handles) triple q + 1
                      gathers its rows after q - 1's stores and before q's, and every store
                      overwrites the whole value with "gathered value + step";
  * ``pcg_draw``      the (u, i, j) the device sampler draws for stream position ``t``.

The learning-rate clock is ``t = t0 + r + 1`` and is carried by the caller across epochs
(``t0`` grows by the number of rows, skipped ones included).  Hyper-parameters reach the engines
as fp32, so they are rounded through fp32 here; everything else is float64.
"""
import numpy as np

M64 = (1 << 64) - 1
PCG_MUL = 6364136223846793005
PCG_INC = 1442695040888963407
GOLDEN = 0x9E3779B97F4A7C15


def _f32(x) -> float:
    return float(np.float32(x))


def eta_at(kind: str, eta0: float, t: float, power_t: float, total_steps: float) -> float:
    if kind == "fixed":
        return eta0
    if kind == "simple":
        return eta0 / (1.0 + t / total_steps) if total_steps > 0 else eta0
    if kind == "inverse":
        return eta0 / max(t, 1.0) ** power_t
    raise ValueError(kind)


def log1pexp(x: float) -> float:
    return float(np.logaddexp(0.0, x))


def _note(step, row, delta) -> None:
    """Record the size (largest |component|) of one update of ``row``.  A test asserts on the
    largest update every touched row received: the net displacement of a row can cancel over
    its visits (it does at k = 1), the size of an update cannot."""
    step[row] = max(step[row], float(np.max(np.abs(delta))))


# ------------------------------------------------------------------------------------ MF
def mf_seq(u, i, r, P, Q, mu, *, adagrad=False, eta0=0.1, lam=0.03, eps=1.0, use_bias=True,
           eta_kind="fixed", power_t=0.1, total_steps=-1.0, epochs=1, t0=0):
    """``epochs`` in-order passes.  Returns a dict: P, Q, Bu, Bi, GP, GQ, GBu, GBi (float64),
    ``rhat`` / ``e2`` [epochs, n] (NaN on skipped rows), ``loss`` [epochs], the clock ``t`` and
    ``step``: per table row, the largest single update it received (see ``_note``)."""
    P, Q = np.array(P, dtype=np.float64), np.array(Q, dtype=np.float64)
    nu, ni = P.shape[0], Q.shape[0]
    Bu, Bi = np.zeros(nu), np.zeros(ni)
    GP, GQ, GBu, GBi = np.zeros_like(P), np.zeros_like(Q), np.zeros(nu), np.zeros(ni)
    step = dict(P=np.zeros(nu), Q=np.zeros(ni), Bu=np.zeros(nu), Bi=np.zeros(ni))
    eta0, lam, eps, power_t, total_steps, mu = (_f32(v) for v in (eta0, lam, eps, power_t, total_steps, mu))
    n = len(u)
    rhat = np.full((epochs, n), np.nan)
    e2 = np.full((epochs, n), np.nan)
    t = int(t0)
    for ep in range(epochs):
        for row in range(n):
            a, b = int(u[row]), int(i[row])
            if not (0 <= a < nu and 0 <= b < ni):
                continue
            bu, bi = (Bu[a], Bi[b]) if use_bias else (0.0, 0.0)
            pa, qb = P[a].copy(), Q[b].copy()
            rh = mu + bu + bi + pa @ qb
            e = float(r[row]) - rh
            rhat[ep, row], e2[ep, row] = rh, e * e
            gp, gq = e * qb - lam * pa, e * pa - lam * qb
            gbu, gbi = e - lam * bu, e - lam * bi
            if not adagrad:
                eta = eta_at(eta_kind, eta0, float(t + row + 1), power_t, total_steps)
                P[a], Q[b] = pa + eta * gp, qb + eta * gq
                if use_bias:
                    Bu[a], Bi[b] = bu + eta * gbu, bi + eta * gbi
            else:
                GP[a] += gp * gp
                GQ[b] += gq * gq
                P[a] = pa + eta0 * gp / np.sqrt(eps + GP[a])
                Q[b] = qb + eta0 * gq / np.sqrt(eps + GQ[b])
                if use_bias:
                    GBu[a] += gbu * gbu
                    GBi[b] += gbi * gbi
                    Bu[a] = bu + eta0 * gbu / np.sqrt(eps + GBu[a])
                    Bi[b] = bi + eta0 * gbi / np.sqrt(eps + GBi[b])
            _note(step["P"], a, P[a] - pa)
            _note(step["Q"], b, Q[b] - qb)
            if use_bias:
                _note(step["Bu"], a, Bu[a] - bu)
                _note(step["Bi"], b, Bi[b] - bi)
        t += n
    return dict(P=P, Q=Q, Bu=Bu, Bi=Bi, GP=GP, GQ=GQ, GBu=GBu, GBi=GBi, rhat=rhat, e2=e2,
                loss=np.nansum(e2, axis=1), t=t, step=step)


# ------------------------------------------------------------------------------------ BPR
class _BPR:
    """Tables and hyper-parameters of one BPR run; ``gather`` / ``store`` are the two halves of a
    triple's update, so the sequential and the pipelined order share one rule."""

    def __init__(self, P, Q, Bi, loss, eta0, lambda_u, lambda_i, lambda_j, lambda_b, use_bias,
                 eta_kind, power_t, total_steps):
        self.P, self.Q = np.array(P, dtype=np.float64), np.array(Q, dtype=np.float64)
        self.Bi = np.zeros(self.Q.shape[0]) if Bi is None else np.array(Bi, dtype=np.float64)
        self.loss = int(loss)
        self.eta0, self.lu, self.li, self.lj, self.lb, self.power_t, self.total = (
            _f32(v) for v in (eta0, lambda_u, lambda_i, lambda_j, lambda_b, power_t, total_steps))
        self.use_bias, self.eta_kind = bool(use_bias), eta_kind
        self.step = dict(P=np.zeros(self.P.shape[0]), Q=np.zeros(self.Q.shape[0]),
                         Bi=np.zeros(self.Q.shape[0]))

    def valid(self, u, i, j) -> bool:
        return 0 <= u < self.P.shape[0] and 0 <= i < self.Q.shape[0] and 0 <= j < self.Q.shape[0] and i != j

    def gather(self, u, i, j):
        if not self.valid(u, i, j):
            return None
        bi, bj = (self.Bi[i], self.Bi[j]) if self.use_bias else (0.0, 0.0)
        return self.P[u].copy(), self.Q[i].copy(), self.Q[j].copy(), bi, bj

    def store(self, u, i, j, g, t) -> float:
        """Apply the step computed from the gathered values ``g`` at clock ``t``; returns the
        triple's loss log(1 + exp(-x))."""
        pu, qi, qj, bi, bj = g
        x = bi - bj + pu @ (qi - qj)
        if self.loss == 2:
            s = 1.0 / (1.0 + np.exp(-x))
            z = s * (1.0 - s)
        else:                                   # lnLogistic and logistic: sigma(-x)
            z = 1.0 / (1.0 + np.exp(x))
        eta = eta_at(self.eta_kind, self.eta0, float(t), self.power_t, self.total)
        self.P[u] = pu + eta * (z * (qi - qj) - self.lu * pu)
        self.Q[i] = qi + eta * (z * pu - self.li * qi)
        self.Q[j] = qj + eta * (-z * pu - self.lj * qj)
        if self.use_bias:
            self.Bi[i] = bi + eta * (z - self.lb * bi)
            self.Bi[j] = bj + eta * (-z - self.lb * bj)
            _note(self.step["Bi"], i, self.Bi[i] - bi)
            _note(self.step["Bi"], j, self.Bi[j] - bj)
        _note(self.step["P"], u, self.P[u] - pu)
        _note(self.step["Q"], i, self.Q[i] - qi)
        _note(self.step["Q"], j, self.Q[j] - qj)
        return log1pexp(-x)

    def result(self, losses, t):
        return dict(P=self.P, Q=self.Q, Bi=self.Bi, loss=np.asarray(losses), t=t, step=self.step)


def bpr_seq(tu, ti, tj, P, Q, Bi=None, *, loss=0, eta0=0.005, lambda_u=1e-4, lambda_i=1e-4,
            lambda_j=1e-4, lambda_b=0.01, use_bias=True, eta_kind="fixed", power_t=0.1,
            total_steps=-1.0, epochs=1, t0=0):
    """``epochs`` in-order passes over the triples.  Returns P, Q, Bi, ``loss`` [epochs] (the sum
    of log(1 + exp(-x)) over the valid triples), the clock ``t`` and ``step`` as ``mf_seq``."""
    m = _BPR(P, Q, Bi, loss, eta0, lambda_u, lambda_i, lambda_j, lambda_b, use_bias, eta_kind,
             power_t, total_steps)
    n, t, losses = len(tu), int(t0), []
    for _ in range(epochs):
        acc = 0.0
        for r in range(n):
            trip = int(tu[r]), int(ti[r]), int(tj[r])
            g = m.gather(*trip)
            if g is not None:
                acc += m.store(*trip, g, t + r + 1)
        losses.append(acc)
        t += n
    return m.result(losses, t)


def bpr_pipelined(tu, ti, tj, P, Q, Bi=None, *, stride, loss=0, eta0=0.005, lambda_u=1e-4,
                  lambda_i=1e-4, lambda_j=1e-4, lambda_b=0.01, use_bias=True, eta_kind="fixed",
                  power_t=0.1, total_steps=-1.0, epochs=1, t0=0):
    """bpr_pf3_kernel's order.  Slot s of ``stride`` handles triples s, s + stride, ...; within a
    slot, triple q + 1 is gathered before triple q is computed and stored, so two consecutive
    triples of a slot that share a row see it one update stale and the later store overwrites
    the earlier one.  Slots are taken one after the other: the caller keeps them row-disjoint.
    Every launch (epoch) starts its own pipeline."""
    m = _BPR(P, Q, Bi, loss, eta0, lambda_u, lambda_i, lambda_j, lambda_b, use_bias, eta_kind,
             power_t, total_steps)
    n, t, losses = len(tu), int(t0), []
    trip = lambda r: (int(tu[r]), int(ti[r]), int(tj[r]))  # noqa: E731
    for _ in range(epochs):
        acc = 0.0
        for s in range(min(stride, n)):
            chain = list(range(s, n, stride))
            ga = m.gather(*trip(chain[0]))
            for pos, r in enumerate(chain):
                gb = m.gather(*trip(chain[pos + 1])) if pos + 1 < len(chain) else None
                if ga is not None:
                    acc += m.store(*trip(r), ga, t + r + 1)
                ga = gb
        losses.append(acc)
        t += n
    return m.result(losses, t)


# ------------------------------------------------------------------------------------ sampler
def _pcg(s: int):
    """One PCG-XSH-RR step: (32-bit output, next state)."""
    nxt = (s * PCG_MUL + PCG_INC) & M64
    xs = (((s >> 18) ^ s) >> 27) & 0xFFFFFFFF
    rot = s >> 59
    return ((xs >> rot) | (xs << ((-rot) & 31))) & 0xFFFFFFFF, nxt


def pcg_draw(seed: int, t: int, csr, n_items: int, max_tries: int = 16):
    """The triple drawn for stream position ``t`` (the model's running clock plus the row):
    ``(u, i, j, rejections)`` with j = -1 when all ``max_tries`` candidates were positives of u.
    ``csr`` = (ptr, items sorted per user, user of each pair), as ``BPRMF.build_csr`` returns."""
    ptr, items, pos_user = csr
    s = ((int(seed) << 32) ^ ((int(t) * GOLDEN) & M64)) & M64
    _, s = _pcg(s)
    o1, s = _pcg(s)
    o2, s = _pcg(s)
    pidx = ((o1 << 32) | o2) % len(items)
    u, i = int(pos_user[pidx]), int(items[pidx])
    mine = items[int(ptr[u]):int(ptr[u + 1])]
    rejected = 0
    for _ in range(max_tries):
        o, s = _pcg(s)
        j = o % n_items
        k = int(np.searchsorted(mine, j))
        if k < len(mine) and int(mine[k]) == j:
            rejected += 1
            continue
        return u, i, j, rejected
    return u, i, -1, rejected
