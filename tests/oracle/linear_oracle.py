"""Per-example numpy / float64 restatement of the online linear family (docs/compat.md).

Independent of csrc/kernels/linear_rules.h: written from the definitions
and the published algorithms, and used to pin the C++/HIP rules:

  Rosenblatt perceptron; Crammer et al. 2006 (PA, PA-I, PA-II, classification and regression);
  Dredze/Crammer/Pereira 2008 (CW, variance form, diagonal Σ); Crammer/Kulesza/Dredze 2009 (AROW);
  Wang/Zhao/Hoi 2012 (SCW-I, SCW-II); Duchi/Hazan/Singer 2011 + Xiao 2010 (AdaGrad, AdaGrad-RDA);
  Zeiler 2012 (AdaDelta); Tieleman & Hinton / Graves 2013 (RMSprop); Kingma & Ba 2015 (Adam),
  Reddi et al. 2018 (AMSGrad), Dozat 2016 (NAdam), Koushik & Hayashi 2016 (Eve),
  Baydin et al. 2018 (hypergradient Adam).

Two entry points:
  * ``train(algo, rows, y, dims, ...)``: the first four rules on rows of ones (kept as it was);
  * ``new_state`` / ``train_rows``: every rule, CSR rows with real values, the hyper-parameters of
    a ``LinParams`` (``hyper(P)``), the engines' row semantics (step counter carried in the
    state, row order / shard given as a list of row ids, features outside [0, dims) ignored).

Row semantics shared with the engines: the lanes of a wave gather a row's features in parallel,
so a row is "all sums first, then one update per feature"; features are distinct within a row.

Branch guard: ``st["guard"]`` holds, per kind, the smallest distance of a branching quantity
from its threshold over the run ("margin": row-level quantities such as a hinge margin;
"sign": |w| of a weight whose sign an L1 / elastic-net term reads).  A quantity that is exactly
zero because every weight it is made of is still zero is the same zero in fp32 and counts as safe.
"""
import math
from types import SimpleNamespace

import numpy as np

# ---------------------------------------------------------------------------- legacy entry


def train(algo, rows, y, dims, r=0.1, c=1.0, eta0=0.1, power_t=0.1, eps=1e-6):
    w = np.zeros(dims)
    cov = np.ones(dims)
    G = np.zeros(dims)
    t = 0
    for feats, yy in zip(rows, y):
        t += 1
        i = np.asarray(feats, dtype=np.int64)
        x = np.ones(len(i))
        p = float((w[i] * x).sum())
        if algo == "perceptron":
            if yy * p <= 0:
                w[i] += yy * x
        elif algo == "pa1":
            loss = max(0.0, 1 - yy * p)
            if loss > 0:
                eta = min(c, loss / float((x * x).sum()))
                w[i] += eta * yy * x
        elif algo == "arow":
            m = yy * p
            var = float((cov[i] * x * x).sum())
            if m < 1:
                beta = 1.0 / (var + r)
                alpha = (1 - m) * beta
                sx = cov[i] * x
                w[i] += alpha * yy * sx
                cov[i] -= beta * sx * sx
        elif algo == "adagrad_logloss":  # train_classifier -loss logloss -opt adagrad -reg no
            z = yy * p
            d = -yy / (1 + math.exp(z))
            g = d * x
            G[i] += g * g
            eta = eta0 / (t ** power_t)
            w[i] -= eta * g / (np.sqrt(G[i]) + eps)
        else:
            raise ValueError(algo)
    return w, cov


# ---------------------------------------------------------------------------- names <-> ABI ids
ALGO_NAMES = ["perceptron", "pa", "pa1", "pa2", "cw", "arow", "arowh", "scw", "scw2", "adagrad_rda",
              "logress", "pa1_regr", "pa2_regr", "pa1a_regr", "pa2a_regr", "arow_regr", "arowe_regr",
              "arowe2_regr", "adagrad_regr", "adadelta_regr", "general"]
LOSS_NAMES = ["hinge", "log", "squared_hinge", "modified_huber", "squared", "quantile",
              "epsilon_insensitive", "squared_epsilon_insensitive", "huber"]
OPT_NAMES = ["sgd", "momentum", "nesterov", "adagrad", "rmsprop", "rmsprop_graves", "adadelta", "adam",
             "nadam", "eve", "adam_hd"]
REG_NAMES = ["no", "l1", "l2", "elasticnet", "rda"]
ETA_NAMES = ["fixed", "simple", "inverse"]
COVAR = {"cw", "arow", "arowh", "scw", "scw2", "arow_regr", "arowe_regr", "arowe2_regr"}
MULTICLASS = {"perceptron", "pa", "pa1", "pa2", "cw", "arow", "arowh", "scw", "scw2"}

RS_T, RS_N, RS_MEAN, RS_M2, RS_EVE_D, RS_EVE_F = range(6)


def hyper(P):
    """Hyper-parameters of a ``LinParams`` (the float32 values, widened), with names for the ids."""
    H = SimpleNamespace(**{n.rstrip("_"): getattr(P, n) for n, _ in P._fields_})
    H.lam = getattr(P, "lambda_")
    H.algo, H.loss, H.opt = ALGO_NAMES[P.algo], LOSS_NAMES[P.loss], OPT_NAMES[P.opt]
    H.reg, H.eta = REG_NAMES[P.reg], ETA_NAMES[P.eta]
    return H


def new_state(dims, L=1, covar=False, init_covar=1.0):
    S = np.zeros((L, dims, 4))
    if covar:
        S[..., 1] = init_covar
    return {"S": S, "rs": np.zeros(8), "touched": np.zeros(dims, dtype=bool), "loss": 0.0,
            "guard": {"margin": math.inf, "sign": math.inf}, "early_flushes": 0}


def _guard(st, kind, d):
    d = abs(float(d))
    if d != 0.0 and d < st["guard"][kind]:       # an exact zero: see the module docstring
        st["guard"][kind] = d


# ---------------------------------------------------------------------------- losses
def loss_value(name, p, y, H):
    if name == "hinge":
        return max(0.0, 1.0 - y * p)
    if name == "log":
        return float(np.logaddexp(0.0, -y * p))
    if name == "squared_hinge":
        return max(0.0, 1.0 - y * p) ** 2
    if name == "modified_huber":
        z = y * p
        return 0.0 if z >= 1 else ((1 - z) ** 2 if z >= -1 else -4.0 * z)
    if name == "squared":
        return 0.5 * (p - y) ** 2
    if name == "quantile":
        e = y - p
        return H.quantile_tau * e if e > 0 else (H.quantile_tau - 1.0) * e
    if name == "epsilon_insensitive":
        return max(0.0, abs(y - p) - H.epsilon)
    if name == "squared_epsilon_insensitive":
        return max(0.0, abs(y - p) - H.epsilon) ** 2
    if name == "huber":
        r = abs(p - y)
        return 0.5 * r * r if r <= H.huber_c else H.huber_c * (r - 0.5 * H.huber_c)
    raise ValueError(name)


def loss_dloss(name, p, y, H):
    """d loss / d p."""
    if name == "hinge":
        return -y if y * p < 1 else 0.0
    if name == "log":
        return -y * 0.5 * (1.0 - math.tanh(0.5 * y * p))         # -y sigmoid(-yp)
    if name == "squared_hinge":
        return -2.0 * y * max(0.0, 1.0 - y * p)
    if name == "modified_huber":
        z = y * p
        return 0.0 if z >= 1 else (-2.0 * y * (1 - z) if z >= -1 else -4.0 * y)
    if name == "squared":
        return p - y
    if name == "quantile":
        return -H.quantile_tau if y > p else 1.0 - H.quantile_tau
    if name == "epsilon_insensitive":
        e = y - p
        return -np.sign(e) if abs(e) > H.epsilon else 0.0
    if name == "squared_epsilon_insensitive":
        e = y - p
        return -2.0 * np.sign(e) * max(0.0, abs(e) - H.epsilon)
    if name == "huber":
        r = p - y
        return r if abs(r) <= H.huber_c else H.huber_c * np.sign(r)
    raise ValueError(name)


def loss_kink_distance(name, p, y, H):
    """Distance of (p, y) from the nearest point where the loss changes its branch."""
    if name in ("hinge", "squared_hinge"):
        return abs(1.0 - y * p)
    if name == "modified_huber":
        return min(abs(1.0 - y * p), abs(1.0 + y * p))
    if name == "quantile":
        return abs(y - p)
    if name in ("epsilon_insensitive", "squared_epsilon_insensitive"):
        return abs(abs(y - p) - H.epsilon)
    if name == "huber":
        return abs(abs(y - p) - H.huber_c)
    return math.inf


# losses whose kink the branch guard watches (Huber's two branches meet with equal value and slope)
GUARDED_LOSSES = {"hinge", "squared_hinge", "modified_huber", "quantile", "epsilon_insensitive",
                  "squared_epsilon_insensitive"}


# ---------------------------------------------------------------------------- schedules
def eta_at(H, t):
    if H.eta == "fixed":
        return H.eta0
    if H.eta == "simple":
        return H.eta0 / (1.0 + t / H.total_steps) if H.total_steps > 0 else H.eta0
    return H.eta0 / max(t, 1.0) ** H.power_t


def _penalty_grad(H, w, st):
    if H.reg in ("l1", "elasticnet"):
        nz = np.abs(w[w != 0.0])
        if nz.size:
            _guard(st, "sign", nz.min())
    if H.reg == "l1":
        return H.lam * np.sign(w)
    if H.reg == "l2":
        return H.lam * w
    if H.reg == "elasticnet":
        return H.lam * (H.l1_ratio * np.sign(w) + (1.0 - H.l1_ratio) * w)
    return 0.0


def rda_weight(u, G, t, eta, lam):
    """AdaGrad-RDA closed form (Duchi et al. 2011 §1.3.1 with the l1 proximal of Xiao 2010):
    w = -sign(u) eta t / sqrt(G) [|u| / t - lam]_+ ."""
    shrink = np.maximum(np.abs(u) / t - lam, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = -np.sign(u) * eta * t * shrink / np.sqrt(G)
    return np.where(shrink > 0.0, w, 0.0)


def optimizer_step(H, C, g, t, eve_d, st):
    """One step of the general learner's optimizer on the feature block C [n, 4] = {w, s1, s2, s3}
    with the loss gradient g [n] (the regulariser's term is added here) at step t."""
    w, s1, s2, s3 = C[:, 0], C[:, 1], C[:, 2], C[:, 3]
    eta = eta_at(H, t)
    if H.opt == "adagrad" and H.reg == "rda":
        s1 += g                                     # u: sum of gradients
        s2 += g * g                                 # G: sum of squared gradients
        w[:] = rda_weight(s1, s2, t, eta, H.lam)
        return
    g = g + _penalty_grad(H, w, st)
    b1, b2, eps = H.beta1, H.beta2, H.eps
    if H.opt == "sgd":
        w -= eta * g
    elif H.opt == "momentum":                       # classical momentum, mu = beta1
        s1[:] = b1 * s1 + eta * g
        w -= s1
    elif H.opt == "nesterov":                       # pinned: Sutskever's look-ahead form
        v0 = s1.copy()
        s1[:] = b1 * v0 - eta * g
        w += -b1 * v0 + (1.0 + b1) * s1
    elif H.opt == "adagrad":
        s1 += g * g
        w -= eta * g / (np.sqrt(s1) + eps)
    elif H.opt == "rmsprop":
        s1[:] = H.decay * s1 + (1.0 - H.decay) * g * g
        w -= eta * g / (np.sqrt(s1) + eps)
    elif H.opt == "rmsprop_graves":                 # Graves 2013 eq. 38-45: n, g-bar, delta
        s1[:] = H.decay * s1 + (1.0 - H.decay) * g * g
        s2[:] = H.decay * s2 + (1.0 - H.decay) * g
        den = s1 - s2 * s2 + eps
        den = np.where(den > 0.0, den, eps)
        s3[:] = b1 * s3 - eta * H.alpha * g / np.sqrt(den)
        w += s3
    elif H.opt == "adadelta":
        s1[:] = H.rho * s1 + (1.0 - H.rho) * g * g
        dx = np.sqrt(s2 + eps) / np.sqrt(s1 + eps) * g
        s2[:] = H.rho * s2 + (1.0 - H.rho) * dx * dx
        w -= dx
    elif H.opt in ("adam", "eve", "adam_hd"):
        m0, v0 = s1.copy(), s2.copy()
        s1[:] = b1 * m0 + (1.0 - b1) * g
        s2[:] = b2 * v0 + (1.0 - b2) * g * g
        c1, c2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        vhat = s2
        alpha = H.alpha
        if H.opt == "adam" and H.amsgrad:
            s3[:] = np.maximum(s3, s2)
            vhat = s3
        if H.opt == "adam_hd":
            # pinned: per-coordinate alpha_i (s3), previous direction with step t-1's corrections
            s3[s3 == 0.0] = H.alpha
            if t > 1:
                u0 = (m0 / (1.0 - b1 ** (t - 1))) / (np.sqrt(v0 / (1.0 - b2 ** (t - 1))) + eps)
                s3 += H.beta_hd * g * u0
            alpha = s3
        lr = eta * alpha * math.sqrt(c2) / c1
        if H.opt == "eve":
            lr = lr / (eve_d if eve_d > 0 else 1.0)
        w -= lr * s1 / (np.sqrt(vhat) + eps)
    elif H.opt == "nadam":
        s1[:] = b1 * s1 + (1.0 - b1) * g
        s2[:] = b2 * s2 + (1.0 - b2) * g * g
        mhat = b1 * s1 / (1.0 - b1 ** (t + 1)) + (1.0 - b1) * g / (1.0 - b1 ** t)
        vhat = s2 / (1.0 - b2 ** t)
        w -= eta * H.alpha * mhat / (np.sqrt(vhat) + eps)
    else:
        raise ValueError(H.opt)


# ---------------------------------------------------------------------------- closed forms
def pa_step(kind, loss, sq, C):
    """Crammer et al. 2006: tau for PA / PA-I / PA-II given the suffered loss and ||x||^2."""
    if kind == "pa":
        return loss / sq
    if kind == "pa1":
        return min(C, loss / sq)
    return loss / (sq + 1.0 / (2.0 * C))


def cw_alpha(m, v, phi):
    """Dredze et al. 2008 (variance form): the larger root of
    2 phi v^2 a^2 + v (1 + 2 phi m) a + (m - phi v) = 0, clipped at 0."""
    if v == 0.0:
        return 0.0
    b = 1.0 + 2.0 * phi * m
    disc = b * b - 8.0 * phi * (m - phi * v)
    return max(0.0, (-b + math.sqrt(max(disc, 0.0))) / (4.0 * phi * v))


def scw_alpha_beta(kind, m, v, phi, C):
    """Wang et al. 2012, Propositions 1 and 2."""
    p2 = phi * phi
    if kind == "scw":
        psi, zeta = 1.0 + p2 / 2.0, 1.0 + p2
        a = (-m * psi + math.sqrt(max(m * m * p2 * p2 / 4.0 + v * p2 * zeta, 0.0))) / (v * zeta)
        a = min(C, max(0.0, a))
    else:
        n = v + 1.0 / (2.0 * C)
        gamma = phi * math.sqrt(p2 * m * m * v * v + 4.0 * n * v * (n + v * p2))
        a = max(0.0, (-(2.0 * m * n + p2 * m * v) + gamma) / (2.0 * (n * n + n * v * p2)))
    u = 0.25 * (-a * v * phi + math.sqrt(a * a * v * v * p2 + 4.0 * v)) ** 2
    beta = a * phi / (math.sqrt(u) + v * a * phi)
    return a, beta


def _welford(rs, y):
    """Running sample standard deviation of the targets (Welford), this target included."""
    n = rs[RS_N] + 1.0
    d = y - rs[RS_MEAN]
    rs[RS_MEAN] += d / n
    rs[RS_M2] += d * (y - rs[RS_MEAN])
    rs[RS_N] = n
    return math.sqrt(rs[RS_M2] / (n - 1.0)) if n > 1 else 0.0


def _conf_update(kind, C, a, b, x):
    """Mean / diagonal covariance update: CW adds to the precision, AROW / SCW subtract."""
    w, s = C[:, 0], C[:, 1]
    w += a * s * x
    if kind == "cw":
        s[:] = 1.0 / (1.0 / s + b * x * x)
    else:
        s -= b * s * s * x * x


# ---------------------------------------------------------------------------- the learners
def _binary_row(H, st, C, x, y, t):
    """Row rule + feature update of a binary / regression learner on the row's block C [n, 4]."""
    rs = st["rs"]
    a = H.algo
    p = float(C[:, 0] @ x)
    sq = float(x @ x)
    v = float(C[:, 1] @ (x * x)) if a in COVAR else 0.0
    if a == "perceptron":
        m = y * p
        _guard(st, "margin", m)
        st["loss"] += 1.0 if m <= 0 else 0.0
        if m <= 0:
            C[:, 0] += y * x
    elif a in ("pa", "pa1", "pa2"):
        l = 1.0 - y * p
        st["loss"] += max(l, 0.0)
        if l > 0 and sq > 0:
            C[:, 0] += pa_step(a, l, sq, H.c) * y * x
    elif a == "cw":
        m = y * p
        _guard(st, "margin", m)                    # the 0/1 loss count
        st["loss"] += 1.0 if m < 0 else 0.0
        al = cw_alpha(m, v, H.phi)
        if al > 0:
            _conf_update("cw", C, al * y, 2.0 * al * H.phi, x)
    elif a in ("arow", "arowh"):
        l = (H.c if a == "arowh" else 1.0) - y * p
        _guard(st, "margin", l)                    # the covariance shrinks by a finite step
        st["loss"] += max(l, 0.0)
        if l > 0:
            beta = 1.0 / (v + H.r)
            _conf_update("arow", C, l * beta * y, beta, x)
    elif a in ("scw", "scw2"):
        m = y * p
        l = H.phi * math.sqrt(v) - m
        st["loss"] += max(l, 0.0)
        if l > 0 and v > 0:
            al, beta = scw_alpha_beta(a, m, v, H.phi, H.c)
            if al > 0:
                _conf_update("scw", C, al * y, beta, x)
    elif a == "adagrad_rda":
        l = 1.0 - y * p
        _guard(st, "margin", l)
        st["loss"] += max(l, 0.0)
        if l > 0:
            g = -y * x
            C[:, 1] += g
            C[:, 2] += g * g
            C[:, 0] = rda_weight(C[:, 1], C[:, 2], t, H.eta0, H.lam)
    elif a in ("logress", "adagrad_regr", "adadelta_regr"):
        s = 0.5 * (1.0 + math.tanh(0.5 * p))
        clamp = -math.log(1e-7)                     # cross-entropy with both logs clamped
        st["loss"] += (y * min(float(np.logaddexp(0.0, -p)), clamp)
                       + (1.0 - y) * min(float(np.logaddexp(0.0, p)), clamp))
        g = (y - s) * x                             # ascent direction of the log-likelihood
        if a == "logress":
            C[:, 0] += eta_at(H, t) * g
        elif a == "adagrad_regr":
            C[:, 1] += g * g
            C[:, 0] += H.eta0 * g / np.sqrt(H.eps + C[:, 1])
        else:
            C[:, 1] = H.rho * C[:, 1] + (1.0 - H.rho) * g * g
            dx = np.sqrt(C[:, 2] + H.eps) / np.sqrt(C[:, 1] + H.eps) * g
            C[:, 2] = H.rho * C[:, 2] + (1.0 - H.rho) * dx * dx
            C[:, 0] += dx
    elif a in ("pa1_regr", "pa2_regr", "pa1a_regr", "pa2a_regr"):
        eps = H.epsilon * (_welford(rs, y) if a in ("pa1a_regr", "pa2a_regr") else 1.0)
        e = y - p
        l = abs(e) - eps
        st["loss"] += max(l, 0.0)
        if l > 0 and sq > 0:
            C[:, 0] += np.sign(e) * pa_step("pa1" if a.startswith("pa1") else "pa2", l, sq, H.c) * x
    elif a in ("arow_regr", "arowe_regr", "arowe2_regr"):
        e = y - p
        if a == "arow_regr":
            l = e
        else:
            eps = H.epsilon * (_welford(rs, y) if a == "arowe2_regr" else 1.0)
            _guard(st, "margin", abs(e) - eps)     # the covariance shrinks by a finite step
            l = np.sign(e) * max(0.0, abs(e) - eps)
        st["loss"] += abs(l)
        if l != 0:
            beta = 1.0 / (v + H.r)
            _conf_update("arow", C, l * beta, beta, x)
    else:
        raise ValueError(a)


# Eve's smoothing constants as the engines hold them (float32): 1 - 0.999f differs from 0.001f by
# 1.3e-5 of itself, and the running d settles at their ratio
_EVE_KEEP, _EVE_TAKE = float(np.float32(0.999)), float(np.float32(0.001))


def _general_row(H, st, p, y):
    """Loss, its derivative and Eve's feedback for one row of the general learner."""
    rs = st["rs"]
    if H.loss in GUARDED_LOSSES:
        _guard(st, "margin", loss_kink_distance(H.loss, p, y, H))
    l = loss_value(H.loss, p, y, H)
    st["loss"] += l
    if H.opt == "eve":
        # Koushik & Hayashi 2016 on the per-row loss; pinned: clip [0.1, 10], smoothing 0.999,
        # f + 1e-8, d = 1 on the first row
        f, f0 = l + 1e-8, rs[RS_EVE_F]
        if f0 > 0:
            r = min(max(abs(f - f0) / min(f, f0), 0.1), 10.0)
            rs[RS_EVE_D] = _EVE_KEEP * rs[RS_EVE_D] + _EVE_TAKE * r
        else:
            rs[RS_EVE_D] = 1.0
        rs[RS_EVE_F] = f
    return loss_dloss(H.loss, p, y, H)


def _multiclass_row(H, st, S, i, x, y):
    L = S.shape[0]
    act = int(y)
    a = H.algo
    scores = S[:, i, 0] @ x
    var = S[:, i, 1] @ (x * x)
    if L < 2 or act < 0 or act >= L:
        return
    wrong = [l for l in range(L) if l != act]
    miss = max(wrong, key=lambda l: (scores[l], -l))           # the first of equal scores
    for l in wrong:
        if l != miss:
            _guard(st, "margin", scores[miss] - scores[l])
    m = float(scores[act] - scores[miss])
    v = float(var[act] + var[miss])
    sq = float(x @ x)
    al, b = 0.0, 0.0
    if a == "perceptron":
        _guard(st, "margin", m)
        st["loss"] += 1.0 if m <= 0 else 0.0
        al = 1.0 if m <= 0 else 0.0
    elif a in ("pa", "pa1", "pa2"):
        l = 1.0 - m
        st["loss"] += max(l, 0.0)
        if l > 0 and sq > 0:
            al = pa_step(a, l, 2.0 * sq, H.c)                  # ||x_act - x_miss||^2 = 2 ||x||^2
    elif a == "cw":
        _guard(st, "margin", m)
        st["loss"] += 1.0 if m < 0 else 0.0
        al = cw_alpha(m, v, H.phi)
        b = 2.0 * al * H.phi
    elif a in ("arow", "arowh"):
        l = (H.c if a == "arowh" else 1.0) - m
        _guard(st, "margin", l)
        st["loss"] += max(l, 0.0)
        if l > 0:
            b = 1.0 / (v + H.r)
            al = l * b
    elif a in ("scw", "scw2"):
        l = H.phi * math.sqrt(v) - m
        st["loss"] += max(l, 0.0)
        if l > 0 and v > 0:
            al, b = scw_alpha_beta(a, m, v, H.phi, H.c)
    else:
        raise ValueError(a)
    if al <= 0:
        return
    for l, sgn in ((act, 1.0), (miss, -1.0)):
        C = S[l, i]
        if a in COVAR:
            _conf_update("cw" if a == "cw" else "arow", C, sgn * al, b, x)
        else:
            C[:, 0] += sgn * al * x
        S[l, i] = C


def train_rows(H, st, dims, indptr, idx, val, y, rows, mini_batch=1, steps=None, touched_cap=None):
    """Run the learner over the row ids ``rows`` in that order (a shard, a permutation, ...).

    The step of a row is the state's counter + 1 (carried across calls), or ``steps[j]`` for the
    engines that number the rows themselves (t0 + q + 1).  ``mini_batch`` M > 1 (general learner):
    M rows are scored against the same weights, then every feature they touched takes one
    optimizer step with the mean gradient at the step of the batch's last row; a short tail is
    divided by its own size.  ``touched_cap``: the replica kernel's batch list holds that many
    features and the batch is cut short (and divided by the rows it has) once fewer than 256
    entries are free."""
    S, rs = st["S"], st["rs"]
    L = S.shape[0]
    rows = list(rows)
    minib = mini_batch > 1 and H.algo == "general" and L == 1
    acc = np.zeros(dims)
    in_acc = np.zeros(dims, dtype=bool)
    in_batch = 0
    for j, row in enumerate(rows):
        k0, k1 = int(indptr[row]), int(indptr[row + 1])
        i = np.asarray(idx[k0:k1], dtype=np.int64)
        x = np.ones(k1 - k0) if val is None else np.asarray(val[k0:k1], dtype=np.float64)
        ok = (i >= 0) & (i < dims)
        i, x = i[ok], x[ok]
        t = float(steps[j]) if steps is not None else rs[RS_T] + 1.0
        rs[RS_T] = t
        st["touched"][i] = True
        yy = float(y[row])
        if L > 1:
            _multiclass_row(H, st, S, i, x, yy)
            continue
        if H.algo != "general":
            C = S[0, i]
            _binary_row(H, st, C, x, yy, t)
            S[0, i] = C
            continue
        d = _general_row(H, st, float(S[0, i, 0] @ x), yy)
        if not minib:
            if d != 0.0:
                C = S[0, i]
                optimizer_step(H, C, d * x, t, rs[RS_EVE_D], st)
                S[0, i] = C
            continue
        if d != 0.0:
            acc[i] += d * x
            in_acc[i] = True
        in_batch += 1
        full = touched_cap is not None and int(in_acc.sum()) + 256 > touched_cap
        if in_batch == mini_batch or j + 1 == len(rows) or full:
            st["early_flushes"] += int(full and in_batch < mini_batch and j + 1 < len(rows))
            f = np.nonzero(in_acc)[0]
            C = S[0, f]
            optimizer_step(H, C, acc[f] / in_batch, t, rs[RS_EVE_D], st)
            S[0, f] = C
            acc[f] = 0.0
            in_acc[f] = False
            in_batch = 0
    return st
