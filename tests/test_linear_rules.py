"""Every rule and every kernel path of the online linear family against the fp64 oracle
(tests/oracle/linear_oracle.py), on rows that are wider than a wave, carry real values, hold
out-of-range indices and can be empty.

Independent and pinned parts of the oracle
------------------------------------------
Independently derived (from the papers named in the oracle's docstring and SURVEY.md C3-C8): the
nine losses and their derivatives (finite-difference test below), the PA / PA-I / PA-II steps
(constraint test), the CW and SCW closed forms (constraint tests), the AROW update (monotone
covariance test), AdaGrad, AdaGrad-RDA's closed form, RMSprop, AdaDelta, momentum, Adam, AMSGrad,
NAdam's bias corrections, the regularisers' gradients, the three eta schedules, Welford's running
deviation, the mini-batch rule and the multiclass "actual vs best wrong label" reduction.
Pinned to the engine where no definition decides (docs/compat.md):
  * Eve: relative loss change clipped to [0.1, 10], smoothed by 0.999, f + 1e-8, d = 1 on the
    first row, tracked on the per-row loss;
  * AdamHD: one step size per coordinate, previous direction taken with step t-1's bias
    corrections, alpha_i initialised at the first update;
  * Nesterov: w += -mu v_prev + (1 + mu) v with v = mu v_prev - eta g;
  * RMSprop-Graves: the denominator n - gbar^2 + eps replaced by eps where it is not positive;
  * logistic regressors: loss clamped at log(1e-7), `train_adagrad_regr` divides by
    sqrt(eps + G) with eps 1;
  * multiclass PA divides by 2 ||x||^2; the first of equal best wrong labels is taken;
  * the replica kernel's mini-batch list: a batch is cut short once fewer than 256 of its
    ``touched_cap`` entries are free and divided by the rows it has (the CPU engine has no list
    and never cuts; the oracle takes the cap as an argument).

Tolerance (measured, CPU engine vs oracle, err = max|S - S_ref| / max(1, max|S_ref|))
-------------------------------------------------------------------------------------
Worst value per rule family (``MEASURED`` below): perceptron / PA / AdaGrad-RDA 3.8e-7, CW / AROW /
SCW 4.2e-7, logistic regressors 4.3e-7, PA and AROW regression 5.5e-7, multiclass 4.6e-7, general
learner defaults 4.3e-7, optimizers x logloss 5.5e-7, AdamHD 1.15e-6 (its step sizes alpha_i:
increments of ~1e-8 added to 1.0 in fp32), losses 5.7e-7, regularisers 6.6e-7, eta schedules 1.8e-7,
mini-batch 2.8e-7.  ``BOUND`` = 32 x the largest = 3.68e-5, used by every comparison of this module
on the CPU and on the GPU (the factor covers the GPU's 64-lane tree order of the row sums and the
float atomics of the mini-batch engine).  No rule needs 1e-5.

Branch guard
------------
A rule with a discontinuous branch may legitimately differ when fp32 and fp64 fall on different
sides.  The oracle reports the smallest distance of such a quantity from its threshold; every
case asserts it is >= ``GUARD`` (a condition on the fixture: the seed was chosen for it).

Out of scope: the shared kernel's hot-feature paths (pre-aggregated sums, owner mode: not
sequential by design, covered by the logloss-parity tests of tests/test_linear.py), multi-wave
Hogwild behaviour, the multi-GPU mix.
"""
import functools
import math
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from hivemall_amd.models import linear as L
from hivemall_amd.ops import linear as LO
from tests.oracle import linear_oracle as O

SEED = 7
# label-noise stream per (dims, task), chosen on the CPU so that every case meets the branch guard
LABEL_SEEDS = {(300, "multiclass"): 1}
N_ROWS = 400
DIMS = 300
WIDTHS = (0, 1, 2, 63, 64, 65, 130)
GUARD = 1e-4
# worst CPU-engine error per rule family on this fixture (two passes of 400 rows; the larger of the
# state, replica-scalar and loss errors).  AdamHD's is on its step sizes alpha_i = 1 + sum of
# 1e-6 g u: increments of ~1e-8 added to 1.0 in fp32, whose half-ulp is 6e-8.  No rule needs 1e-5.
MEASURED = {
    "perceptron / PA / AdaGrad-RDA": 3.82e-07,
    "CW / AROW / SCW": 4.22e-07,
    "logistic regressors": 4.32e-07,
    "PA regression": 5.50e-07,
    "AROW regression": 5.50e-07,
    "multiclass (9 rules)": 4.55e-07,
    "general learner defaults": 4.31e-07,
    "optimizers x logloss (all but AdamHD), AMSGrad": 5.47e-07,
    "AdamHD": 1.15e-06,
    "losses x SGD / Adam": 5.66e-07,
    "regularisers x SGD / AdaGrad": 6.64e-07,
    "eta schedules": 1.82e-07,
    "mini-batch 7": 2.79e-07,
}
BOUND = 32 * max(MEASURED.values())                 # 3.68e-5


# ---------------------------------------------------------------------------- fixture
@dataclass
class Fixture:
    dims: int
    indptr: torch.Tensor
    idx: torch.Tensor
    val: torch.Tensor
    y: dict

    @property
    def n(self):
        return self.indptr.numel() - 1

    def to(self, dev):
        return Fixture(self.dims, self.indptr.to(dev), self.idx.to(dev), self.val.to(dev),
                       {k: v.to(dev) for k, v in self.y.items()})


def make_fixture(dims, n=N_ROWS, widths=WIDTHS, bad=True):
    """~400 rows of distinct features, widths from WIDTHS (the narrow ones rarer: the score of a
    one-feature row is small, which crowds the branch thresholds at zero), values uniform in
    [-1, 1], a few indices -1 and dims + 3; labels from three hidden linear models plus noise."""
    rng = np.random.default_rng([SEED, dims])
    wd = rng.choice(widths, size=n, p=[0.04, 0.04, 0.04, 0.2, 0.24, 0.24, 0.2])
    wd[:len(widths)] = widths                       # every width at least once
    truth = rng.normal(size=(3, dims)) / 4.0
    # at most 300 features are in use, spread over [0, dims) with both ends: rows of a wide model
    # then share features as those of the dims-300 one do (rows that share two or three features
    # start with near-equal label scores, which no seed keeps apart)
    active = np.sort(rng.choice(dims, size=min(dims, 300), replace=False))
    active[0], active[-1] = 0, dims - 1
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(wd)
    idx = np.zeros(indptr[-1], dtype=np.int32)
    val = rng.uniform(-1.0, 1.0, size=indptr[-1]).astype(np.float32)
    score = np.zeros((n, 3))
    for q in range(n):
        f = active[rng.choice(active.size, size=wd[q], replace=False)]
        idx[indptr[q]:indptr[q + 1]] = f
        score[q] = truth[:, f] @ val[indptr[q]:indptr[q + 1]]
    if bad:                                         # a few indices outside [0, dims)
        wide = np.nonzero(wd >= 2)[0]
        for j, q in enumerate(wide[:8]):
            idx[indptr[q] + (j % wd[q])] = -1 if j % 2 == 0 else dims + 3
    def noise(task, shape):
        return np.random.default_rng([SEED, dims, LABEL_SEEDS.get((dims, task), 0)]).normal(size=shape)

    y = {"binary": np.where(score[:, 0] + 0.3 * noise("binary", n) > 0, 1.0, -1.0),
         "regression": 4.0 * score[:, 0] + 2.0 * noise("regression", n),
         "multiclass": np.argmax(score + 0.3 * noise("multiclass", (n, 3)), axis=1).astype(np.float64)}
    y["logistic"] = (y["binary"] > 0).astype(np.float64)
    return Fixture(dims, torch.from_numpy(indptr), torch.from_numpy(idx), torch.from_numpy(val),
                   {k: torch.from_numpy(v.astype(np.float32)) for k, v in y.items()})


@functools.lru_cache(maxsize=None)
def fixture(dims):
    return make_fixture(dims)


_PERM = np.random.default_rng(11).permutation(N_ROWS).astype(np.int32)


@functools.lru_cache(maxsize=None)
def shuffled(dims):
    """The same rows stored in another order: row q of ``fixture(dims)`` sits at ``_PERM[q]``, so a
    pass with ``order = _PERM`` walks the fixture's rows 0, 1, 2, ... and has the same reference."""
    fx = fixture(dims)
    ip = fx.indptr.numpy()
    inv = np.argsort(_PERM)                         # stored position -> fixture row
    cut = np.concatenate([np.arange(ip[q], ip[q + 1]) for q in inv]).astype(np.int64)
    nip = np.concatenate([[0], np.cumsum(np.diff(ip)[inv])]).astype(np.int64)
    return Fixture(dims, torch.from_numpy(nip), fx.idx[cut].contiguous(), fx.val[cut].contiguous(),
                   {k: v[inv].contiguous() for k, v in fx.y.items()})


@functools.lru_cache(maxsize=None)
def three_rows(dims):
    """Rows 3, 5 and 6 of the fixture alone: 63, 65 and 130 non-zeros."""
    fx = fixture(dims)
    ip = fx.indptr.numpy()
    rows3 = [3, 5, 6]
    assert [int(ip[q + 1] - ip[q]) for q in rows3] == [63, 65, 130]
    cut = np.concatenate([np.arange(ip[q], ip[q + 1]) for q in rows3])
    return Fixture(dims, torch.from_numpy(np.concatenate([[0], np.cumsum([ip[q + 1] - ip[q] for q in rows3])])),
                   fx.idx[cut].contiguous(), fx.val[cut].contiguous(),
                   {k: v[rows3].contiguous() for k, v in fx.y.items()})


# ---------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    id: str
    name: str
    opts: str = ""
    mb: int = 1
    w0: float = 0.0       # warm start: weight +w0 on even features, -w0 on odd ones

    @property
    def cls(self):
        return L.LEARNERS[self.name]

    @property
    def task(self):
        t = self.cls.TASK
        if t == "regression" and self.cls.ALGO in ("logress", "adagrad_regr", "adadelta_regr"):
            return "logistic"
        return t

    @property
    def labels(self):
        return 3 if self.task == "multiclass" else 1

    @property
    def covar(self):
        return self.cls.ALGO in LO.COVAR_ALGOS

    @property
    def general(self):
        return self.cls.ALGO == "general"

    def start(self, dims):
        return self.w0 * np.where(np.arange(dims) % 2 == 0, 1.0, -1.0)

    def learner(self, dims):
        m = self.cls(f"{self.opts} -dims {dims}", device="cpu")
        m.P.n_labels = self.labels
        return m


CLS_LOSSES = ["hinge", "logloss", "squared_hinge", "modified_huber"]
REG_LOSSES = ["squared", "quantile", "epsilon_insensitive", "squared_epsilon_insensitive", "huber"]
OPTS = ["sgd", "momentum", "nesterov", "adagrad", "rmsprop", "rmspropgraves", "adadelta", "adam", "nadam",
        "eve", "adam_hd"]
_ETA0 = {"sgd": 0.05, "momentum": 0.01, "nesterov": 0.01, "adagrad": 0.1, "rmsprop": 0.01,
         "rmspropgraves": 0.001, "adadelta": 0.1, "adam": 0.01, "nadam": 0.01, "eve": 0.01, "adam_hd": 0.01}


def _general_cases():
    out = []
    for o in OPTS:
        out.append(Case(f"opt-{o}", "train_classifier", f"-loss logloss -opt {o} -reg no -eta0 {_ETA0[o]}"))
    for l in CLS_LOSSES + REG_LOSSES:
        name = "train_classifier" if l in CLS_LOSSES else "train_regressor"
        extra = " -quantile_tau 0.3" if l == "quantile" else (" -huber_c 0.5" if l == "huber" else "")
        for o in ("sgd", "adam"):
            out.append(Case(f"loss-{l}-{o}", name, f"-loss {l} -opt {o} -reg no -eta0 {_ETA0[o]}{extra}"))
    for r in ("no", "l1", "l2", "elasticnet", "rda"):
        for o in ("sgd", "adagrad"):
            # sgn(w) of L1 / elastic net: from a zero start a case's ~37,000 feature updates always
            # meet weights within GUARD of zero (smallest |w| 4e-7 .. 8e-6 on the seeds tried), so
            # these cases start at +-0.25 and keep every weight away from it (both signs occur)
            out.append(Case(f"reg-{r}-{o}", "train_classifier",
                            f"-loss logloss -opt {o} -reg {r} -lambda 0.01 -l1_ratio 0.3 "
                            f"-eta0 {0.005 if o == 'sgd' else 0.01}",
                            w0=0.25 if r in ("l1", "elasticnet") else 0.0))
    out.append(Case("eta-fixed", "train_classifier", "-loss logloss -opt sgd -reg no -eta fixed -eta0 0.02"))
    out.append(Case("eta-simple", "train_classifier", "-loss logloss -opt sgd -reg no -eta simple -t 800 -eta0 0.05"))
    out.append(Case("eta-inverse", "train_classifier",
                    "-loss logloss -opt sgd -reg no -eta inverse -power_t 0.25 -eta0 0.05"))
    out.append(Case("amsgrad", "train_classifier", "-loss logloss -opt adam -reg no -amsgrad -eta0 0.01"))
    out.append(Case("mb7-sgd", "train_classifier", "-loss logloss -opt sgd -reg no -eta0 0.05", mb=7))
    out.append(Case("mb7-adam-l2", "train_classifier", "-loss logloss -opt adam -reg l2 -eta0 0.01", mb=7))
    out.append(Case("mb7-default", "train_classifier", "", mb=7))
    return out


CASES = [Case(n, n) for n in L.LEARNERS] + _general_cases()
BY_ID = {c.id: c for c in CASES}
NONCOV = [c for c in CASES if not c.covar and c.labels == 1 and c.mb == 1]


def _ids(cases):
    return [c.id for c in cases]


# ---------------------------------------------------------------------------- oracle runs (cached)
_ORACLE = {}


def oracle_run(case, fx, row_lists, steps=None, cap=None, key=None):
    """Oracle over ``row_lists`` (one list of row ids per pass) from a fresh state."""
    k = (case.id, fx.dims, key, cap)
    if key is not None and k in _ORACLE:
        return _ORACLE[k]
    m = case.learner(fx.dims)
    H = O.hyper(m.P)
    st = O.new_state(fx.dims, case.labels, case.covar, m.P.init_covar)
    st["S"][..., 0] = case.start(fx.dims)
    ip, ix, vv = fx.indptr.cpu().numpy(), fx.idx.cpu().numpy(), fx.val.cpu().numpy()
    y = fx.y[case.task].cpu().numpy()
    for j, rows in enumerate(row_lists):
        O.train_rows(H, st, fx.dims, ip, ix, vv, y, rows, mini_batch=case.mb,
                     steps=None if steps is None else steps[j], touched_cap=cap)
    if key is not None:
        _ORACLE[k] = st
    return st


def two_passes(case, fx, cap=None):
    n = fx.n
    return oracle_run(case, fx, [range(n), range(n)], cap=cap, key="2p")


def rel_err(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - ref).max() / max(1.0, np.abs(ref).max()))


def errors(S, touched, rs, loss, ref):
    """S [L, dims, 4], touched [dims], rs [8] or None, loss float vs an oracle state."""
    e = {"S": rel_err(S, ref["S"]), "loss": rel_err([loss], [ref["loss"]]),
         "touched": int((np.asarray(touched).astype(bool) != ref["touched"]).sum())}
    if rs is not None:                              # each scalar on its own scale
        e["rs"] = max(rel_err([a], [b]) for a, b in zip(np.asarray(rs)[:6], ref["rs"][:6]))
    return e


def check(S, touched, rs, loss, ref, what=""):
    e = errors(S, touched, rs, loss, ref)
    print(what, e)
    assert e["touched"] == 0, (what, e)
    assert e["S"] <= BOUND and e["loss"] <= BOUND and e.get("rs", 0.0) <= BOUND, (what, e)
    return e


def guard_ok(ref):
    g = ref["guard"]
    assert g["margin"] >= GUARD and g["sign"] >= GUARD, g


def replica_run(case, fx, dev, R=1, order=None, passes=2):
    """The replica engine (CPU engine or linear_train_kernel) over ``passes`` passes."""
    m = case.learner(fx.dims)
    st = LO.new_state(R, case.labels, fx.dims, dev, case.covar, m.P.init_covar, case.mb)
    st.S[..., 0] = torch.from_numpy(case.start(fx.dims)).to(st.S)
    f = fx.to(dev)
    od = None if order is None else torch.as_tensor(order, dtype=torch.int32, device=dev)
    loss = torch.zeros(R, dtype=torch.float64)
    for _ in range(passes):
        loss += LO.train_pass(st, m.P, f.indptr, f.idx, f.val, f.y[case.task], od, case.mb).cpu()
    return st, loss.numpy()


# ---------------------------------------------------------------------------- oracle properties (CPU)
_H = O.hyper(L.TrainRegressor("-loss huber -huber_c 0.7 -quantile_tau 0.3 -epsilon 0.2", device="cpu").P)


@pytest.mark.parametrize("loss", O.LOSS_NAMES)
def test_oracle_dloss_is_the_derivative_of_loss(loss):
    rng = np.random.default_rng(0)
    seen = 0
    for _ in range(400):
        p = rng.uniform(-3, 3)
        y = rng.choice([-1.0, 1.0]) if loss in O.LOSS_NAMES[:4] else rng.uniform(-2, 2)
        if O.loss_kink_distance(loss, p, y, _H) < 1e-3:
            continue
        h = 1e-6
        fd = (O.loss_value(loss, p + h, y, _H) - O.loss_value(loss, p - h, y, _H)) / (2 * h)
        assert abs(fd - O.loss_dloss(loss, p, y, _H)) < 1e-7 * max(1.0, abs(fd)), (loss, p, y)
        seen += 1
    assert seen > 300


@pytest.mark.parametrize("name", ["train_pa", "train_pa1", "train_pa2"])
def test_oracle_pa_step_meets_its_constraint(name):
    """PA: the hinge loss of the row is 0 after the step; PA-I: the same unless clipped at C, and
    then the step is exactly C; PA-II: w moves by l / (|x|^2 + 1/2C), so the loss that remains is
    l / (1 + 2C|x|^2)."""
    fx = fixture(DIMS)
    c = BY_ID[name]
    H = O.hyper(c.learner(DIMS).P)
    H.c = 0.05
    ip, ix, vv, y = (fx.indptr.numpy(), fx.idx.numpy(), fx.val.numpy(), fx.y["binary"].numpy().astype(np.float64))
    st = O.new_state(DIMS)
    clipped = free = 0
    for q in range(fx.n):
        i = ix[ip[q]:ip[q + 1]].astype(np.int64)
        ok = (i >= 0) & (i < DIMS)
        i, x = i[ok], vv[ip[q]:ip[q + 1]][ok].astype(np.float64)
        before = st["S"][0, i, 0].copy()
        l0 = max(0.0, 1 - y[q] * float(before @ x))
        O.train_rows(H, st, DIMS, ip, ix, vv, y, [q])
        after = st["S"][0, i, 0]
        l1 = max(0.0, 1 - y[q] * float(after @ x))
        if l0 == 0 or x.size == 0:
            assert np.array_equal(before, after)
            continue
        sq = float(x @ x)
        tau = float(np.abs(after - before).max() / np.abs(x).max())
        if name == "train_pa":
            assert l1 < 1e-12
        elif name == "train_pa1":
            if l0 / sq > H.c:
                assert abs(tau - H.c) < 1e-12 and l1 > 0
                clipped += 1
            else:
                assert l1 < 1e-12
                free += 1
        else:
            assert abs(l1 - l0 / (1 + 2 * H.c * sq)) < 1e-12
    if name == "train_pa1":
        assert clipped > 10 and free > 10


def test_oracle_cw_scw_closed_forms_meet_their_constraints():
    """CW: alpha solves 2 phi v^2 a^2 + v (1 + 2 phi m) a + (m - phi v) = 0, i.e. the updated
    margin equals phi x the updated variance.  SCW-I (unclipped): updated margin = phi x updated
    deviation.  SCW-II: the loss left after the step is alpha / 2C (its squared slack)."""
    rng = np.random.default_rng(3)
    n = 0
    for _ in range(3000):
        m, v, phi, C = rng.uniform(-3, 3), rng.uniform(0.01, 5), rng.uniform(0.1, 2), rng.uniform(0.1, 10)
        a = O.cw_alpha(m, v, phi)
        if a > 0:
            assert abs(2 * phi * v * v * a * a + v * (1 + 2 * phi * m) * a + (m - phi * v)) < 1e-10
            assert abs((m + a * v) - phi * v / (1 + 2 * a * phi * v)) < 1e-10
            n += 1
        else:
            assert m - phi * v >= 0
        a, b = O.scw_alpha_beta("scw", m, v, phi, 1e9)
        if a > 0:
            assert abs((m + a * v) - phi * math.sqrt(v - b * v * v)) < 1e-10
        a1, _ = O.scw_alpha_beta("scw", m, v, phi, C)
        assert a1 == min(a, C)
        a, b = O.scw_alpha_beta("scw2", m, v, phi, C)
        if a > 0:
            assert abs(phi * math.sqrt(v - b * v * v) - (m + a * v) - a / (2 * C)) < 1e-10
    assert n > 500


@pytest.mark.parametrize("name", ["train_arow", "train_arowh", "train_arow_regr", "train_multiclass_arow"])
def test_oracle_arow_covariance_stays_positive_and_never_grows(name):
    fx = fixture(DIMS)
    c = BY_ID[name]
    H = O.hyper(c.learner(DIMS).P)
    st = O.new_state(DIMS, c.labels, True, 1.0)
    ip, ix, vv, y = (fx.indptr.numpy(), fx.idx.numpy(), fx.val.numpy(), fx.y[c.task].numpy())
    prev = st["S"][..., 1].copy()
    for q in range(fx.n):
        O.train_rows(H, st, DIMS, ip, ix, vv, y, [q])
        cur = st["S"][..., 1]
        assert (cur > 0).all() and (cur <= prev).all()
        prev = cur.copy()
    assert (prev < 1.0).any()


@pytest.mark.parametrize("table", ["LEARNERS", "LOSSES", "OPTIMIZERS", "REGS", "ETAS"])
def test_every_option_has_an_oracle_case(table):
    """A new learner / loss / optimizer / regulariser / eta schedule without a case here fails."""
    Ps = [c.learner(DIMS).P for c in CASES]
    if table == "LEARNERS":
        assert set(L.LEARNERS) == {c.name for c in CASES}
        assert {LO.ALGOS[cl.ALGO] for cl in L.LEARNERS.values()} <= set(range(len(O.ALGO_NAMES)))
        return
    field, names = {"LOSSES": ("loss", O.LOSS_NAMES), "OPTIMIZERS": ("opt", O.OPT_NAMES),
                    "REGS": ("reg", O.REG_NAMES), "ETAS": ("eta", O.ETA_NAMES)}[table]
    ids = set(getattr(LO, table).values())
    assert ids == set(range(len(names))), "the oracle's name table does not cover the engine's ids"
    have = {getattr(P, field) for c, P in zip(CASES, Ps) if c.general}
    assert ids <= have, sorted(ids - have)


# ---------------------------------------------------------------------------- CPU engine vs oracle
@pytest.mark.parametrize("cid", _ids(CASES))
def test_cpu_engine_matches_oracle(cid):
    """One replica, two passes (the step counter carries): whole state, touched mask, replica
    scalars and loss."""
    case, fx = BY_ID[cid], fixture(DIMS)
    ref = two_passes(case, fx)
    guard_ok(ref)
    st, loss = replica_run(case, fx, "cpu")
    check(st.S[0].numpy(), st.touched[0].numpy(), st.RS[0].numpy(), loss[0], ref, cid)
    assert ref["touched"].sum() > 250 and np.abs(ref["S"][..., 0]).max() > 1e-2   # it did train


def test_cpu_predict_matches_fp64():
    _predict_cases("cpu")


# ---------------------------------------------------------------------------- GPU: replica kernel
def _cap(dims):
    return max(64 * 8, min(dims, 1 << 22))          # ops/linear.py new_state


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _ids(CASES))
def test_gpu_replica_lds_matches_oracle(cid):
    """linear_train_kernel<true>: dims 300, the model in LDS, R = 1, every rule."""
    case, fx = BY_ID[cid], fixture(DIMS)
    ref = two_passes(case, fx, cap=_cap(DIMS) if case.mb > 1 else None)
    guard_ok(ref)
    st, loss = replica_run(case, fx, "cuda")
    check(st.S[0].cpu().numpy(), st.touched[0].cpu().numpy(), st.RS[0].cpu().numpy(), loss[0], ref, cid)


GLOBAL_CASES = ["train_pa1", "train_cw", "train_arow", "train_scw2", "train_adagrad_rda", "train_pa2a_regr",
                "train_arowe2_regr", "opt-adam", "opt-eve", "mb7-sgd", "train_multiclass_arow"]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", GLOBAL_CASES)
def test_gpu_replica_global_matches_oracle(cid):
    """linear_train_kernel<false>: L x 4200 x 16 B > 64 KiB, the model stays in global memory."""
    case, fx = BY_ID[cid], fixture(4200)
    assert case.labels * fx.dims * 16 > 64 * 1024
    ref = two_passes(case, fx, cap=_cap(4200) if case.mb > 1 else None)
    guard_ok(ref)
    st, loss = replica_run(case, fx, "cuda")
    check(st.S[0].cpu().numpy(), st.touched[0].cpu().numpy(), st.RS[0].cpu().numpy(), loss[0], ref, cid)


def _shard_check(case, fx, R, tag, stored=None, order=None):
    """Replica r against an oracle run over rows [n r / R, n (r + 1) / R) of ``fx``; the engine
    may read the same rows from ``stored`` through ``order``."""
    n = fx.n
    refs = []
    for r in range(R):
        rows = list(range(n * r // R, n * (r + 1) // R))
        refs.append(oracle_run(case, fx, [rows, rows], key=("shard", tag, R, r)))
        guard_ok(refs[-1])
    st, loss = replica_run(case, fx if stored is None else stored, "cuda", R=R, order=order)
    for r, ref in enumerate(refs):
        check(st.S[r].cpu().numpy(), st.touched[r].cpu().numpy(), st.RS[r].cpu().numpy(), loss[r], ref,
              f"{tag} R={R} r={r}")


SHARD_CASES = ["train_scw2", "opt-adam", "train_pa2a_regr", "train_multiclass_perceptron"]


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 3, 8])
@pytest.mark.parametrize("cid", SHARD_CASES)
def test_gpu_replica_shards_match_oracle(cid, R):
    """Replica r runs rows [n r / R, n (r + 1) / R) in order with its own scalars."""
    _shard_check(BY_ID[cid], fixture(DIMS), R, "full")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", SHARD_CASES)
def test_gpu_replica_shards_with_order(cid):
    """The same shards read through an ``order`` permutation of rows stored in another order."""
    _shard_check(BY_ID[cid], fixture(DIMS), 3, "full", stored=shuffled(DIMS), order=_PERM)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", SHARD_CASES)
def test_gpu_replica_empty_shards(cid):
    """R = 5 over 3 rows: shards 0 and 2 get no row and must leave their replica, scalars and
    loss untouched."""
    assert [3 * r // 5 for r in range(6)] == [0, 0, 1, 1, 2, 3]
    _shard_check(BY_ID[cid], three_rows(DIMS), 5, "3 rows")


MC_CASES = [c.id for c in CASES if c.labels == 3]


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [DIMS, 1500])
@pytest.mark.parametrize("cid", MC_CASES)
def test_gpu_multiclass_matches_oracle(cid, dims):
    """L = 3 in LDS (dims 300) and in global memory (dims 1500: 72 KB), rows of 65 and 130
    non-zeros: every in-range feature of a processed row is touched, also past the first 64."""
    case, fx = BY_ID[cid], fixture(dims)
    assert (3 * dims * 16 > 64 * 1024) == (dims == 1500)
    ref = two_passes(case, fx)
    guard_ok(ref)
    st, loss = replica_run(case, fx, "cuda")
    check(st.S[0].cpu().numpy(), st.touched[0].cpu().numpy(), st.RS[0].cpu().numpy(), loss[0], ref, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [DIMS, 1500])
@pytest.mark.parametrize("cid", ["train_multiclass_perceptron", "train_multiclass_arow"])
def test_gpu_multiclass_wide_rows_touch_every_feature(cid, dims):
    """Three rows of 63, 65 and 130 non-zeros seen once: over the whole fixture every feature also
    turns up among some row's first 64, which hides a mask that is set for the first chunk only.
    Here features 65.. of the wide rows are touched by nothing else (the kernel used to leave them
    unmarked: the model table dropped them and the mix kept replica 0's value)."""
    case, fx = BY_ID[cid], three_rows(dims)
    ref = oracle_run(case, fx, [range(3)], key="3 rows once")
    guard_ok(ref)
    assert ref["touched"].sum() > 130
    st, loss = replica_run(case, fx, "cuda", passes=1)
    check(st.S[0].cpu().numpy(), st.touched[0].cpu().numpy(), st.RS[0].cpu().numpy(), loss[0], ref, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [DIMS, 520, 4200])
@pytest.mark.parametrize("M", [2, 7])
@pytest.mark.parametrize("cid", ["mb7-sgd", "mb7-adam-l2"])
def test_gpu_replica_minibatch_matches_oracle(cid, M, dims):
    """The replica kernel's mini-batch rule.  Its batch list holds touched_cap = max(512, dims)
    features and a batch is cut short once fewer than 256 entries are free: at dims 300 (cap 512)
    after 257 distinct features, at dims 520 after 265, never at dims 4200.  A cut batch takes its
    step with the mean over the rows it has, at the step of its last row (pinned: the oracle
    cuts at the same points)."""
    base = BY_ID[cid]
    case = Case(f"{cid}-M{M}", base.name, base.opts, mb=M)
    fx = fixture(dims)
    ref = two_passes(case, fx, cap=_cap(dims))
    guard_ok(ref)
    if M == 7:
        assert (ref["early_flushes"] > 0) == (dims < 4200), ref["early_flushes"]
    st, loss = replica_run(case, fx, "cuda")
    check(st.S[0].cpu().numpy(), st.touched[0].cpu().numpy(), st.RS[0].cpu().numpy(), loss[0], ref, case.id)


# ---------------------------------------------------------------------------- GPU: shared / seq kernels
def _table_engine(kind, case, fx, order, **kw):
    """Two passes of the shared-table or the near-sequential kernel with one wave."""
    m = case.learner(fx.dims)
    f = fx.to("cuda")
    if kind == "shared":
        st = LO.new_shared_state(fx.dims, "cuda", fx.n, waves=kw.get("waves", 1), replicas=1, reload=kw["reload"])
        run = LO.train_pass_shared
    else:
        st = LO.new_seq_state(fx.dims, "cuda", waves=kw.get("waves", 1), spread=kw["spread"])
        run = LO.train_pass_seq
    st.S[..., 0] = torch.from_numpy(case.start(fx.dims)).to(st.S)
    od = None if order is None else torch.as_tensor(order, dtype=torch.int32, device="cuda")
    loss = torch.zeros(st.RS.shape[0], dtype=torch.float64)
    for ep in range(kw.get("passes", 2)):
        loss += run(st, m.P, f.indptr, f.idx, f.val, f.y[case.task], t0=ep * fx.n, order=od).cpu()
    return st, loss.numpy()



@pytest.mark.gpu
@pytest.mark.parametrize("cid", _ids(NONCOV))
def test_gpu_shared_kernel_one_wave_matches_oracle(cid):
    """linear_shared_kernel with one wave (no hot features): the sequential learner with step
    t0 + q + 1; ``reload`` both ways, with and without ``order``."""
    case, fx = BY_ID[cid], fixture(DIMS)
    ref = two_passes(case, fx)
    guard_ok(ref)
    for perm in (None, _PERM):
        for reload in (True, False):
            st, loss = _table_engine("shared", case, fx if perm is None else shuffled(DIMS), perm, reload=reload)
            check(st.S[0, 0].cpu().numpy(), st.touched[0].cpu().numpy(), st.RS[0].cpu().numpy(), loss[0], ref,
                  f"{cid} reload={reload} order={perm is not None}")


@pytest.mark.gpu
@pytest.mark.parametrize("spread", [1, 8])
@pytest.mark.parametrize("cid", _ids(NONCOV))
def test_gpu_seq_kernel_one_wave_matches_oracle(cid, spread):
    """linear_seq_kernel with one wave: the sequential learner through the software pipeline."""
    case, fx = BY_ID[cid], fixture(DIMS)
    ref = two_passes(case, fx)
    guard_ok(ref)
    for perm in (None, _PERM):
        st, loss = _table_engine("seq", case, fx if perm is None else shuffled(DIMS), perm, spread=spread)
        check(st.S[0, 0].cpu().numpy(), st.touched[0].cpu().numpy(), st.RS[0].cpu().numpy(), loss[0], ref,
              f"{cid} spread={spread} order={perm is not None}")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["train_pa1", "opt-adam", "train_pa2a_regr", "opt-eve"])
def test_gpu_seq_kernel_fewer_rows_than_waves(cid):
    """W = 8 waves, 5 rows with disjoint features (widths 65, 1, 0, 130, 2): wave g runs row g
    alone at step g + 1, waves 5..7 stay idle and leave their scalars and loss at zero."""
    case = BY_ID[cid]
    rng = np.random.default_rng(5)
    wd = [65, 1, 0, 130, 2]
    feats = rng.permutation(DIMS)[:sum(wd)].astype(np.int32)
    ip = np.concatenate([[0], np.cumsum(wd)]).astype(np.int64)
    base = fixture(DIMS)
    fx = Fixture(DIMS, torch.from_numpy(ip), torch.from_numpy(feats),
                 torch.from_numpy(rng.uniform(-1, 1, size=sum(wd)).astype(np.float32)),
                 {k: v[:5].contiguous() for k, v in base.y.items()})
    st, loss = _table_engine("seq", case, fx, None, spread=8, waves=8, passes=1)
    S, T, RS = st.S[0, 0].cpu().numpy(), st.touched[0].cpu().numpy().astype(bool), st.RS.cpu().numpy()
    seen = np.zeros(DIMS, dtype=bool)
    for g in range(5):
        ref = oracle_run(case, fx, [[g]], steps=[[g + 1]])
        f = ref["touched"]
        assert f.sum() == wd[g] and np.array_equal(T[f], ref["touched"][f])
        e = {"S": rel_err(S[f], ref["S"][0][f]), "rs": rel_err(RS[g, :6], ref["rs"][:6]),
             "loss": rel_err([loss[g]], [ref["loss"]])}
        assert max(e.values()) <= BOUND, (g, e)
        seen |= f
    assert np.array_equal(T, seen) and not S[~seen].any()
    assert not RS[5:].any() and not loss[5:].any()


# ---------------------------------------------------------------------------- GPU: mini-batch engine
@pytest.mark.gpu
@pytest.mark.parametrize("M", [2, 7, 400, 1000])
@pytest.mark.parametrize("opt", [o for o in OPTS if o != "eve"])
def test_gpu_minibatch_engine_matches_oracle(opt, M):
    """linear_mb_grad_kernel + linear_mb_apply_kernel: a tail batch (7), exactly one batch (400)
    and a batch larger than the pass (1000); two passes, steps t0 + q + 1."""
    base = BY_ID[f"opt-{opt}"]
    case = Case(f"{base.id}-M{M}", base.name, base.opts, mb=M)
    fx = fixture(DIMS)
    n = fx.n
    ref = oracle_run(case, fx, [range(n), range(n)], steps=[range(1, n + 1), range(n + 1, 2 * n + 1)], key="mbe")
    guard_ok(ref)
    m = case.learner(DIMS)
    f = fx.to("cuda")
    st = LO.new_minibatch_state(DIMS, "cuda", M, 130)
    loss = 0.0
    for ep in range(2):
        loss += LO.train_pass_minibatch(st, m.P, f.indptr, f.idx, f.val, f.y[case.task], t0=ep * n, M=M).item()
    check(st.S[0, 0].cpu().numpy(), st.touched[0].cpu().numpy(), None, loss, ref, case.id)
    assert not st.scratch["ga"].any() and not st.scratch["mark"].any()      # the batch buffers are left zeroed


# ---------------------------------------------------------------------------- GPU: mix kernels
def _mix_case(R, Lb, dims, kld, dev="cuda"):
    rng = np.random.default_rng(R * 100 + Lb * 10 + kld)
    S = rng.normal(size=(R, Lb, dims, 4)).astype(np.float32)
    S[..., 1] = rng.uniform(0.05, 2.0, size=(R, Lb, dims)).astype(np.float32)
    T = rng.random((R, dims)) < 0.5
    T[:, :40] = False                               # touched by no replica
    T[:, 40:80] = False
    T[rng.integers(0, R, size=40), np.arange(40, 80)] = True    # by exactly one
    T[:, 80:120] = True                             # by all
    S[0, :, 80:90, 1] = 1e-14                       # a covariance below the 1e-12 clamp
    st = LO.LinearState(torch.from_numpy(S).to(dev), torch.from_numpy(T.astype(np.uint8)).to(dev),
                        torch.zeros((R, 8), device=dev), True)
    S0 = S.copy()
    num, den, cnt = LO.mix_reduce(st, bool(kld))
    w_out, cov_out = LO.mix_apply(st, bool(kld), num, den, cnt)
    S1 = st.S.cpu().numpy()
    w_out, cov_out = w_out.cpu().numpy(), cov_out.cpu().numpy()
    # fp64 reference
    D = S0.astype(np.float64)
    t = T[:, None, :].astype(np.float64)
    inv = 1.0 / np.maximum(D[..., 1], 1e-12) if kld else np.ones_like(D[..., 1])
    c = np.broadcast_to(t, inv.shape).sum(0)
    hit = c > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        w = (D[..., 0] * inv * t).sum(0) / (inv * t).sum(0)
        scale = (np.abs(D[..., 0]) * inv * t).sum(0) / (inv * t).sum(0)
        cv = c / (inv * t).sum(0)
    # R products of two roundings, two sums of R terms, one division: (2 R + 3) half-ulps
    tol = (R + 4) * 2.0 ** -23
    assert np.array_equal(cnt.cpu().numpy().reshape(Lb, dims), c)
    assert (np.abs(w_out - w)[hit] <= tol * scale[hit] + 1e-30).all()
    assert np.array_equal(w_out[~hit], S0[0, ..., 0][~hit])                 # replica 0's value
    for r in range(R):
        # untouched elements stay bit-identical, touched ones hold the mixed value in every replica
        assert np.array_equal(S1[r][~hit], S0[r][~hit])
        assert np.array_equal(S1[r, ..., 0][hit], w_out[hit])
        assert np.array_equal(S1[r, ..., 2:], S0[r, ..., 2:])               # optimizer state stays local
        if kld:
            assert np.array_equal(S1[r, ..., 1][hit], cov_out[hit])
        else:
            assert np.array_equal(S1[r, ..., 1], S0[r, ..., 1])
    if kld:
        assert (np.abs(cov_out - cv)[hit] <= tol * cv[hit]).all()
        assert np.array_equal(cov_out[~hit], S0[0, ..., 1][~hit])
    else:
        assert np.array_equal(cov_out, S0[0, ..., 1])
    assert hit[:, 40:120].all() and not hit[:, :40].any()


@pytest.mark.gpu
@pytest.mark.parametrize("kld", [0, 1])
@pytest.mark.parametrize("Lb", [1, 3])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_gpu_mix_kernels_match_fp64(R, Lb, kld):
    _mix_case(R, Lb, 1000, kld)


@pytest.mark.gpu
def test_gpu_mix_kernels_grid_stride():
    """L x dims just above 8192 x 256 elements: the grid-stride loops take a second trip."""
    _mix_case(2, 1, 8192 * 256 + 300, 1)


# ---------------------------------------------------------------------------- predict
def _predict_one(dev, dims, Lb, indptr, idx, val, with_cov):
    rng = np.random.default_rng(dims + Lb)
    w = rng.normal(size=(Lb, dims)).astype(np.float32)
    cov = rng.uniform(0.1, 2.0, size=(Lb, dims)).astype(np.float32) if with_cov else None
    tw = torch.from_numpy(w).to(dev)
    tc = torch.from_numpy(cov).to(dev) if with_cov else None
    out, var = LO.predict_scores(tw, torch.from_numpy(indptr).to(dev), torch.from_numpy(idx).to(dev),
                                 None if val is None else torch.from_numpy(val).to(dev), tc)
    assert (var is None) == (not with_cov)
    n = indptr.size - 1
    ok = (idx >= 0) & (idx < dims)
    row = np.repeat(np.arange(n), np.diff(indptr))[ok]
    i = idx[ok].astype(np.int64)
    x = np.ones(i.size) if val is None else val[ok].astype(np.float64)
    cntr = np.bincount(row, minlength=n).astype(np.float64)
    for l in range(Lb):
        term = w[l].astype(np.float64)[i] * x
        ref = np.bincount(row, weights=term, minlength=n)
        mag = np.bincount(row, weights=np.abs(term), minlength=n)
        # a sequential fp32 sum of k products: (k + 1) half-ulps of the summed magnitudes
        assert (np.abs(out[:, l].cpu().numpy() - ref) <= (cntr + 2) * 2.0 ** -24 * mag + 1e-30).all()
        if with_cov:
            term = cov[l].astype(np.float64)[i] * x * x
            ref = np.bincount(row, weights=term, minlength=n)
            assert (np.abs(var[:, l].cpu().numpy() - ref) <= (cntr + 3) * 2.0 ** -24 * ref + 1e-30).all()


def _predict_cases(dev):
    fx = fixture(DIMS)
    rng = np.random.default_rng(9)
    # the fixture (empty rows, indices -1 and dims + 3) plus one row of 5,000 non-zeros
    big = rng.integers(-2, DIMS + 4, size=5000).astype(np.int32)
    indptr = np.concatenate([fx.indptr.numpy(), [fx.indptr[-1].item() + 5000]]).astype(np.int64)
    idx = np.concatenate([fx.idx.numpy(), big])
    val = np.concatenate([fx.val.numpy(), rng.uniform(-1, 1, size=5000).astype(np.float32)])
    for Lb in (1, 3):
        for with_cov in (False, True):
            _predict_one(dev, DIMS, Lb, indptr, idx, val, with_cov)
    _predict_one(dev, DIMS, 3, indptr, idx, None, True)
    # grid stride: n x L above 65,536 x 256 lanes, one-feature rows
    n = 65536 * 256 + 1000
    idx1 = (np.arange(n, dtype=np.int64) * 7 % (DIMS + 2) - 1).astype(np.int32)
    _predict_one(dev, DIMS, 1, np.arange(n + 1, dtype=np.int64), idx1,
                 rng.uniform(-1, 1, size=n).astype(np.float32), True)


@pytest.mark.gpu
def test_gpu_predict_kernel_matches_fp64():
    _predict_cases("cuda")
