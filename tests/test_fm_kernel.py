"""Every path of the sparse FM kernel (csrc/kernels/fm.hip, hm_fm_step) and of its CPU twin
(csrc/host/fm_cpu.cpp) against the float64 oracle tests/oracle/fm_oracle.py::fm_run.

The kernel is Hogwild across waves, so a launch is compared exactly only on row sets whose result
does not depend on the order in which the waves run:
  A  disjoint rows: no id occurs in two rows of a launch;
  B  rows r and r + nw (the same wave, one after the other) share most ids, rows of different
     waves share none (``working_waves`` mirrors the launch geometry);
  C  one row per launch: rows share ids freely, the bias is on.

Tolerances.  fp32 paths: rtol 1e-4, atol 1e-6 against the oracle (as tests/test_fm.py).  The fp32
CPU engine's largest deviation from the oracle on w and V over the cases of this file is 0.09 of
that tolerance, so no state check needs a wider one; predictions and losses add SUM_EPS x the size
of the sums they are the difference of (close_outputs).  bf16 tables: every stored value is one
of the two bf16 neighbours of the oracle's value, the same fp32 tolerance allowed at a grid point.
"""
from collections import namedtuple
from dataclasses import dataclass, replace

import numpy as np
import pytest
import torch

from hivemall_amd.ops import fm as fmop
from hivemall_amd.ops.fm import FMHyper, fm_step
from tests.oracle.fm_oracle import fm_run

RTOL, ATOL = 1e-4, 1e-6
F32 = lambda v: float(np.float32(v))              # a hyper-parameter as the engines receive it
# A prediction is a difference of sums that nearly cancel, so its error is a fraction of the size
# of those sums (fm_run's `mag`), not of |p|.  Measured: the fp32 CPU engine on every fp32 input of
# this file is at most 1.44e-7 mag (2.4 x 2^-24) off the oracle; allowed: 4x that, for the GPU's
# other summation order and __expf / __logf.  test_fm_cpu_engine_prediction_error_behind_sum_eps
# pins the measurement itself on the inputs that gave it.
CPU_SUM_EPS = 1.5e-7
SUM_EPS = 5.8e-7
OOR = (-1, None, 2 ** 31 - 1, -2 ** 31)          # None: dims


@dataclass
class Case:
    indptr: np.ndarray            # int64 [n + 1], absolute offsets
    idx: np.ndarray               # int32
    val: np.ndarray | None        # float32
    y: np.ndarray | None          # float32 [n]
    dims: int

    @property
    def n(self):
        return len(self.indptr) - 1

    def touched(self):
        a, b = int(self.indptr[0]), int(self.indptr[-1])
        i = self.idx[a:b].astype(np.int64)
        m = np.zeros(self.dims, dtype=bool)
        m[i[(i >= 0) & (i < self.dims)]] = True
        return m

    def rows(self, a, b):
        """Rows [a, b) as a CSR slice of the same idx / val (indptr[0] != 0 for a > 0)."""
        return Case(self.indptr[a:b + 1], self.idx, self.val, None if self.y is None else self.y[a:b],
                    self.dims)


def _hyper(**kw):
    base = dict(eta0=0.05, power_t=0.25, total_steps=-1.0, eta_kind=0, lambda0=0.01, lambda_w=0.02,
                lambda_v=0.03, classification=True, use_w0=False, seed=31)
    base.update(kw)
    return FMHyper(**base)


def _labels(rng, n, cls):
    return (np.where(rng.random(n) < 0.4, 1.0, -1.0) if cls else rng.normal(0, 1, n)).astype(np.float32)


def _values(rng, m):
    """x in +-[0.5, 1.5]: never 0, so every feature of a trained row moves."""
    return (rng.uniform(0.5, 1.5, m) * rng.choice([-1.0, 1.0], m)).astype(np.float32)


def _case(rows, vals, y, dims):
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows] + [np.zeros(0, np.int64)])
    val = None if vals is None else np.concatenate(list(vals) + [np.zeros(0, np.float32)]).astype(np.float32)
    return Case(indptr, idx.astype(np.int32), val, y, dims)


def disjoint_rows(n, rng, cls=True, with_val=True, nnz=(1, 7), spare=16):
    """Schedule A: n rows over a permutation of the ids, `spare` ids left untouched."""
    cnt = rng.integers(nnz[0], nnz[1] + 1, n)
    dims = int(cnt.sum()) + spare
    ids = rng.permutation(dims)[:cnt.sum()]
    rows = np.split(ids, np.cumsum(cnt)[:-1])
    vals = [_values(rng, len(r)) for r in rows] if with_val else None
    return _case(rows, vals, _labels(rng, n, cls), dims)


def same_wave_rows(nw, per_wave, rng, cls=True, pool=8, take=6, spare=8):
    """Schedule B: row r draws `take` of the `pool` ids that belong to wave r % nw."""
    n = per_wave * nw + 3
    rows = [(r % nw) * pool + rng.permutation(pool)[:take] for r in range(n)]
    return _case(rows, [_values(rng, take) for _ in rows], _labels(rng, n, cls), nw * pool + spare)


def shared_rows(n, rng, cls=True, with_val=True, dims=48, nnz=(3, 10)):
    """Schedule C (and any sequential engine): rows share the ids of a small table freely."""
    rows = [rng.permutation(dims - 4)[:rng.integers(nnz[0], nnz[1] + 1)] for _ in range(n)]
    vals = [_values(rng, len(r)) for r in rows] if with_val else None
    return _case(rows, vals, _labels(rng, n, cls), dims)


def edge_rows(rng, cls=True, reps=2, spare=24):
    """Disjoint rows of 0, 1, 63, 64, 65, 128 and 130 non-zeros (`reps` times, shuffled), values in
    [-2, 2] with explicit zeros, ids out of range in the first 64 slots and in later chunks."""
    sizes = rng.permutation(np.repeat([0, 1, 63, 64, 65, 128, 130], reps))
    dims = int(sizes.sum()) + spare
    ids = rng.permutation(dims)
    rows, vals, at, q = [], [], 0, 0
    for m in sizes:
        r = ids[at:at + m].astype(np.int64)
        at += m
        v = rng.uniform(-2, 2, m).astype(np.float32)
        if m >= 63:
            v[1] = 0.0
            for slot in (2, 40, m - 1) + ((64, 66) if m > 66 else ()):
                o = OOR[q % 4]
                r[slot] = dims if o is None else o
                q += 1
            if m > 70:
                v[70] = 0.0
        rows.append(r)
        vals.append(v)
    return _case(rows, vals, _labels(rng, len(rows), cls), dims)


def init_tables(dims, KP, k, dtype, seed, vscale=0.3, wscale=0.1):
    """V0 [dims, KP] (columns k.. zero) and w, float64 copies of values the dtype holds exactly."""
    g = torch.Generator().manual_seed(seed)
    V = torch.zeros(dims, KP)
    V[:, :k] = torch.randn(dims, k, generator=g) * vscale
    w = torch.randn(dims, generator=g) * wscale
    return V.to(dtype).double().numpy(), w.double().numpy()


def make_state(V0, w_init, dtype, dev, w0_init=0.0, shards=1, spread=False):
    """Engine state holding V0 / w_init; the bias is w0_init in shard 0, or spread unevenly over
    all the shards.  Returns (state, bias as the engine will sum it)."""
    dims, KP = V0.shape
    w, V = fmop.new_state_tables(dims, KP, dtype, dev)
    V.copy_(torch.from_numpy(V0).to(dtype))
    w.copy_(torch.from_numpy(w_init).float())
    if dev == "cpu":
        w0 = torch.full((1,), float(w0_init))
    else:
        parts = np.zeros(shards, dtype=np.float32)
        if spread:
            parts[:] = w0_init * (np.arange(shards) + 1.0) / (shards * (shards + 1) / 2)
        else:
            parts[0] = w0_init
        w0 = torch.zeros(32 * shards)
        w0[::32] = torch.from_numpy(parts)
        w0 = w0.to(dev)
    st = {"w": w, "V": V, "w0": w0}
    return st, bias_of(st)


def bias_of(state):
    v = state["w0"].double().cpu().numpy()
    if v.size == 1:
        return float(v[0])
    off = np.ones(v.size, dtype=bool)
    off[::32] = False
    assert not v[off].any(), "only the shard slots of w0 may be written"
    return float(v[::32].sum())


def tables_of(state):
    return state["w"].double().cpu().numpy(), state["V"].double().cpu().numpy()


def to_dev(case, dev):
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    # a sliced indptr keeps its absolute offsets into the full idx / val, as train_rows passes it
    return (t(case.indptr, torch.int64), t(case.idx, torch.int32), t(case.val, torch.float32),
            t(case.y, torch.float32))


def launch(state, case, h, k, dev, t0=0, train=True, grid=0, hot=None, with_y=True):
    """One fm_step over the case's rows; returns (pred, loss) as float64 arrays."""
    ip, idx, val, y = to_dev(case, dev)
    pred = torch.full((case.n,), float("nan"), device=dev)
    loss = torch.full((case.n,), float("nan"), device=dev) if with_y else None
    fm_step(state, ip, idx, val, y if with_y else None, h, k, train=train, t0=t0, pred=pred, loss=loss,
            grid=grid, hot=hot)
    if dev != "cpu":
        torch.cuda.synchronize()
    return pred.double().cpu().numpy(), None if loss is None else loss.double().cpu().numpy()


Ref = namedtuple("Ref", "w0 w V pred loss mag")


def oracle(case, V0, w_init, w0_init, h, k, t0=0, train=True, with_y=True):
    mag = []
    out = fm_run(case.indptr, case.idx, case.val, case.y if with_y else None, case.dims, k, V0, w_init,
                 w0_init, h, t0=t0, train=train, mag=mag)
    return Ref(*out, np.array(mag))


def _close(got, want, what):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=what)


def close_outputs(pred, loss, ref, h, what="", rows=slice(None)):
    """pred / loss of an engine against the oracle's.  p is a difference of sums that nearly
    cancel, so its fp32 error is SUM_EPS of the size of those sums (ref.mag), whatever |p| is; the
    loss moves by at most max(1, |d|) times the error of p."""
    rp, rl, slack = ref.pred[rows], ref.loss[rows], SUM_EPS * ref.mag[rows]
    err = np.abs(pred - rp)
    ok = err <= RTOL * np.abs(rp) + ATOL + slack
    assert ok.all(), (what + " pred", pred[~ok][:4], rp[~ok][:4], slack[~ok][:4])
    if loss is not None:
        dmax = 1.0 if h.classification else np.maximum(1.0, np.sqrt(2 * rl))
        ok = np.abs(loss - rl) <= RTOL * np.abs(rl) + ATOL + dmax * slack
        assert ok.all(), (what + " loss", loss[~ok][:4], rl[~ok][:4])


def bf16_floor(x):
    """Largest bf16 value <= float32(x), as float64."""
    b = np.asarray(x, dtype=np.float64).astype(np.float32).view(np.uint32)
    t = b & np.uint32(0xFFFF0000)
    # clearing the low bits rounds toward zero: an inexact negative goes one step further down
    t = np.where((b >> 31 == 1) & (b != t), t + np.uint32(0x10000), t).astype(np.uint32)
    return t.view(np.float32).astype(np.float64)


def bf16_ceil(x):
    return -bf16_floor(-np.asarray(x, dtype=np.float64))


def assert_bf16_neighbours(got, exact, what):
    """got is the bf16 value below or above `exact` (fp32 tolerance at a grid point)."""
    tol = RTOL * np.abs(exact) + ATOL
    lo, hi = bf16_floor(exact - tol), bf16_ceil(exact + tol)
    bad = (got < lo) | (got > hi)
    assert not bad.any(), (what, int(bad.sum()), got[bad][:4], exact[bad][:4])


def check_tables(case, V0, w_init, got_w, got_V, ref_w, ref_V, k, dtype, what=""):
    """State after training against the oracle: touched entries to tolerance (bf16: neighbour
    rule, valid when every id was stepped once from V0), untouched entries and the padded columns
    bit-exact."""
    m = case.touched()
    assert np.array_equal(got_w[~m], w_init[~m]), what + " untouched w"
    assert np.array_equal(got_V[~m], V0[~m]), what + " untouched V"
    assert not got_V[:, k:].any(), what + " padded columns"
    _close(got_w, ref_w, what + " w")
    if dtype == torch.float32:
        _close(got_V[:, :k], ref_V[:, :k], what + " V")
    else:
        assert_bf16_neighbours(got_V[:, :k], ref_V[:, :k], what + " V")


def assert_rows_moved(case, got_w, w_init, what=""):
    for r in range(case.n):
        i = case.idx[case.indptr[r]:case.indptr[r + 1]]
        assert len(i) and (got_w[i] != w_init[i]).all(), f"{what} row {r} was not trained"


def run_and_check(case, h, KP, k, dtype, dev, seed=0, t0=0, grid=0, hot=None, w0_init=0.0, shards=1,
                  vscale=0.3, what=""):
    """One training launch from fresh tables against the oracle; returns the engine's tables."""
    V0, w_init = init_tables(case.dims, KP, k, dtype, seed, vscale=vscale)
    st, b0 = make_state(V0, w_init, dtype, dev, w0_init, shards)
    pred, loss = launch(st, case, h, k, dev, t0=t0, grid=grid, hot=hot)
    ref = oracle(case, V0, w_init, b0, h, k, t0=t0)
    gw, gV = tables_of(st)
    close_outputs(pred, loss, ref, h, what)
    check_tables(case, V0, w_init, gw, gV, ref.w, ref.V, k, dtype, what)
    if h.use_w0:
        _close(bias_of(st), ref.w0, what + " w0")
    return gw, gV, w_init


# ----------------------------------------------------------------------------- CPU engine
@pytest.fixture
def cpu_layout(monkeypatch):
    monkeypatch.setattr(fmop, "W_RECORD", False)     # the CPU engine takes contiguous tables


CPU_HYPERS = {
    "cls_bias": _hyper(use_w0=True),
    "cls_inverse": _hyper(eta_kind=2, use_w0=True),
    "reg_clip": _hyper(classification=False, min_target=-0.4, max_target=0.4, use_w0=True),
}


@pytest.mark.parametrize("with_val", [True, False])
@pytest.mark.parametrize("hname", list(CPU_HYPERS))
def test_fm_cpu_engine_shared_rows(cpu_layout, hname, with_val):
    h = CPU_HYPERS[hname]
    case = shared_rows(64, np.random.default_rng(5), cls=h.classification, with_val=with_val)
    run_and_check(case, h, 8, 8, torch.float32, "cpu", w0_init=0.3)


def test_fm_cpu_engine_clip_is_active(cpu_layout):
    h = CPU_HYPERS["reg_clip"]
    case = shared_rows(64, np.random.default_rng(6), cls=False)
    V0, w_init = init_tables(case.dims, 8, 8, torch.float32, 1)
    pred = oracle(case, V0, w_init, 0.0, h, 8)[3]
    assert (pred == F32(-0.4)).sum() > 3 and (pred == F32(0.4)).sum() > 3 and (np.abs(pred) < 0.39).sum() > 3
    run_and_check(case, h, 8, 8, torch.float32, "cpu", seed=1)


@pytest.mark.parametrize("t0", [0, 1000])
@pytest.mark.parametrize("eta_kind,total", [(0, -1.0), (1, 500.0), (1, -1.0), (2, -1.0)])
def test_fm_cpu_engine_eta_schedules(cpu_layout, eta_kind, total, t0):
    h = _hyper(eta_kind=eta_kind, total_steps=total, use_w0=True)
    case = shared_rows(48, np.random.default_rng(7))
    run_and_check(case, h, 8, 8, torch.float32, "cpu", t0=t0, w0_init=-0.2)


@pytest.mark.parametrize("KP,k", [(8, 5), (4, 3), (8, 1)])
def test_fm_cpu_engine_padded_factors(cpu_layout, KP, k):
    case = shared_rows(48, np.random.default_rng(8))
    run_and_check(case, _hyper(use_w0=True), KP, k, torch.float32, "cpu")


@pytest.mark.parametrize("cls", [True, False])
def test_fm_cpu_engine_edge_rows(cpu_layout, cls):
    """Empty rows, a row of 130 non-zeros, ids -1 / dims / 2^31 - 1 / -2^31, zero values."""
    case = edge_rows(np.random.default_rng(9), cls=cls, reps=1)
    assert {0, 130} <= set(np.diff(case.indptr)) and case.idx.max() == 2 ** 31 - 1 and case.idx.min() < 0
    assert case.dims in case.idx and (case.val == 0).any()
    h = _hyper(classification=cls, use_w0=True, min_target=-1.0, max_target=1.0)
    run_and_check(case, h, 8, 8, torch.float32, "cpu", vscale=0.05)


def test_fm_cpu_engine_indptr_slice(cpu_layout):
    full = shared_rows(40, np.random.default_rng(10))
    part = full.rows(7, 29)
    assert part.indptr[0] > 0
    run_and_check(part, _hyper(use_w0=True, eta_kind=2), 8, 8, torch.float32, "cpu", t0=7)


@pytest.mark.parametrize("cls", [True, False])
def test_fm_cpu_engine_predict_only(cpu_layout, cls):
    h = _hyper(classification=cls, use_w0=True, min_target=-0.4, max_target=0.4)
    case = shared_rows(40, np.random.default_rng(11), cls=cls)
    V0, w_init = init_tables(case.dims, 8, 8, torch.float32, 2)
    st, b0 = make_state(V0, w_init, torch.float32, "cpu", 0.25)
    pred, loss = launch(st, case, h, 8, "cpu", train=False)
    ref = oracle(case, V0, w_init, b0, h, 8, train=False)
    gw, gV = tables_of(st)
    assert np.array_equal(gw, w_init) and np.array_equal(gV, V0) and bias_of(st) == b0
    assert np.array_equal(ref[1], w_init) and np.array_equal(ref[2], V0) and ref[0] == b0
    close_outputs(pred, loss, ref, h)


def test_fm_cpu_engine_prediction_error_behind_sum_eps(cpu_layout):
    """The CPU engine's predictions on the rows of test_fm_gpu_factors_and_dtypes_sequential (the
    inputs with the largest error measured, 1.44e-7 of `mag`) stay within CPU_SUM_EPS, so the 4x of
    SUM_EPS keeps meaning 4x: an engine that loses accuracy fails here first."""
    assert SUM_EPS <= 4 * CPU_SUM_EPS
    h = _hyper(use_w0=True, lambda0=0.05, eta_kind=2)
    worst = 0.0
    for KP, k in FACTORS:
        case = shared_rows(64, np.random.default_rng(KP * 64 + k + 1))
        V0, w_init = init_tables(case.dims, KP, k, torch.float32, 0)
        st, b0 = make_state(V0, w_init, torch.float32, "cpu", 0.3)
        pred, _ = launch(st, case, h, k, "cpu")
        ref = oracle(case, V0, w_init, b0, h, k)
        worst = max(worst, float((np.abs(pred - ref.pred) / ref.mag).max()))
    print("largest |pred - oracle| / mag:", worst)
    assert worst <= CPU_SUM_EPS, worst


# ----------------------------------------------------------------------------- stochastic rounding
SR_N = 32768
SR_ULP = 2.0 ** -8                      # bf16 spacing in [0.5, 1)
SR_BOUND = 5 / (2 * np.sqrt(SR_N))      # 5 sigma of the mean of N errors of variance <= 1/4


def sr_inputs():
    """One step in which every V element moves down by 0.15 .. 0.3 bf16 ulp: V0 on the bf16 grid
    strictly inside (0.5, 1), x = 1e-6 (the data term vanishes), 2 eta lambda_v = 0.3 ulp."""
    rng = np.random.default_rng(12)
    KP = 32
    case = disjoint_rows(128, rng, with_val=True, nnz=(8, 8), spare=8)
    case.val[:] = 1e-6
    case.y[:] = 1.0
    assert case.touched().sum() * KP == SR_N
    V0 = 0.5 + rng.integers(1, 128, (case.dims, KP)) * SR_ULP
    h = _hyper(eta0=0.1, lambda_v=0.3 * SR_ULP / 0.2, lambda_w=0.0)
    w_init = np.zeros(case.dims)
    exact = oracle(case, V0, w_init, 0.0, h, KP)[2]
    return case, V0, w_init, h, KP, exact


def test_fm_sr_inputs_and_bound_on_emulated_rounding():
    case, V0, w_init, h, KP, exact = sr_inputs()
    m = case.touched()
    assert np.array_equal(V0, torch.from_numpy(V0).to(torch.bfloat16).double().numpy())
    frac = (V0[m] - exact[m]) / SR_ULP
    assert frac.size == SR_N and frac.min() >= 0.1 and frac.max() <= 0.4
    assert np.array_equal(bf16_ceil(exact[m]), V0[m]) and np.array_equal(bf16_floor(exact[m]), V0[m] - SR_ULP)
    u = np.random.default_rng(13).random(frac.shape)
    unbiased = V0[m] - SR_ULP * (u < frac)
    assert abs(((unbiased - exact[m]) / SR_ULP).mean()) <= SR_BOUND
    nearest = torch.from_numpy(exact[m]).to(torch.bfloat16).double().numpy()
    assert ((nearest - exact[m]) / SR_ULP).mean() >= 0.1 > SR_BOUND


# ----------------------------------------------------------------------------- GPU kernel
def select(mp, variant=0, xcds=6, wpb=2, record=False, hot_every=1, w0_every=None):
    """Kernel variant and launch geometry of the following fm_step calls.  HM_FM_XCDS is always
    set, which also keeps the early-training ramp from overriding grid and xcds."""
    mp.setenv("HM_FM_VARIANT", str(variant))
    mp.setenv("HM_FM_XCDS", str(xcds))
    if w0_every is None:
        mp.delenv("HM_FM_W0_EVERY", raising=False)
    else:
        mp.setenv("HM_FM_W0_EVERY", str(w0_every))
    mp.setattr(fmop, "WPB", wpb)
    mp.setattr(fmop, "W_RECORD", record)
    mp.setattr(fmop, "HOT_EVERY", hot_every)


def working_waves(grid, n_rows, wpb, xcds, variant):
    """Waves that take rows in one hm_fm_step launch (csrc/kernels/fm.hip launch()): wave g trains
    rows g, g + nw, g + 2 nw, ..."""
    blocks = grid if grid > 0 else (256 if xcds < 8 else 128)
    blocks = max(1, min(blocks, (n_rows + 3) // 4, 256 * 8 * 4))
    lb = blocks * 4 // wpb
    if xcds < 8 and variant != 1:
        lb = -(-lb // xcds) * xcds       # working workgroups: xcds of every 8 launched
    return lb * wpb


def test_working_waves_mirror():
    assert working_waves(1, 100, 4, 8, 0) == 4 and working_waves(1, 100, 2, 6, 0) == 12
    assert working_waves(1, 100, 2, 6, 1) == 4 and working_waves(3, 100, 1, 6, 0) == 12
    assert working_waves(3, 5, 1, 8, 0) == 8 and working_waves(0, 600, 2, 8, 0) == 512
    assert working_waves(0, 10 ** 6, 2, 6, 0) == 1032 and working_waves(0, 10 ** 6, 2, 8, 3) == 512


# (variant, waves per workgroup, xcds, grid): every value of every axis with variant 0, every
# variant with three geometries
GEOMETRIES = [(0, 2, 6, 1), (0, 1, 6, 3), (0, 4, 6, 0), (0, 2, 1, 3), (0, 2, 8, 1), (0, 4, 8, 3),
              (0, 1, 1, 1), (0, 2, 8, 0),
              (1, 2, 6, 1), (1, 4, 8, 3), (1, 1, 6, 0),
              (2, 2, 6, 1), (2, 1, 8, 3), (2, 4, 1, 1),
              (3, 2, 6, 3), (3, 4, 8, 1), (3, 2, 1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("variant,wpb,xcds,grid", GEOMETRIES)
def test_fm_gpu_disjoint_rows_every_geometry(monkeypatch, variant, wpb, xcds, grid):
    """Schedule A: waves with 0, 1 and several rows and a ragged tail.  A row skipped or trained
    twice is a mismatch; every row's features must have moved."""
    select(monkeypatch, variant, xcds, wpb)
    nw = working_waves(grid, 1 << 30, wpb, xcds, variant)
    # the auto grid (0; 512 to 1032 working waves) gives every row of a small launch its own wave:
    # only the last size runs its pipeline over several rows
    sizes = sorted({1, nw - 1, nw, nw + 1, 3 * nw + 5}) if grid > 0 else [1, 37, 600, 3 * nw + 5]
    for n in sizes:
        case = disjoint_rows(n, np.random.default_rng(100 + n), nnz=(1, 7 if n < 100 else 5 if n < 1000 else 2))
        gw, _, w_init = run_and_check(case, _hyper(), 8, 8, torch.float32, "cuda", seed=n, grid=grid,
                                      what=f"n={n}")
        assert_rows_moved(case, gw, w_init, f"n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant,wpb,xcds,grid", GEOMETRIES)
def test_fm_gpu_same_wave_reuses_features(monkeypatch, variant, wpb, xcds, grid):
    """Schedule B: a wave's consecutive rows share 6 of 8 ids (3 of 4 under the auto grid, whose
    512 to 1032 working waves need as many id pools), so the second row must read what the first
    one stored (V is not prefetched across rows) and the prefetched indices, values and labels
    must rotate correctly.  4 to 5 rows a wave."""
    select(monkeypatch, variant, xcds, wpb)
    nw = working_waves(grid, 1 << 30, wpb, xcds, variant)
    pool, take = (8, 6) if grid > 0 else (4, 3)
    case = same_wave_rows(nw, 4, np.random.default_rng(200 + nw), pool=pool, take=take)
    assert working_waves(grid, case.n, wpb, xcds, variant) == nw
    gw, _, w_init = run_and_check(case, _hyper(eta_kind=2), 8, 8, torch.float32, "cuda", grid=grid, t0=3)
    assert_rows_moved(case, gw, w_init)


FACTORS = [(4, 4), (4, 3), (8, 8), (8, 5), (16, 16), (16, 9), (32, 32), (32, 17), (8, 1)]
DTYPES = [torch.float32, torch.bfloat16]


@pytest.mark.gpu
@pytest.mark.parametrize("record", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("KP,k", FACTORS)
def test_fm_gpu_factors_and_dtypes_disjoint_rows(monkeypatch, KP, k, dtype, record):
    """Schedule A (12 working waves, 41 rows) for every table layout, through the pipelined kernel,
    the plain kernel and the SC1 buffer loads / stores."""
    case = disjoint_rows(41, np.random.default_rng(KP * 64 + k))
    for variant in (0, 1, 3):
        select(monkeypatch, variant, 6, 2, record)
        for cls in (True, False):
            h = _hyper(classification=cls, min_target=-0.5, max_target=0.5)
            run_and_check(case, h, KP, k, dtype, "cuda", seed=k, grid=1, what=f"variant {variant}")


def run_sequential(case, h, KP, k, dtype, t_start=0, w0_init=0.3, shards=64, spread=False, seed=0):
    """Schedule C: one launch per row on one state.  fp32 follows the oracle over the whole run;
    a bf16 table is compared step by step against the oracle stepped from the kernel's own
    previous state, so that rounding does not accumulate into the tolerance."""
    V0, w_init = init_tables(case.dims, KP, k, dtype, seed)
    st, b0 = make_state(V0, w_init, dtype, "cuda", w0_init, shards, spread)
    ip, idx, val, y = to_dev(case, "cuda")
    pred = torch.zeros(case.n, device="cuda")
    loss = torch.zeros(case.n, device="cuda")
    stepwise = dtype != torch.float32
    for r in range(case.n):
        if stepwise:
            bw, bV = tables_of(st)
            bb = bias_of(st)
        fm_step(st, ip[r:r + 2], idx, val, y[r:r + 1], h, k, t0=t_start + r, pred=pred[r:r + 1],
                loss=loss[r:r + 1])
        if stepwise:
            one = case.rows(r, r + 1)
            ref = oracle(one, bV, bw, bb, h, k, t0=t_start + r)
            gw, gV = tables_of(st)
            check_tables(one, bV, bw, gw, gV, ref.w, ref.V, k, dtype, f"row {r}")
            _close(bias_of(st), ref.w0, f"row {r} w0")
            close_outputs(pred[r:r + 1].double().cpu().numpy(), loss[r:r + 1].double().cpu().numpy(), ref, h,
                          f"row {r}")
    if not stepwise:
        ref = oracle(case, V0, w_init, b0, h, k, t0=t_start)
        gw, gV = tables_of(st)
        check_tables(case, V0, w_init, gw, gV, ref.w, ref.V, k, dtype)
        _close(bias_of(st), ref.w0, "w0")
        close_outputs(pred.double().cpu().numpy(), loss.double().cpu().numpy(), ref, h)
        assert abs(ref.w0 - b0) > 100 * ATOL        # the bias did move


@pytest.mark.gpu
@pytest.mark.parametrize("record", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("KP,k", FACTORS)
def test_fm_gpu_factors_and_dtypes_sequential(monkeypatch, KP, k, dtype, record):
    """Schedule C, 64 rows that share 44 ids, the bias on (2 lambda0 w0 included)."""
    select(monkeypatch, 0, 6, 2, record)
    case = shared_rows(64, np.random.default_rng(KP * 64 + k + 1))
    assert case.rows(5, 6).indptr[0] > 0
    run_sequential(case, _hyper(use_w0=True, lambda0=0.05, eta_kind=2), KP, k, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("shards,spread", [(1, False), (64, True), (7, True)])
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("cls,t_start", [(True, 0), (False, (1 << 20) + 7)])
def test_fm_gpu_sequential_bias_shards(monkeypatch, cls, t_start, variant, shards, spread):
    """Schedule C with the initial bias in one shard or spread over all of them, on both sides of
    W0_WARM_ROWS (one row per launch: the re-read cadence cannot matter), every kernel variant."""
    select(monkeypatch, variant, 6, 2)
    case = shared_rows(48, np.random.default_rng(300 + shards), cls=cls)
    h = _hyper(classification=cls, use_w0=True, lambda0=0.05, eta_kind=2, min_target=-0.5, max_target=0.5)
    run_sequential(case, h, 8, 8, torch.float32, t_start=t_start, shards=shards, spread=spread)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", [0, 1, 3])
@pytest.mark.parametrize("cls", [True, False])
def test_fm_gpu_row_shapes(monkeypatch, cls, variant, dtype):
    """0, 1, 63, 64, 65, 128 and 130 non-zeros in one launch of 4 working waves (so wide rows also
    go through the prefetch rotation), zero values, ids out of range in every chunk."""
    select(monkeypatch, variant, 8, 4)
    case = edge_rows(np.random.default_rng(400), cls=cls)
    assert working_waves(1, case.n, 4, 8, variant) == 4 < case.n
    h = _hyper(classification=cls, min_target=-1.0, max_target=1.0)
    run_and_check(case, h, 8, 8, dtype, "cuda", grid=1, vscale=0.05)


@pytest.mark.gpu
@pytest.mark.parametrize("t0", [0, 12345, (1 << 20) + 7])
@pytest.mark.parametrize("eta_kind,total", [(0, -1.0), (1, 5000.0), (1, -1.0), (2, -1.0)])
def test_fm_gpu_regression_clip_and_eta_schedules(monkeypatch, eta_kind, total, t0):
    """Schedule A, several rows a wave: the step of row r uses t = t0 + r + 1; the clip is active
    on both sides."""
    select(monkeypatch, 0, 6, 2)
    case = disjoint_rows(41, np.random.default_rng(500), cls=False, nnz=(4, 7))
    h = _hyper(classification=False, eta_kind=eta_kind, total_steps=total, min_target=-0.3, max_target=0.3)
    V0, w_init = init_tables(case.dims, 8, 8, torch.float32, 0)
    pred = oracle(case, V0, w_init, 0.0, h, 8, t0=t0)[3]
    assert (pred == F32(-0.3)).sum() > 2 and (pred == F32(0.3)).sum() > 2 and (np.abs(pred) < 0.29).sum() > 2
    for variant in (0, 1):
        select(monkeypatch, variant, 6, 2)
        run_and_check(case, h, 8, 8, torch.float32, "cuda", grid=1, t0=t0, what=f"variant {variant}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("cls", [True, False])
def test_fm_gpu_predict_only(monkeypatch, cls, variant, dtype):
    """train=False, y=None: the state stays bit-identical, predictions follow the oracle (clipped
    for regression), with the bias spread over 64 shards and several rows a wave."""
    select(monkeypatch, variant, 6, 2)
    h = _hyper(classification=cls, use_w0=True, min_target=-0.4, max_target=0.4)
    case = shared_rows(64, np.random.default_rng(600), cls=cls)
    V0, w_init = init_tables(case.dims, 8, 5, dtype, 3)
    st, b0 = make_state(V0, w_init, dtype, "cuda", 0.25, 64, spread=True)
    w0_before = st["w0"].clone()
    hot = torch.ones(case.dims, dtype=torch.uint8, device="cuda")
    pred, _ = launch(st, case, h, 5, "cuda", train=False, grid=1, hot=hot, with_y=False)
    gw, gV = tables_of(st)
    assert np.array_equal(gw, w_init) and np.array_equal(gV, V0) and torch.equal(st["w0"], w0_before)
    ref = oracle(case, V0, w_init, b0, h, 5, train=False, with_y=False)
    close_outputs(pred, None, ref, h)
    if not cls:
        assert (pred == F32(-0.4)).any() and (pred == F32(0.4)).any() and (np.abs(pred) <= F32(0.4)).all()


@pytest.mark.gpu
def test_fm_gpu_padding_of_trained_rows_is_cleared(monkeypatch):
    """Columns k..KP are padding and must never feed back: the kernel stores zeros there for
    every feature it trains.  Started from non-zero padding, the forward pass sees all KP columns
    (the oracle at k = KP), columns [0, k) take that step, and the padding of every trained
    feature is zero afterwards, of every other feature unchanged."""
    KP, k = 8, 5
    case = disjoint_rows(41, np.random.default_rng(700))
    V0, w_init = init_tables(case.dims, KP, KP, torch.float32, 4)
    m = case.touched()
    for variant in (0, 1, 2):
        select(monkeypatch, variant, 6, 2)
        st, _ = make_state(V0, w_init, torch.float32, "cuda")
        pred, _ = launch(st, case, _hyper(), k, "cuda", grid=1)
        ref = oracle(case, V0, w_init, 0.0, _hyper(), KP)
        gw, gV = tables_of(st)
        close_outputs(pred, None, ref, _hyper())
        _close(gw, ref.w, "w")
        _close(gV[:, :k], ref.V[:, :k], "V")
        assert not gV[m][:, k:].any() and np.array_equal(gV[~m], V0[~m])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("schedule", ["A", "B"])
@pytest.mark.parametrize("hot_every", [1, 4])
@pytest.mark.parametrize("kind", ["ones", "half"])
def test_fm_gpu_hot_feature_stores(monkeypatch, kind, hot_every, schedule, dtype):
    """Hot features (SC1 stores on the rows the hash mask picks): the same step and rounding seed
    as the plain store, so bit-identical to the hot=None run, and on the oracle.  On schedule B
    the next row of the wave reads the SC1-stored line back."""
    select(monkeypatch, 0, 6, 2, hot_every=hot_every)
    nw = working_waves(1, 1 << 30, 2, 6, 0)
    rng = np.random.default_rng(800)
    case = disjoint_rows(3 * nw + 5, rng) if schedule == "A" else same_wave_rows(nw, 4, rng)
    flags = np.ones(case.dims, dtype=np.uint8) if kind == "ones" else (rng.random(case.dims) < 0.5).astype(np.uint8)
    assert flags.any()
    V0, w_init = init_tables(case.dims, 8, 8, dtype, 5)
    h = _hyper()

    def train(rows, hot):
        st, _ = make_state(V0, w_init, dtype, "cuda")
        pred, loss = launch(st, rows, h, 8, "cuda", grid=1, hot=hot)
        return (*tables_of(st), pred, loss)

    plain, got = train(case, None), train(case, torch.from_numpy(flags).cuda())
    for a, b in zip(plain, got):
        assert np.array_equal(a, b)
    gw, gV, pred, loss = got
    assert_rows_moved(case, gw, w_init)
    if dtype == torch.float32 or schedule == "A":
        ref = oracle(case, V0, w_init, 0.0, h, 8)
        close_outputs(pred, loss, ref, h)
        check_tables(case, V0, w_init, gw, gV, ref.w, ref.V, 8, dtype)
        return
    # bf16 on schedule B: a feature is rounded once per row of its wave, so the whole launch is
    # not within one ulp of the oracle.  The launch over the first j * nw rows is the same
    # computation stopped after j rows a wave (rounding is seeded by the row number), and the
    # nw rows between two such stops are disjoint: each stop follows the oracle stepped from the
    # previous stop by the neighbour rule, and the last stop is the full launch.
    assert working_waves(1, nw, 2, 6, 0) == nw
    bw, bV, done = w_init, V0, 0
    while done < case.n:
        stop = min(done + nw, case.n)
        gw, gV, pred, loss = train(case.rows(0, stop), torch.from_numpy(flags).cuda())
        step = case.rows(done, stop)
        ref = oracle(step, bV, bw, 0.0, h, 8, t0=done)
        check_tables(step, bV, bw, gw, gV, ref.w, ref.V, 8, dtype, f"rows {done}..{stop}")
        close_outputs(pred[done:stop], loss[done:stop], ref, h, f"rows {done}..{stop}")
        bw, bV, done = gw, gV, stop
    for a, b in zip((gw, gV, pred, loss), got):
        assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_fm_gpu_hot_flags_on_wide_rows(monkeypatch, dtype):
    """Every id flagged hot on rows of up to 130 non-zeros.  The kernel looks the flag up for the
    first 64 non-zeros of a row only (later chunks always store plainly); either way the result
    is the hot=None run's, bit for bit, and the oracle's."""
    select(monkeypatch, 0, 8, 4)
    case = edge_rows(np.random.default_rng(850))
    V0, w_init = init_tables(case.dims, 8, 8, dtype, 8, vscale=0.05)
    h = _hyper()
    res = []
    for hot in (None, torch.ones(case.dims, dtype=torch.uint8, device="cuda")):
        st, _ = make_state(V0, w_init, dtype, "cuda")
        pred, loss = launch(st, case, h, 8, "cuda", grid=1, hot=hot)
        res.append((*tables_of(st), pred, loss))
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    gw, gV, pred, loss = res[1]
    ref = oracle(case, V0, w_init, 0.0, h, 8)
    close_outputs(pred, loss, ref, h)
    check_tables(case, V0, w_init, gw, gV, ref.w, ref.V, 8, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [1, 64])
@pytest.mark.parametrize("w0_every", [1, 8])
@pytest.mark.parametrize("grid", [1, 3, 16, 0])
def test_fm_gpu_bias_atomics_conserve_every_step(monkeypatch, grid, w0_every, shards):
    """Schedule A with the bias on, lambda0 = 0, fixed eta, every label +1: each row adds
    -eta d_r > 0 to one shard, with d_r recomputed in float64 from the kernel's own prediction.
    The shards must sum to -eta sum d_r: one dropped or doubled atomic moves the sum by more than
    4x the tolerance (asserted).  A wave can only have seen a partial sum of the bias, so every
    prediction exceeds the oracle's bias-free part by something in [0, final bias]."""
    select(monkeypatch, 0, 6, 2, w0_every=w0_every)
    n = 512
    case = disjoint_rows(n, np.random.default_rng(900), nnz=(3, 3))
    case.y[:] = 1.0
    h = _hyper(use_w0=True, lambda0=0.0, eta0=0.002)
    V0, w_init = init_tables(case.dims, 8, 8, torch.float32, 6, vscale=0.1)   # |p| small: d near -1/2
    st, b0 = make_state(V0, w_init, torch.float32, "cuda", 0.0, shards)
    pred, _ = launch(st, case, h, 8, "cuda", grid=grid)
    final = bias_of(st)
    eta = float(np.float32(h.eta0))
    d = -1.0 / (1.0 + np.exp(pred))
    want = -eta * d.sum()
    # fp32 atomics into a sum <= 0.52: half an ulp (3e-8) a step, 512 steps < 1.6e-5 < RTOL * want
    tol = RTOL * want
    assert eta * np.abs(d).min() > 4 * tol
    assert abs(final - want) <= tol, (final, want)
    nobias = oracle(case, V0, w_init, 0.0, replace(h, use_w0=False), 8, train=False)
    seen = pred - nobias.pred
    slack = RTOL * np.abs(pred) + ATOL + SUM_EPS * (nobias.mag + final)
    assert (seen >= -slack).all() and (seen <= final + slack).all(), (seen.min(), seen.max(), final)


@pytest.mark.gpu
@pytest.mark.parametrize("KP", [4, 8])
def test_fm_gpu_stochastic_rounding_is_deterministic_and_seeded(monkeypatch, KP):
    """One bf16 step: the same (seed, t0) gives the same bits; another seed or another t0 gives
    another pattern (some elements differ, not all), each still a neighbour of the exact value."""
    select(monkeypatch, 0, 6, 2)
    case = disjoint_rows(128, np.random.default_rng(1000), nnz=(6, 8))
    V0, w_init = init_tables(case.dims, KP, KP, torch.bfloat16, 7)
    exact = oracle(case, V0, w_init, 0.0, _hyper(), KP, t0=50)[2]
    m = case.touched()

    def run(seed, t0):
        st, _ = make_state(V0, w_init, torch.bfloat16, "cuda")
        launch(st, case, _hyper(seed=seed), KP, "cuda", t0=t0)
        V = tables_of(st)[1]
        assert_bf16_neighbours(V, exact, f"seed {seed} t0 {t0}")
        return V[m]

    base = run(31, 50)
    assert np.array_equal(base, run(31, 50))
    for other in (run(32, 50), run(31, 51)):
        frac = (other != base).mean()
        # an element differs when its two draws fall on either side of its fraction: 2 f (1 - f),
        # about a third on average for fractions spread over (0, 1)
        assert 0.1 < frac < 0.6, frac


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 3])
def test_fm_gpu_stochastic_rounding_is_unbiased(monkeypatch, variant):
    """32768 elements step down by 0.15 .. 0.3 ulp each (sr_inputs, checked on the CPU above).
    With e = (stored - exact) / ulp in (-1, 1) and variance <= 1/4, |mean e| <= 5 / (2 sqrt N);
    round-to-nearest gives mean e >= 0.1."""
    select(monkeypatch, variant, 6, 2)
    case, V0, w_init, h, KP, exact = sr_inputs()
    st, _ = make_state(V0, w_init, torch.bfloat16, "cuda")
    launch(st, case, h, KP, "cuda")
    m = case.touched()
    V = tables_of(st)[1]
    assert np.array_equal(V[~m], V0[~m])
    e = (V[m] - exact[m]) / SR_ULP
    assert e.size == SR_N and (np.abs(e) < 1).all()
    assert 0.05 < (V[m] != V0[m]).mean() < 0.45          # rounded down with probability 0.15 .. 0.3
    assert abs(e.mean()) <= SR_BOUND, (e.mean(), SR_BOUND)
