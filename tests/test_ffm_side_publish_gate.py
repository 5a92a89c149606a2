"""The publish gate of the hot-feature side table (csrc/kernels/ffm.hip, hacc_ctl_off): a starting
block copies ACC to READ only when at least T = EVERY block flushes have been counted (FLUSHED)
since its XCD's last publish (SEEN[x]).  The gate decides how stale READ may be, never what ACC
holds: sums live only in ACC.

The learner is frozen as in test_ffm_side_flush.py (-eta0 0, -lambda 0, w pinned at 0 by -lambda1
1e9): every row's step is fixed by the data, so the hot features must end with the sequential
engine's sums whatever T, the order and the concurrency, and n only grows."""
import functools

import numpy as np
import pytest
import torch

from hivemall_amd.models.ffm import FFMTrainer
from hivemall_amd.ops import ffm as ffm_ops
from hivemall_amd.ops.ffm import ffm_step

pytestmark = pytest.mark.gpu

NF = 1 << 16
FROZEN = "-eta0 0 -lambda 0 -lambda1 1e9 -num_fields 39"
# (state option, factors): the fp32 k = 4 kernel, the bf16 12-B-slot kernel, the fp32 k = 8 instance
KERNELS = {"fp32": ("", 4), "bf16": (" -bf16_state", 4), "fp32_k8": ("", 8)}
NEVER = 1 << 30          # a threshold no launch of these tests reaches: no block publishes
KEYS = ("V", "G", "w", "wz", "wn")


@functools.lru_cache(maxsize=None)
def _data():
    from hivemall_amd.io.synthetic import criteo_ffm

    idx, fld, val, y = criteo_ffm(8192, hash_bits=16, seed=11)
    single = torch.tensor([len(set(r)) == len(r) for r in idx.tolist()])   # no multi-hot rows
    assert int(single.sum()) >= 0.95 * idx.shape[0]
    return tuple(t[single].contiguous() for t in (idx, fld, val, y))


@functools.lru_cache(maxsize=None)
def _planted():
    """The batch with one planted feature at position 0 of every row: every block flushes it."""
    idx, fld, val, y = _data()
    idx = idx.clone()
    plant = int(torch.bincount(idx[:, 0].long()).argmax())
    idx[:, 1:][idx[:, 1:] == plant] = -1       # any other occurrence of it: padding
    idx[:, 0] = plant
    return (idx, fld, val, y), plant


def _trainer(dev, kernel):
    state, k = KERNELS[kernel]
    t = FFMTrainer(f"-classification -factors {k} -seed 3 {FROZEN}{state}", device=dev)
    t.init_state(NF, 39)
    return t


@functools.lru_cache(maxsize=None)
def _reference(kernel):
    """(n, z) of every feature after the sequential CPU engine's pass, and the start state (the
    GPU state's stored, for bf16 rounded, values)."""
    idx, fld, val, y = _data()
    tc, tg = _trainer("cpu", kernel), _trainer("cuda", kernel)
    for k in tc.state:
        tg.state[k].copy_(tc.state[k].to("cuda"))
        tc.state[k].copy_(tg.state[k].float().cpu())
    start = {k: v.clone() for k, v in tc.state.items()}
    ffm_step(tc.state, idx, fld, val, y, tc.hyper)
    return tc.state["wn"].double(), tc.state["wz"].double(), start


def _fresh(kernel):
    tg = _trainer("cuda", kernel)
    for k, v in _reference(kernel)[2].items():
        tg.state[k].copy_(v.to("cuda"))
    ffm_ops._LIN_HOT.clear()
    return tg


def _steps(tg, data, grid, every, nhot=2048, launches=1, before=None):
    """`launches` GPU launches with threshold T = every (None: the default); the side tables
    (hidx, hot_id, hacc).  before(tables): called ahead of the last launch."""
    dev = [t.cuda() for t in data]
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(ffm_ops, "_LIN_HOT_N", nhot)
        if every is not None:
            mp.setattr(ffm_ops, "HACC_PUBLISH_EVERY", every)
        for i in range(launches):
            if before is not None and i == launches - 1:
                before(next(iter(ffm_ops._LIN_HOT.values())))
            ffm_step(tg.state, *dev, tg.hyper, grid=grid)
            torch.cuda.synchronize()
    finally:
        mp.undo()
    return next(iter(ffm_ops._LIN_HOT.values()))[:3]


def _assert_sequential_sums(kernel, tg, hot_id, nhot):
    n_ref, z_ref, _ = _reference(kernel)
    hot = hot_id.long().cpu()
    assert hot.numel() == min(nhot, 1024 if kernel == "bf16" else 2048)
    n, z = tg.state["wn"].double().cpu(), tg.state["wz"].double().cpu()
    assert float(tg.state["w"].float().abs().max()) == 0.0
    np.testing.assert_allclose(n[hot].numpy(), n_ref[hot].numpy(), rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(z[hot].numpy(), z_ref[hot].numpy(), rtol=2e-3,
                               atol=2e-3 * float(z_ref[hot].abs().max()))


@pytest.mark.parametrize("grid", [64, 2048])
@pytest.mark.parametrize("nhot", [2048, 1000, 1])
@pytest.mark.parametrize("every", [1, 8, NEVER])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_gate_loses_no_step(kernel, every, nhot, grid):
    """After one launch the hot features' n and z are the sequential engine's sums at every T: a
    block that skips its publish still flushes into ACC, and the fold takes ACC."""
    tg = _fresh(kernel)
    _, hot_id, hacc = _steps(tg, _data(), grid, every, nhot=nhot)
    assert int(ffm_ops._hacc_ctl(hacc, hot_id.numel())[2]) == every
    _assert_sequential_sums(kernel, tg, hot_id, nhot)


@pytest.mark.parametrize("every", [1, 8, NEVER])
@pytest.mark.parametrize("kernel", ["fp32", "bf16"])
def test_gate_is_what_publishes(kernel, every):
    """Two launches of 4,096 blocks on rows that all hold one planted feature.  READ after the second
    launch lies between the launch-start values and ACC for every entry; with a threshold no launch
    reaches it still IS the launch-start table, although ACC moved; at T = 1 a later block published
    an earlier block's flush of the planted feature."""
    data, plant = _planted()
    tg = _fresh(kernel)
    start = {}

    def before(tables):      # ahead of the second launch: the records dir 0 will copy out
        hot = tables[1].long()
        start["z"], start["n"] = tg.state["wz"][hot].clone(), tg.state["wn"][hot].clone()

    hidx, hot_id, hacc = _steps(tg, data, 4096, every, launches=2, before=before)
    z0, n0 = start["z"], start["n"]
    h = int(hidx[plant])
    assert h >= 0 and float(n0[h]) > 0.0
    acc, read = ffm_ops._hacc_views(hacc, hot_id.numel())
    acc_n, read_n = acc[:, 1], read[:, 1]
    print(f"T = {every}: planted n0 {float(n0[h]):.6g}  READ.n {float(read_n[h]):.6g}  ACC.n {float(acc_n[h]):.6g}")
    assert bool((read_n >= n0).all())
    ulp = torch.nextafter(acc_n, torch.full_like(acc_n, float("inf"))) - acc_n
    assert bool((read_n <= acc_n + ulp).all())
    assert bool((read[:, 2:] == 0).all())
    assert bool(torch.equal(acc_n, tg.state["wn"][hot_id.long()]))   # the fold took ACC, not READ
    assert float(acc_n[h]) > float(n0[h])
    if every == NEVER:
        assert bool(torch.equal(read_n, n0)) and bool(torch.equal(read[:, 0], z0))
    if every == 1:
        assert float(read_n[h]) > float(n0[h])


@pytest.mark.parametrize("every", [1, NEVER])
@pytest.mark.parametrize("kernel", ["fp32", "bf16"])
@pytest.mark.parametrize("grid,rows", [(4096, None), (64, None), (256, 100)])
def test_gate_counters(kernel, every, grid, rows):
    """FLUSHED counts the blocks that had a row (min(G, B)), from zero in every launch; SEEN[x] is a
    value of FLUSHED some block read, 0 when nothing publishes."""
    data = _data() if rows is None else tuple(t[:rows].contiguous() for t in _data())
    B = data[0].shape[0]
    tg = _fresh(kernel)
    for launches in (1, 2):
        _, hot_id, hacc = _steps(tg, data, grid, every)
        flushed, seen, ev = (t.cpu() for t in ffm_ops._hacc_ctl(hacc, hot_id.numel()))
        print(f"T = {every}, G = {grid}, B = {B}, launch {launches}: FLUSHED {int(flushed)} SEEN {seen.tolist()}")
        assert int(ev) == every
        assert int(flushed) == min(grid, B)
        assert bool((seen >= 0).all()) and bool((seen <= flushed).all())
        if every == NEVER:
            assert bool((seen == 0).all())
        if every == 1 and grid == 4096:
            assert bool((seen > 0).any())


def _race_free_rows(B, nf, seed):
    """B rows of 39 slots, feature ids from a seeded permutation: no two slots of the batch share a
    feature, so no row reads what another writes and READ is the launch-start table at any T."""
    g = torch.Generator().manual_seed(seed)
    F = 39
    idx = torch.randperm(nf, generator=g)[:B * F].to(torch.int32).reshape(B, F)
    fld = ((torch.arange(F).unsqueeze(0) + torch.arange(B).unsqueeze(1)) % F).to(torch.int32)
    val = torch.rand(B, F, generator=g) + 0.5
    y = torch.where(torch.rand(B, generator=g) < 0.3, 1.0, -1.0)
    return idx.contiguous(), fld.contiguous(), val.contiguous(), y


@pytest.mark.parametrize("state", ["", " -bf16_state"], ids=["fp32", "bf16"])
def test_gate_race_free_bitwise_across_thresholds(state):
    """700 rows of distinct features on 64 blocks, a learner that moves: V, G, w, wz, wn and the loss
    are bitwise the same at T = 1, the default T and a T that never publishes."""
    nf = 1 << 15
    idx, fld, val, y = (a.cuda() for a in _race_free_rows(700, nf, seed=11))
    t = FFMTrainer("-classification -factors 4 -seed 3" + state, device="cuda")
    t.init_state(nf, 39)
    start = {k: v.clone() for k, v in t.state.items()}
    out = {}
    for every in (1, None, NEVER):
        for k in t.state:
            t.state[k].copy_(start[k])
        ffm_ops._LIN_HOT.clear()
        loss = torch.full((700,), float("nan"), device="cuda")
        mp = pytest.MonkeyPatch()
        try:
            if every is not None:
                mp.setattr(ffm_ops, "HACC_PUBLISH_EVERY", every)
            mp.setattr(ffm_ops, "_CALLS", 0)     # the bf16 stochastic rounding is seeded by the call count
            ffm_step(t.state, idx, fld, val, y, t.hyper, loss=loss, grid=64)
            torch.cuda.synchronize()
        finally:
            mp.undo()
        hacc = next(iter(ffm_ops._LIN_HOT.values()))[2]      # the side table ran
        assert int(ffm_ops._hacc_ctl(hacc, next(iter(ffm_ops._LIN_HOT.values()))[1].numel())[0]) == 64
        out[every] = {k: t.state[k].clone() for k in KEYS}
        out[every]["loss"] = loss
    assert all(not torch.equal(out[1][k], start[k]) for k in KEYS), "the step changed nothing"
    for every in (None, NEVER):
        for k in KEYS + ("loss",):
            assert not torch.isnan(out[every][k].float()).any(), k
            assert torch.equal(out[1][k], out[every][k]), f"{k}: T = 1 and T = {every} differ"


@pytest.mark.parametrize("kernel,nhot", [("fp32", 1), ("fp32", 1000), ("fp32", 2048), ("bf16", 1), ("bf16", 1000)])
def test_gate_control_block_geometry(kernel, nhot):
    """The control block starts on a 128-B line behind READ; FLUSHED, every SEEN[x] and EVERY have
    a line each; the allocation holds all of it, for a single hot feature and for a partial line."""
    tg = _fresh(kernel)
    _, hot_id, hacc = _steps(tg, _data(), 64, None, nhot=nhot)
    n = hot_id.numel()
    assert n == nhot
    off, ctl = ffm_ops._hacc_read_off(n), ffm_ops._hacc_ctl_off(n)
    assert ctl >= off + 4 * n                               # behind READ's n entries of 16 B
    assert hacc.data_ptr() % 128 == 0 and ctl % 32 == 0     # on a 128-B line of its own
    assert hacc.numel() >= ctl + 32 * 10                    # FLUSHED, SEEN[8], EVERY: a line each
    flushed, seen, every = ffm_ops._hacc_ctl(hacc, n)
    line = lambda t: (t.data_ptr() - hacc.data_ptr()) // 128
    lines = [line(flushed)] + [line(seen[x:x + 1]) for x in range(8)] + [line(every)]
    assert lines == list(range(ctl // 32, ctl // 32 + 10))  # ten distinct lines, FLUSHED's the first
    assert int(every) == ffm_ops.HACC_PUBLISH_EVERY
    # nothing else on the counters' lines: the rest of each line is still the allocation's zeros
    block = hacc[ctl:ctl + 320].view(torch.int32).view(10, 32)
    assert bool((block[:, 1:] == 0).all())


def test_gate_one_block_leaves_the_control_block_alone():
    """grid = 1 is the sequential learner: no side table, so nothing reads or writes the control
    block, and the hot features end with the sequential engine's sums."""
    tg = _fresh("fp32")
    dev = [t.cuda() for t in _data()]
    hidx, hot_id, hacc = ffm_ops._lin_hot_tables(tg.state, dev[0], 2048)
    n = hot_id.numel()
    flushed, seen, every = ffm_ops._hacc_ctl(hacc, n)
    flushed.fill_(0x5A5A)
    seen.fill_(0x3C3C)
    ffm_step(tg.state, *dev, tg.hyper, grid=1)
    torch.cuda.synchronize()
    assert next(iter(ffm_ops._LIN_HOT.values()))[2] is hacc
    assert int(flushed) == 0x5A5A and bool((seen == 0x3C3C).all())
    assert int(every) == ffm_ops.HACC_PUBLISH_EVERY
    acc, read = ffm_ops._hacc_views(hacc, n)
    assert bool((acc == 0).all()) and bool((read == 0).all())
    _assert_sequential_sums("fp32", tg, hot_id, 2048)
