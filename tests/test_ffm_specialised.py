"""The fp32 k = 4 training launch of the default learner runs an instantiation of
ffm_pipe_sg32_kernel specialised for it (csrc/kernels/ffm.hip, SG32_TRAIN); ``variant=11`` forces
the same launch (side table, kept registers, grid) onto the generic instantiation.  Only control
flow and address computation differ, so on inputs that cannot race the two must agree bitwise."""
import numpy as np
import pytest
import torch

from hivemall_amd.models.ffm import FFMTrainer
from hivemall_amd.ops.ffm import ffm_step

F = 39
KEYS = ("V", "G", "w", "wz", "wn")


def _rows(B, nf, seed, distinct=True):
    """B rows of 39 slots with explicit fields and values.  distinct: feature ids from a seeded
    permutation, no two slots of the batch share a feature (rows cannot race)."""
    g = torch.Generator().manual_seed(seed)
    assert B * F <= nf
    idx = torch.randperm(nf, generator=g)[:B * F].to(torch.int32).reshape(B, F)
    # every row holds each field once, rotated by the row number (field != position)
    fld = ((torch.arange(F).unsqueeze(0) + torch.arange(B).unsqueeze(1)) % F).to(torch.int32)
    val = torch.rand(B, F, generator=g) + 0.5
    y = torch.where(torch.rand(B, generator=g) < 0.3, 1.0, -1.0)
    return idx.contiguous(), fld.contiguous(), val.contiguous(), y


def _default_and_generic(nf, idx, fld, val, y, grid, lin_mode=None):
    """One train step from the same start through the default path and through variant 11, on one
    state object (so both launches see the same hot-feature side tables)."""
    t = FFMTrainer("-classification -factors 4 -seed 3", device="cuda")
    t.init_state(nf, F)
    start = {k: v.clone() for k, v in t.state.items()}
    dev = [None if a is None else a.cuda() for a in (idx, fld, val, y)]
    out = {}
    for variant in (None, 11):
        for k in t.state:
            t.state[k].copy_(start[k])
        loss = torch.full((idx.shape[0],), float("nan"), device="cuda")
        ffm_step(t.state, dev[0], dev[1], dev[2], dev[3], t.hyper, loss=loss, grid=grid, variant=variant,
                 lin_mode=lin_mode)
        torch.cuda.synchronize()
        out[variant] = {k: t.state[k].clone() for k in KEYS}
        out[variant]["loss"] = loss
    moved = {k: not torch.equal(out[None][k], start[k]) for k in KEYS}
    assert all(moved.values()), f"the step changed nothing in {moved}"
    return out[None], out[11]


def _assert_bitwise(a, b):
    for k in KEYS + ("loss",):
        assert not torch.isnan(a[k]).any(), k
        d = (a[k].double() - b[k].double()).abs().max().item()
        print(f"{k}: max |default - generic| = {d:.3e}")
        assert torch.equal(a[k], b[k]), f"{k}: default and variant 11 differ, max {d:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("lin_mode", [4, 0])
def test_specialised_equals_generic_many_blocks(lin_mode):
    """64 blocks walk 10 to 11 rows each (700 rows: the last-row edges, a block count that does
    not divide B); lin_mode 4 = the side table (LT = 1), 0 = plain record stores (LT = 0)."""
    idx, fld, val, y = _rows(700, 1 << 15, seed=11)
    a, b = _default_and_generic(1 << 15, idx, fld, val, y, grid=64, lin_mode=lin_mode)
    _assert_bitwise(a, b)


@pytest.mark.gpu
def test_specialised_equals_generic_one_block_shared_features():
    """grid = 1, 64 rows over 195 distinct features: rows 2 m and 2 m + 1 hold the same feature at
    every position, so each row's updates are forwarded into the next row's registers."""
    B = 64
    g = torch.Generator().manual_seed(5)
    pos = torch.arange(F).unsqueeze(0)
    idx = (pos + F * ((torch.arange(B).unsqueeze(1) // 2) % 5)).to(torch.int32).contiguous()
    fld = pos.expand(B, F).to(torch.int32).contiguous()
    val = torch.rand(B, F, generator=g) + 0.5
    y = torch.where(torch.rand(B, generator=g) < 0.3, 1.0, -1.0)
    assert idx.unique().numel() == 195
    a, b = _default_and_generic(200, idx, fld, val, y, grid=1)
    _assert_bitwise(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [5, 1])
def test_specialised_equals_generic_padding_and_invalid_rows(B):
    """Fewer rows than blocks (and one row), idx = -1 padding, field ids out of range, and with
    B = 5 one multi-hot row (a field twice), which both launches defer to the grouped-update
    kernel."""
    idx, fld, val, y = _rows(B, 1 << 10, seed=23)
    idx[0, 30:] = -1                     # a short row
    idx[0, 3] = -1                       # a hole
    fld[0, 7] = F                        # field ids out of range: the slot is dropped
    fld[0, 9] = -2
    if B > 1:
        idx[1, :] = -1                   # an empty row
        idx[2, 5] = 1 << 10              # feature id out of range
        fld[3, 4] = fld[3, 20]           # multi-hot: two features of one field
    a, b = _default_and_generic(1 << 10, idx, fld, val, y, grid=64)
    _assert_bitwise(a, b)


@pytest.mark.gpu
def test_implicit_fields_take_the_generic_instantiation_and_equal_cpu():
    """fld = val = None is a launch the specialised configuration must not take (it has no test
    for a missing array): the default path on such rows still equals the CPU engine."""
    B, nf = 700, 1 << 15
    idx, _, _, y = _rows(B, nf, seed=11)
    tc = FFMTrainer("-classification -factors 4 -seed 3", device="cpu")
    tc.init_state(nf, F)
    tg = FFMTrainer("-classification -factors 4 -seed 3", device="cuda")
    tg.init_state(nf, F)
    for k in tc.state:
        tg.state[k].copy_(tc.state[k].cuda())
    lc, lg = torch.empty(B), torch.empty(B, device="cuda")
    ffm_step(tc.state, idx, None, None, y, tc.hyper, loss=lc)
    ffm_step(tg.state, idx.cuda(), None, None, y.cuda(), tg.hyper, loss=lg, grid=64)
    torch.cuda.synchronize()
    np.testing.assert_allclose(lg.cpu().numpy(), lc.numpy(), rtol=1e-4, atol=1e-5)
    for k in KEYS:
        np.testing.assert_allclose(tg.state[k].cpu().numpy(), tc.state[k].numpy(), rtol=1e-4, atol=1e-5,
                                   err_msg=k)
