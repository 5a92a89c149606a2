"""The specialised fp32 k = 4 training launch spreads a row's F F slots over 512 threads (eight
waves, three slots a thread at 39 fields; csrc/kernels/ffm.hip, SG32_TRAIN_TPB) where it used 256
(six slots); ``variant=12`` keeps the 256-thread instantiation.  The per-slot arithmetic is the same;
the forward score is summed in another grouping, so the two agree with the sequential C++ engine to
its rounding, not necessarily with each other bitwise.

The shapes are the smallest that reach each edge of the slot-to-thread map: F = 39 (1,521 slots:
the 15 dead ones at the tail of the last wave), 45 (2,025: the largest slot count, 4 a thread), 32
and 33 (either side of the 2 / 3 slots-a-thread boundary: 1,024 and 1,089 against 1,024), 2 (one
wave holds every slot); 700 rows on 64 blocks (10 or 11 rows a block) and a single row."""
import functools

import numpy as np
import pytest
import torch

from hivemall_amd.models.ffm import FFMTrainer
from hivemall_amd.ops.ffm import ffm_step

pytestmark = pytest.mark.gpu

KEYS = ("V", "G", "w", "wz", "wn")
OPTS = "-classification -factors 4 -seed 3"
FIELDS = (39, 45, 32, 33, 2)
ROWS = (700, 1)
NF = 1 << 15                     # >= 700 x 45 distinct features


def _rows(B, F, nf, seed):
    """B rows of F slots with explicit fields and values; feature ids from a seeded permutation, so no
    two slots of the batch share a feature (rows cannot race); each row holds every field once,
    rotated by the row number (field != position)."""
    g = torch.Generator().manual_seed(seed)
    assert B * F <= nf
    idx = torch.randperm(nf, generator=g)[:B * F].to(torch.int32).reshape(B, F)
    fld = ((torch.arange(F).unsqueeze(0) + torch.arange(B).unsqueeze(1)) % F).to(torch.int32)
    val = torch.rand(B, F, generator=g) + 0.5
    y = torch.where(torch.rand(B, generator=g) < 0.3, 1.0, -1.0)
    return idx.contiguous(), fld.contiguous(), val.contiguous(), y


def _cpu_step(nf, F, rows):
    """(start state, state and loss after one step of the sequential C++ engine)."""
    tc = FFMTrainer(OPTS, device="cpu")
    tc.init_state(nf, F)
    start = {k: v.clone() for k, v in tc.state.items()}
    loss = torch.full((rows[0].shape[0],), float("nan"))
    ffm_step(tc.state, *rows, tc.hyper, loss=loss)
    ref = {k: tc.state[k].clone() for k in KEYS}
    ref["loss"] = loss
    return start, ref


def _gpu_step(nf, F, rows, start, grid, variant):
    tg = FFMTrainer(OPTS, device="cuda")
    tg.init_state(nf, F)
    for k in tg.state:
        tg.state[k].copy_(start[k].cuda())
    loss = torch.full((rows[0].shape[0],), float("nan"), device="cuda")
    ffm_step(tg.state, *[t.cuda() for t in rows], tg.hyper, loss=loss, grid=grid, variant=variant)
    torch.cuda.synchronize()
    out = {k: tg.state[k].cpu() for k in KEYS}
    out["loss"] = loss.cpu()
    return out


@functools.lru_cache(maxsize=None)
def _reference(F, B):
    rows = _rows(B, F, NF, seed=100 * F + B)
    return (rows,) + _cpu_step(NF, F, rows)


@functools.lru_cache(maxsize=None)
def _launch(F, B, variant):
    rows, start, _ = _reference(F, B)
    return _gpu_step(NF, F, rows, start, 64, variant)


def _assert_close(got, ref, rtol=1e-4, atol=1e-5):
    for k in KEYS + ("loss",):
        a, b = got[k].numpy(), ref[k].numpy()
        assert not np.isnan(a).any(), k
        print(f"{k}: max |gpu - cpu| = {np.abs(a.astype(np.float64) - b).max():.3e}")
        np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=k)


def _assert_moved(got, start):
    moved = {k: not torch.equal(got[k], start[k]) for k in KEYS}
    assert all(moved.values()), f"the step changed nothing in {moved}"


@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("F", FIELDS)
def test_default_equals_sequential_engine(F, B):
    """One train step of the default path on rows that cannot race: V, G, w, wz, wn and the loss
    are the sequential engine's."""
    _, start, ref = _reference(F, B)
    got = _launch(F, B, None)
    _assert_moved(got, start)
    _assert_close(got, ref)


@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("F", FIELDS)
def test_default_and_256_thread_variant_agree_with_the_engine(F, B):
    """The same launches through variant 12: both thread counts are within the engine's bound; the
    difference between them (the forward sum's grouping) is printed."""
    _, start, ref = _reference(F, B)
    new, old = _launch(F, B, None), _launch(F, B, 12)
    _assert_moved(old, start)
    _assert_close(old, ref)
    _assert_close(new, ref)
    for k in KEYS + ("loss",):
        d = (new[k].double() - old[k].double()).abs().max().item()
        print(f"{k}: max |512 threads - 256 threads| = {d:.3e}")


def test_one_block_forwards_updates_between_rows_of_shared_features():
    """grid = 1, 64 rows over 195 distinct features (the rows of test_ffm_specialised's one-block
    test): rows 2 m and 2 m + 1 hold the same feature at every position, so each row's updates are
    forwarded into the next row's registers, slot by slot of the new slot-to-thread map.  One block
    is the sequential learner: the state equals the engine's."""
    B, F = 64, 39
    g = torch.Generator().manual_seed(5)
    pos = torch.arange(F).unsqueeze(0)
    idx = (pos + F * ((torch.arange(B).unsqueeze(1) // 2) % 5)).to(torch.int32).contiguous()
    fld = pos.expand(B, F).to(torch.int32).contiguous()
    val = torch.rand(B, F, generator=g) + 0.5
    y = torch.where(torch.rand(B, generator=g) < 0.3, 1.0, -1.0)
    assert idx.unique().numel() == 195
    rows = (idx, fld, val, y)
    start, ref = _cpu_step(200, F, rows)
    got = _gpu_step(200, F, rows, start, 1, None)
    _assert_moved(got, start)
    _assert_close(got, ref)


@pytest.mark.parametrize("B", [5, 1])
def test_padding_invalid_ids_empty_and_multihot_rows_equal_the_engine(B):
    """Fewer rows than blocks (and one row), idx = -1 padding, field and feature ids out of range,
    an empty row, and with B = 5 one multi-hot row (a field twice), which the launch defers to the
    grouped-update kernel."""
    F, nf = 39, 1 << 10
    idx, fld, val, y = _rows(B, F, nf, seed=23)
    idx[0, 30:] = -1                     # a short row
    idx[0, 3] = -1                       # a hole
    fld[0, 7] = F                        # field ids out of range: the slot is dropped
    fld[0, 9] = -2
    if B > 1:
        idx[1, :] = -1                   # an empty row
        idx[2, 5] = nf                   # feature id out of range
        fld[3, 4] = fld[3, 20]           # multi-hot: two features of one field
    rows = (idx, fld, val, y)
    start, ref = _cpu_step(nf, F, rows)
    got = _gpu_step(nf, F, rows, start, 64, None)
    _assert_moved(got, start)
    _assert_close(got, ref)


@pytest.mark.parametrize("nhot,grid", [(1000, 64), (2048, 2048)])
def test_side_table_loses_no_hot_step(nhot, grid):
    """test_ffm_side_flush's construction (V frozen, w pinned: every row's step is fixed by the data)
    through the default launch: the hot features end with the sequential engine's sums, so the
    block sums, the flush strides and the publish hold at the new thread count."""
    from tests.test_ffm_side_flush import _assert_no_step_lost

    _assert_no_step_lost("fp32", nhot, grid)
