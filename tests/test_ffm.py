import numpy as np
import pytest
import torch

from hivemall_amd.io.synthetic import criteo_like
from hivemall_amd.models.ffm import FFMBatch, FFMTrainer, train_ffm
from hivemall_amd.ops.ffm import ffm_step, is_packed, new_state_tables
from tests.oracle.ffm_oracle import ffm_train_rows


def _trainer(dev, nf=64, nfld=6, k=4, extra=""):
    t = FFMTrainer(f"-classification -factors {k} -seed 3 {extra}", device=dev)
    t.init_state(nf, nfld)
    return t


def _np_state(t):
    return {k: v.detach().cpu().numpy().astype(np.float64).copy() for k, v in t.state.items()}


@pytest.mark.parametrize("use_bias,adagrad", [(False, ""), (True, ""), (True, "-elementwise_adagrad")])
def test_ffm_cpu_engine_matches_oracle(use_bias, adagrad):
    rng = np.random.default_rng(0)
    B, F, NF = 40, 6, 64
    idx = rng.integers(0, NF, size=(B, F)).astype(np.int32)
    val = rng.uniform(0.5, 2.0, size=(B, F)).astype(np.float32)
    y = np.where(rng.random(B) < 0.4, 1.0, -1.0).astype(np.float32)
    t = _trainer("cpu", NF, F, extra=("-w0 " if use_bias else "") + adagrad)
    assert t.state["G"].dim() == (3 if adagrad else 2)
    ref = _np_state(t)
    h = t.hyper
    hp = dict(eta0=h.eta0, eps=h.eps, lambda_v=h.lambda_v, alpha=h.alpha, beta=h.beta,
              lambda1=h.lambda1, lambda2=h.lambda2)
    ref_loss, ref_pred = ffm_train_rows(ref, idx, y, hp, val=val, use_bias=use_bias)
    loss = torch.empty(B)
    ffm_step(t.state, torch.from_numpy(idx), None, torch.from_numpy(val), torch.from_numpy(y), h,
             loss=loss)
    np.testing.assert_allclose(loss.numpy(), ref_loss, rtol=2e-4, atol=2e-5)
    for k in ("V", "G", "w", "wz", "wn", "bias"):
        np.testing.assert_allclose(t.state[k].numpy(), ref[k], rtol=2e-4, atol=2e-5, err_msg=k)


def _multihot_rows(B, F, NF, NFLD, seed):
    """Rows whose fields repeat (several features of one field) and, now and then, a feature
    twice in one row."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, NF, size=(B, F)).astype(np.int32)
    fld = rng.integers(0, NFLD, size=(B, F)).astype(np.int32)
    idx[::5, 1] = idx[::5, 0]                       # a repeated feature
    val = rng.uniform(0.5, 2.0, size=(B, F)).astype(np.float32)
    y = np.where(rng.random(B) < 0.4, 1.0, -1.0).astype(np.float32)
    return idx, fld, val, y


@pytest.mark.parametrize("adagrad", ["", "-elementwise_adagrad"])
def test_ffm_cpu_engine_matches_oracle_multihot_fields(adagrad):
    """field:index:value rows with repeated fields: each (feature, field)
    address is updated once per row with the summed gradient of every pair that maps to it."""
    B, F, NF, NFLD = 40, 7, 32, 3
    idx, fld, val, y = _multihot_rows(B, F, NF, NFLD, 11)
    assert any(len(set(r)) < F for r in fld)
    t = _trainer("cpu", NF, NFLD, extra="-w0 " + adagrad)
    ref = _np_state(t)
    h = t.hyper
    hp = dict(eta0=h.eta0, eps=h.eps, lambda_v=h.lambda_v, alpha=h.alpha, beta=h.beta,
              lambda1=h.lambda1, lambda2=h.lambda2)
    ref_loss, _ = ffm_train_rows(ref, idx, y, hp, fld=fld, val=val, use_bias=True)
    loss = torch.empty(B)
    ffm_step(t.state, torch.from_numpy(idx), torch.from_numpy(fld), torch.from_numpy(val),
             torch.from_numpy(y), h, loss=loss)
    np.testing.assert_allclose(loss.numpy(), ref_loss, rtol=2e-4, atol=2e-5)
    for k in ("V", "G", "w", "wz", "wn", "bias"):
        np.testing.assert_allclose(t.state[k].numpy(), ref[k], rtol=2e-4, atol=2e-5, err_msg=k)


def test_ffm_oracle_row_gradient_is_the_objective_gradient():
    """fp64 autograd of one row's FFM objective (logistic loss of p plus lambda_v/2 |V|^2 over
    the addresses the row touches) equals the oracle's per-address gradient, repeated fields
    and a repeated feature included."""
    from tests.oracle.ffm_oracle import row_grads

    rng = np.random.default_rng(3)
    F, NF, NFLD, K = 6, 7, 3, 4
    ii = np.array([0, 1, 2, 0, 3, 4])                 # feature 0 twice
    ff = np.array([0, 1, 1, 2, 1, 0])                 # fields 0 and 1 repeated
    xx = rng.uniform(0.5, 2.0, size=F)
    y, lam = 1.0, 0.01
    V = torch.tensor(rng.normal(size=(NF, NFLD, K)), dtype=torch.float64, requires_grad=True)
    p = sum((V[ii[a], ff[b]] * V[ii[b], ff[a]]).sum() * xx[a] * xx[b]
            for a in range(F) for b in range(a + 1, F))
    touched = sorted({(int(ii[a]), int(ff[b])) for a in range(F) for b in range(F) if a != b})
    reg = 0.5 * lam * sum((V[i, f] ** 2).sum() for i, f in touched)
    loss = torch.nn.functional.softplus(-y * p) + reg
    loss.backward()
    kappa = float(-y / (1 + torch.exp(y * p)))
    Vn = V.detach().numpy()
    g = row_grads(lambda i, f: Vn[i, f], ii, ff, xx, kappa, lam)
    assert sorted(g) == touched
    for (i, f), gv in g.items():
        np.testing.assert_allclose(gv, V.grad[i, f].numpy(), rtol=1e-10, atol=1e-12)
    # untouched addresses get no gradient
    mask = np.ones((NF, NFLD), bool)
    for i, f in touched:
        mask[i, f] = False
    assert np.abs(V.grad.numpy()[mask]).max() == 0.0


def _to_packed(t):
    """Copy a trainer's split V/G tables into the packed [NF, NFLD, 2, Kp] layout."""
    NF, NFLD, kp = t.state["V"].shape
    V, G = new_state_tables(NF, NFLD, kp, t.state["V"].dtype, t.state["V"].device, packed=True)
    V.copy_(t.state["V"])
    G.copy_(t.state["G"])
    t.state["V"], t.state["G"] = V, G
    assert is_packed(V, G)


@pytest.mark.parametrize("k", [4, 8])
def test_ffm_packed_layout_matches_split_cpu(k):
    """The packed V|G slot layout (GPU default) runs the same arithmetic as split tables."""
    rng = np.random.default_rng(2)
    B, F, NF = 64, 6, 48
    idx = torch.from_numpy(rng.integers(0, NF, size=(B, F)).astype(np.int32))
    val = torch.from_numpy(rng.uniform(0.5, 2.0, size=(B, F)).astype(np.float32))
    y = torch.from_numpy(np.where(rng.random(B) < 0.4, 1.0, -1.0).astype(np.float32))
    a = _trainer("cpu", NF, F, k=k, extra="-w0 -elementwise_adagrad")
    b = _trainer("cpu", NF, F, k=k, extra="-w0 -elementwise_adagrad")
    _to_packed(b)
    la, lb = torch.empty(B), torch.empty(B)
    ffm_step(a.state, idx, None, val, y, a.hyper, loss=la)
    ffm_step(b.state, idx, None, val, y, b.hyper, loss=lb)
    assert torch.equal(la, lb)
    for key in ("V", "G", "w", "wz", "wn", "bias"):
        assert torch.equal(a.state[key], b.state[key].contiguous()), key
    assert b.state_dict()["V"].is_contiguous()


@pytest.mark.parametrize("k", [4, 8])
def test_ffm_slot_block_layout_matches_split_cpu(k):
    """Per-slot G in the GPU's feature-block layout ([V | G | tail] per feature, line-padded)
    runs the same arithmetic as separate V / G tables; the block's pad slots and tail stay 0."""
    from hivemall_amd.ops.ffm import slot_block_layout

    rng = np.random.default_rng(4)
    B, F, NF = 64, 6, 48
    idx = torch.from_numpy(rng.integers(0, NF, size=(B, F)).astype(np.int32))
    val = torch.from_numpy(rng.uniform(0.5, 2.0, size=(B, F)).astype(np.float32))
    y = torch.from_numpy(np.where(rng.random(B) < 0.4, 1.0, -1.0).astype(np.float32))
    a = _trainer("cpu", NF, F, k=k, extra="-w0")
    b = _trainer("cpu", NF, F, k=k, extra="-w0")
    V, G = new_state_tables(NF, F, a.kp, torch.float32, "cpu", packed=True, slot_g=True)
    V.copy_(b.state["V"])
    G.copy_(b.state["G"])
    b.state["V"], b.state["G"] = V, G
    fs, bs, goff = slot_block_layout(F, a.kp, torch.float32)
    assert V.stride(0) * 4 == bs and G.data_ptr() - V.data_ptr() == goff and bs % 128 == 0
    la, lb = torch.empty(B), torch.empty(B)
    for _ in range(2):
        ffm_step(a.state, idx, None, val, y, a.hyper, loss=la)
        ffm_step(b.state, idx, None, val, y, b.hyper, loss=lb)
    assert torch.equal(la, lb)
    for key in ("V", "G", "w", "wz", "wn", "bias"):
        assert torch.equal(a.state[key], b.state[key].contiguous()), key


def test_ffm_adagrad_state_converts_between_forms_cpu():
    """A per-element checkpoint loads into a per-slot trainer as the sum over the factors
    (the per-slot accumulator is that sum) and vice versa (spread evenly)."""
    a = _trainer("cpu", 16, 4, extra="-elementwise_adagrad")
    a.state["G"].uniform_(0, 1)
    sd = a.state_dict()
    b = FFMTrainer("-classification -factors 4 -seed 3", device="cpu")
    b.load_state_dict(sd)
    assert b.state["G"].shape == (16, 4)
    assert torch.allclose(b.state["G"], a.state["G"].sum(-1))
    c = FFMTrainer("-classification -factors 4 -seed 3 -elementwise_adagrad", device="cpu")
    c.load_state_dict(b.state_dict())
    assert c.state["G"].shape == (16, 4, 4)
    assert torch.allclose(c.state["G"].sum(-1), b.state["G"])


def test_ffm_fields_and_padding_cpu():
    rows = [["0:1:1.0", "1:5:0.5", "2:7"], ["0:2", "2:3:2.0"], ["1:1"]]
    t = FFMTrainer("-c -factors 3 -seed 1", device="cpu")
    b = t.prepare(rows, [1, 0, 1])
    assert b.idx.shape == (3, 3) and (b.idx[1:, 2] == -1).all() or b.idx[2, 1] == -1
    t.fit(batch=b)
    tab = t.model_table()
    assert list(tab.columns) == ["model_id", "i", "Wi", "Vi"]
    assert tab.iloc[0]["i"] == -1
    lin = tab[tab["Vi"].isna() & (tab["i"] >= 0)]
    assert set(lin["i"].tolist()) == {1, 2, 3, 5, 7}
    vrows = tab[tab["Vi"].notna()]
    assert len(vrows) == 5 * t.num_fields and len(vrows.iloc[0]["Vi"]) == 3


def test_ffm_learns_criteo_like_cpu():
    idx, y = criteo_like(20000, hash_bits=16, seed=5)
    t = FFMTrainer("-classification -factors 4 -num_fields 39 -feature_hashing 16 -iters 1 -seed 1 -w0",
                   device="cpu")
    t.fit(batch=FFMBatch(idx, None, None, y))
    eidx, ey, elog = criteo_like(5000, hash_bits=16, seed=77, return_logit=True)
    p = t.predict_raw(batch=FFMBatch(eidx, None, None, None))
    yy = (ey > 0).float()
    ll = torch.nn.functional.binary_cross_entropy_with_logits(p, yy).item()
    base = torch.nn.functional.binary_cross_entropy(yy.mean().expand_as(yy), yy).item()
    assert ll < base, (ll, base)
    assert len(t.cv.history) >= 1


def test_train_ffm_udtf_strings():
    rows = [["0:a:1", "1:b:1"], ["0:c:1", "1:b:1"], ["0:a:1", "1:d:1"]] * 5
    tab = train_ffm(rows, [1, 0, 1] * 5, "-c -feature_hashing 8 -num_fields 4 -iters 2", device="cpu")
    assert (tab["Vi"].isna()).sum() == 5  # bias row + 4 hashed features (a,b,c,d)


@pytest.mark.gpu
@pytest.mark.parametrize("adagrad", ["", "-elementwise_adagrad"])
@pytest.mark.parametrize("layout,reload,k", [("packed", True, 4), ("packed", False, 4),
                                             ("split", True, 4), ("packed", True, 8),
                                             ("packed", False, 8)])
def test_ffm_gpu_matches_cpu_engine(layout, reload, k, adagrad):
    """HIP kernels vs the sequential C++ engine: identical on rows with disjoint features (no
    Hogwild interaction).  Per-slot AdaGrad (default): the pipelined sg32 kernel on the
    feature-block layout (k = 4: 16-B slots; k = 8: 32-B slots, 512-thread blocks), the generic
    kernel for split tables; per-element
    (-elementwise_adagrad): the packed-slot and split-table kernels, with and without reload."""
    torch.manual_seed(0)
    B, F, NFLD = 512, 39, 39
    B_NF = B * F
    idx = torch.arange(B * F, dtype=torch.int32).reshape(B, F)  # all features distinct
    y = torch.where(torch.rand(B) < 0.3, 1.0, -1.0)
    val = torch.rand(B, F) + 0.5
    tc = _trainer("cpu", B_NF, NFLD, k=k, extra=adagrad)
    tg = _trainer("cuda", B_NF, NFLD, k=k, extra=adagrad + (" -split_state" if layout == "split" else ""))
    if adagrad:
        assert is_packed(tg.state["V"], tg.state["G"]) == (layout == "packed")
    else:
        assert tg.state["V"].is_contiguous() == (layout == "split")
    tg.hyper.reload = reload
    for key in tc.state:
        tg.state[key].copy_(tc.state[key].cuda())
    lc = torch.empty(B)
    lg = torch.empty(B, device="cuda")
    ffm_step(tc.state, idx, None, val, y, tc.hyper, loss=lc)
    ffm_step(tg.state, idx.cuda(), None, val.cuda(), y.cuda(), tg.hyper, loss=lg)
    torch.cuda.synchronize()
    np.testing.assert_allclose(lg.cpu().numpy(), lc.numpy(), rtol=1e-4, atol=1e-5)
    for key in ("V", "G", "w", "wz", "wn"):
        np.testing.assert_allclose(tg.state[key].cpu().numpy(), tc.state[key].numpy(), rtol=1e-4, atol=1e-5,
                                   err_msg=key)


@pytest.mark.gpu
@pytest.mark.parametrize("adagrad", ["", "-elementwise_adagrad"])
@pytest.mark.parametrize("layout", ["packed", "split"])
def test_ffm_gpu_bf16_state_close_to_fp32_engine(layout, adagrad):
    """bf16 stochastic-rounded V (both layouts, both AdaGrad forms) tracks the fp32 sequential
    engine (per-slot G stays fp32; per-element G is bf16 too)."""
    torch.manual_seed(1)
    B, F = 256, 39
    idx = torch.arange(B * F, dtype=torch.int32).reshape(B, F)
    y = torch.where(torch.rand(B) < 0.3, 1.0, -1.0)
    tc = _trainer("cpu", B * F, F, extra=adagrad)
    tg = _trainer("cuda", B * F, F, extra=adagrad + " -bf16_state" + (" -split_state" if layout == "split" else ""))
    assert tg.state["V"].dtype == torch.bfloat16
    for key in tc.state:
        tg.state[key].copy_(tc.state[key].cuda())
    lc = torch.empty(B)
    lg = torch.empty(B, device="cuda")
    ffm_step(tc.state, idx, None, None, y, tc.hyper, loss=lc)
    ffm_step(tg.state, idx.cuda(), None, None, y.cuda(), tg.hyper, loss=lg)
    torch.cuda.synchronize()
    np.testing.assert_allclose(lg.cpu().numpy(), lc.numpy(), rtol=2e-2, atol=2e-3)
    np.testing.assert_allclose(tg.state["V"].float().cpu().numpy(), tc.state["V"].numpy(), rtol=2e-2, atol=2e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("adagrad,k", [("", 4), ("-elementwise_adagrad", 4), ("-w0", 4), ("", 8)])
def test_ffm_gpu_single_block_is_exactly_sequential(adagrad, k):
    """grid=1: one workgroup walks the rows in order = Hivemall's per-row semantics.  The generic
    kernel (variant 1) has no lookahead; the pipelined default DMAs row r+1's slots before row
    r's updates land, and forwards its own updates into the slots both rows hold (ffm.hip
    ffm_pipe_sg32_kernel): on rows without a repeated feature, 3e-8 / 6e-8 from the sequential
    engine (profiles/r5/pytest_ffm_q.log; 2.05e-3 before the forwarding,
    profiles/r4/ffm_single_block_forwarding.log)."""
    from hivemall_amd.models import ffm as ffm_model
    from hivemall_amd.ops import ffm as ffm_op

    idx, y = criteo_like(20000, hash_bits=16, seed=5)
    eidx, ey = criteo_like(5000, hash_bits=16, seed=99)
    # field-disjoint ids (field f owns [1024 f, 1024 f + 1024)): no row repeats a feature, so no
    # row is deferred to the grouped-update kernel -- a deferred (multi-hot) row trains after its
    # batch's other rows, a reordering that moved this logloss by -4e-4 at 2^16 hashed ids
    # (~1 % of the rows hold a hash collision; profiles/r5/pytest_ffm_q.log)
    fid = torch.arange(39, dtype=idx.dtype)
    idx = idx % 1024 + fid * 1024
    eidx = eidx % 1024 + fid * 1024
    yy = (ey > 0).float()
    res = {}
    old = ffm_op._VARIANT, ffm_model.RAMP_ROWS
    ffm_model.RAMP_ROWS = 0          # the store kernel itself, not the learner's atomic ramp
    try:
        for dev, v in (("cpu", 0), ("cuda", 1), ("cuda", 0)):
            ffm_op._VARIANT = v
            t = FFMTrainer(f"-classification -factors {k} -num_fields 39 -feature_hashing 16 -seed 1 "
                           + adagrad, device=dev)
            t.grid = 1
            t.fit(batch=FFMBatch(idx, None, None, y).to(dev))
            p = t.predict_raw(batch=FFMBatch(eidx, None, None, None).to(dev)).cpu()
            res[(dev, v)] = torch.nn.functional.binary_cross_entropy_with_logits(p, yy).item()
    finally:
        ffm_op._VARIANT, ffm_model.RAMP_ROWS = old
    print("single-block", adagrad, res)
    assert abs(res[("cpu", 0)] - res[("cuda", 1)]) < 1e-4, res
    assert abs(res[("cpu", 0)] - res[("cuda", 0)]) < 1e-4, res


@pytest.mark.gpu
def test_ffm_gpu_single_block_multihot_rows_train_in_order():
    """with -grid 1 (one block = the sequential learner) a batch holding multi-hot rows
    (hashed collisions at 2^12 ids: many rows repeat a feature) is trained in row order by the
    generic kernel instead of deferring those rows to after the batch, so it equals the CPU
    engine on exactly the rows the pipelined-kernel exactness test has to avoid."""
    from hivemall_amd.models import ffm as ffm_model
    from hivemall_amd.ops import ffm as ffm_op

    idx, y = criteo_like(6000, hash_bits=12, seed=5)
    eidx, ey = criteo_like(3000, hash_bits=12, seed=99)
    assert ffm_op._has_multihot(idx, None)
    yy = (ey > 0).float()
    res = {}
    old = ffm_model.RAMP_ROWS
    ffm_model.RAMP_ROWS = 0
    try:
        for dev in ("cpu", "cuda"):
            t = FFMTrainer("-classification -factors 4 -num_fields 39 -feature_hashing 12 -seed 1", device=dev)
            t.grid = 1
            t.fit(batch=FFMBatch(idx, None, None, y).to(dev))
            p = t.predict_raw(batch=FFMBatch(eidx, None, None, None).to(dev)).cpu()
            res[dev] = torch.nn.functional.binary_cross_entropy_with_logits(p, yy).item()
    finally:
        ffm_model.RAMP_ROWS = old
    assert abs(res["cpu"] - res["cuda"]) < 1e-4, res


def test_ffm_multihot_detection():
    from hivemall_amd.ops.ffm import _has_multihot

    idx = torch.tensor([[1, 2, 3], [4, 5, 6]], dtype=torch.int32)
    assert not _has_multihot(idx, None)
    assert _has_multihot(torch.tensor([[1, 2, 1]], dtype=torch.int32), None)
    assert not _has_multihot(torch.tensor([[1, -1, -1]], dtype=torch.int32), None)   # padding
    fld = torch.tensor([[0, 1, 2], [0, 0, 1]], dtype=torch.int32)
    assert _has_multihot(idx, fld)
    assert not _has_multihot(idx, fld[:1].repeat(2, 1))


@pytest.mark.gpu
def test_ffm_gpu_global_bias_loses_no_updates():
    """-w0: every block updates the one global bias; its FTRL state (z0, n0) is accumulated
    atomically, so n0 = sum over rows of the squared row gradient |kappa| = 1 - exp(-loss)
    (a plain read-modify-write from thousands of blocks loses most of them), and the cached
    w0 = f(z0, n0)."""
    torch.manual_seed(0)
    B, F = 4096, 8
    idx = torch.arange(B * F, dtype=torch.int32).reshape(B, F).cuda()   # only the bias is shared
    y = torch.where(torch.rand(B) < 0.3, 1.0, -1.0).cuda()
    t = _trainer("cuda", B * F, F, extra="-w0")
    loss = torch.empty(B, device="cuda")
    ffm_step(t.state, idx, None, None, y, t.hyper, loss=loss)
    b = t.state["bias"].cpu().double()
    n_rows = ((1 - torch.exp(-loss.double())) ** 2).sum().item()
    assert n_rows > 100 and abs(b[2].item() - n_rows) / n_rows < 1e-3, (b[2].item(), n_rows)
    w0 = -b[1].item() / ((t.hyper.beta + b[2].sqrt().item()) / t.hyper.alpha)
    assert abs(b[0].item() - w0) < 1e-5


@pytest.mark.gpu
def test_ffm_gpu_hogwild_logloss_parity_with_sequential():
    """Full-chip Hogwild vs the sequential engine at 500 K rows (an early-training regime, where
    concurrent read-modify-writes of the hot slots lose the most): the generic kernel (no
    lookahead, ~1,000 rows in flight) measured 0.0117, the pipelined kernel 0.0195-0.0221
    (profiles/ffm_r3/hogwild_probe.log, profiles/r4/ffm_early_grid_curve.jsonl); the learner's
    default atomic-update ramp over the first 2^18 rows 0.0026.  With the linear records in the
    feature blocks the generic kernel measured 0.0152-0.0165 (one 16-B record access or three 4-B
    words alike) against 0.0121-0.0124 with separate linear arrays, the pipelined 0.0215 vs
    0.0195-0.0199: the cost is the layout (round 6, profiles/r6/ffm_generic_lin_layout.jsonl;
    docs/compat.md "Test bounds"), which the headline keeps for +19 % rows/s.
    At the bench's 12.6 M rows the gap is +2.5e-3 .. +2.8e-3 (test_ffm_gpu_bench_scale_parity_pinned).
    Bounds = measurement + margin."""
    from hivemall_amd.models import ffm as ffm_model
    from hivemall_amd.ops import ffm as ffm_op

    idx, y = criteo_like(500000, hash_bits=20, seed=5)
    eidx, ey = criteo_like(100000, hash_bits=20, seed=99)
    yy = (ey > 0).float()
    res = {}
    old = ffm_op._VARIANT, ffm_model.RAMP_ROWS
    try:
        # (device, kernel variant, early-training ramp rows)
        for dev, v, ramp in (("cpu", 0, 0), ("cuda", 1, 0), ("cuda", 0, 0), ("cuda", 0, 1 << 18)):
            ffm_op._VARIANT = v
            ffm_model.RAMP_ROWS = ramp
            t = FFMTrainer("-classification -factors 4 -num_fields 39 -feature_hashing 20 -seed 1",
                           device=dev)
            t.fit(batch=FFMBatch(idx, None, None, y).to(dev))
            ffm_op._VARIANT = 0
            p = t.predict_raw(batch=FFMBatch(eidx, None, None, None).to(dev)).cpu()
            res[(dev, v, ramp)] = torch.nn.functional.binary_cross_entropy_with_logits(p, yy).item()
    finally:
        ffm_op._VARIANT, ffm_model.RAMP_ROWS = old
    seq = res[("cpu", 0, 0)]
    assert abs(seq - res[("cuda", 1, 0)]) < 0.021, res
    assert abs(seq - res[("cuda", 0, 0)]) < 0.026, res
    # the learner's default: the first 2^18 rows through the atomic-update kernel (measured
    # 0.0026, profiles/r4/ffm_early_ramp_atomic.jsonl)
    assert abs(seq - res[("cuda", 0, 1 << 18)]) < 0.006, res


# Held-out logloss of the sequential C++ engine (per-slot AdaGrad, fp32) on bench.py's exact
# 1-rank stream drawn by the CPU generator on the driver's data (criteo_ffm: explicit fields and
# values; 12,582,912 rows; benchmarks/ffm_parity_bench_scale.py, profiles/r4/ffm_parity_bench_scale_ffmdata.log).
SEQ_BENCH_SCALE_LOGLOSS = 0.44501


@pytest.mark.gpu
@pytest.mark.parametrize("state", ["", " -bf16_state"])
def test_ffm_gpu_hot_linear_steps_are_not_lost(state, monkeypatch):
    """The side-table linear mode (HM_FFM_LIN_ATOMIC=4, the default) loses no linear FTRL step at
    full-chip concurrency.  With V frozen (-eta0 0, -lambda 0) and w pinned at 0 (-lambda1 1e9) every
    row's kappa is fixed by the data alone, so whatever order and concurrency the kernel trains in,
    each hot feature (the side table's: the 1,024 most frequent of the batch) must end with z = sum
    of its rows' g and n = sum of g^2 — what the sequential engine computes.  (The other features
    keep plain record stores: a concurrent row can still overwrite one of their steps.)  The plain
    record stores (mode 0) lose most steps of the hot features at this concurrency; the test checks
    that too, so it does not pass vacuously."""
    from hivemall_amd.io.synthetic import criteo_ffm
    from hivemall_amd.ops import ffm as ffm_ops

    idx, fld, val, y = criteo_ffm(65536, hash_bits=20, seed=11)
    single = torch.tensor([len(set(r)) == len(r) for r in idx.tolist()])   # no multi-hot rows
    idx, fld, val, y = idx[single], fld[single], val[single], y[single]
    opts = "-eta0 0 -lambda 0 -lambda1 1e9 -num_fields 39" + state
    tc = _trainer("cpu", 1 << 20, 39, extra=opts)
    tgs = {m: _trainer("cuda", 1 << 20, 39, extra=opts) for m in ("4", "0")}
    for tg in tgs.values():
        _copy_state(tc, tg)                 # the same (bf16-rounded) V everywhere
    ffm_step(tc.state, idx, fld, val, y, tc.hyper)
    n_ref = tc.state["wn"].double()
    z_ref = tc.state["wz"].double()
    cnt = torch.bincount(idx.reshape(-1).long(), minlength=1 << 20)
    top = torch.argsort(cnt, descending=True)[:512]
    res = {}
    # two launches with the hot set rebuilt at each (HM_FFM_LIN_HOT_REFRESH 1): every record holds
    # its folded state between launches, so the rebuild loses nothing
    monkeypatch.setattr(ffm_ops, "_LIN_HOT_REFRESH", 1)
    half = idx.shape[0] // 2
    for mode, tg in tgs.items():
        monkeypatch.setattr(ffm_ops, "_LIN_ATOMIC", int(mode))
        ffm_ops._LIN_HOT.clear()
        for sl in (slice(0, half), slice(half, None)):
            ffm_step(tg.state, idx[sl].cuda(), fld[sl].cuda(), val[sl].cuda(), y[sl].cuda(), tg.hyper)
        torch.cuda.synchronize()
        res[mode] = (tg.state["wn"].double().cpu(), tg.state["wz"].double().cpu(), tg.state["w"].cpu())
    n4, z4, w4 = res["4"]
    assert float(w4.abs().max()) == 0.0
    hot = torch.argsort(cnt, descending=True)[:768]       # in both launches' side tables
    np.testing.assert_allclose(n4[hot].numpy(), n_ref[hot].numpy(), rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(z4[hot].numpy(), z_ref[hot].numpy(), rtol=2e-3,
                               atol=2e-3 * float(z_ref[hot].abs().max()))
    n0 = res["0"][0]
    assert float((n0[top] / n_ref[top]).median()) < 0.5   # plain stores: most hot steps lost


@pytest.mark.gpu
def test_ffm_gpu_bench_scale_parity_pinned():
    """The bench-scale parity record as a test, on the headline's own data: bench.py
    --gen-device cpu trains the same 12.6 M-row criteo_ffm stream (48 steps over 8 resident
    batches) as the sequential engine's reference run.  The same kernel on one block reproduces
    0.44501 exactly (profiles/r5/ffm_stream_gap_src.jsonl).  At full-chip concurrency, with the
    hot features' linear steps in the side table (round 6, no linear step lost), the fp32 run
    measures +1.85e-3 and bf16 +2.33e-3 (profiles/r6/linhot/); what is left is lost V-slot
    updates, which grow with the epochs over the resident batches (the host model,
    benchmarks/ffm_hogwild_sim.py: +0.8e-3 of slot gap after 25 steps, +2.0e-3 after 48).  Bounds:
    fp32 2.5e-3 (SURVEY's 1e-3 is met on the driver's 25-step stream, +0.96e-3, not on this one),
    bf16 3e-3 (SURVEY's bf16 tolerance).  Before the side table: fp32 +2.5e-3 .. +2.8e-3, bf16
    +4.0e-3 .. +4.3e-3 (round 5)."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gen-device", "cpu",
                        "--data", "criteo_ffm", "--full"],
                       capture_output=True, text=True, timeout=110, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["rows_trained_per_rank"] == 12582912 and rec["dtype"] == "fp32"
    assert rec["config"]["early_ramp_warmup_steps"] == 1
    assert rec["config"]["linear_steps"] == "side-table"   # one rank keeps every hot linear step
    assert -1.0e-3 <= rec["logloss_heldout"] - SEQ_BENCH_SCALE_LOGLOSS <= 2.5e-3, rec["logloss_heldout"]
    assert abs(rec["logloss_heldout_bf16"] - SEQ_BENCH_SCALE_LOGLOSS) <= 3e-3, rec["logloss_heldout_bf16"]


def _copy_state(tc, tg, rows=None):
    """CPU trainer state -> GPU state (rows ``rows`` of the GPU tables when given), then the CPU
    state <- the GPU's stored values (the same bf16-rounded start for both engines)."""
    for k in tc.state:
        dst = tg.state[k] if rows is None or k == "bias" else tg.state[k][rows]
        dst.copy_(tc.state[k].to(dst.device))
        tc.state[k].copy_(dst.float().cpu())


def _assert_state_close(tc, tg, tol, rows=None):
    for k in ("V", "G", "w", "wz", "wn"):
        a = tg.state[k] if rows is None else tg.state[k][rows]
        np.testing.assert_allclose(a.float().cpu().numpy(), tc.state[k].numpy(), rtol=tol,
                                   atol=tol * 1e-1, err_msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize("lpack", ["1", "0"])
@pytest.mark.parametrize("extra,tol,k", [("", 1e-4, 4), (" -bf16_state", 2e-2, 4), ("", 1e-4, 8)])
def test_ffm_gpu_explicit_fields_and_values_match_cpu_engine(extra, tol, k, lpack, monkeypatch):
    """field:index:value rows as the SQL / UDTF path hands them to the kernel: an explicit
    field id per feature (every row a random permutation of the 39 fields) and random values,
    through the pipelined sg32 (fp32) and sg12 (bf16) kernels vs the sequential C++ engine on
    disjoint-feature rows.  (Rows with a repeated field: test_ffm_gpu_multihot_rows_match_cpu_engine.)
    lpack "0": the linear records in the feature blocks accessed as three 4-B words instead of
    one 16-B record (the bf16 kernel's block-tail zeroing must skip them either way)."""
    monkeypatch.setenv("HM_FFM_LPACK", lpack)
    g = torch.Generator().manual_seed(7)
    B, F = 384, 39
    idx = torch.arange(B * F, dtype=torch.int32).reshape(B, F)
    fld = torch.stack([torch.randperm(F, generator=g) for _ in range(B)]).to(torch.int32)
    val = torch.rand(B, F, generator=g) * 3.0 + 0.1
    y = torch.where(torch.rand(B, generator=g) < 0.3, 1.0, -1.0)
    tc = _trainer("cpu", B * F, F, k=k)
    tg = _trainer("cuda", B * F, F, k=k, extra=extra)
    _copy_state(tc, tg)
    lc, lg = torch.empty(B), torch.empty(B, device="cuda")
    ffm_step(tc.state, idx, fld, val, y, tc.hyper, loss=lc)
    ffm_step(tg.state, idx.cuda(), fld.cuda(), val.cuda(), y.cuda(), tg.hyper, loss=lg)
    torch.cuda.synchronize()
    np.testing.assert_allclose(lg.cpu().numpy(), lc.numpy(), rtol=1e-4, atol=1e-5)
    _assert_state_close(tc, tg, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("extra,tol", [("", 1e-4), (" -bf16_state", 2e-2), (" -elementwise_adagrad", 1e-4)])
def test_ffm_gpu_multihot_rows_match_cpu_engine(extra, tol):
    """Rows with repeated fields (39 features over 10 fields) and, in every 4th row, one feature
    twice: the pipelined kernels defer these rows to the grouped-update kernel, which updates
    each (feature, field) address once with the summed gradient, as the C++ engine and the
    oracle do.  Rows use disjoint features, so the Hogwild order does not matter; every 3rd row
    has distinct fields and takes the pipelined path in the same launch."""
    g = torch.Generator().manual_seed(17)
    B, F, NFLD = 384, 39, 39
    idx = torch.arange(B * F, dtype=torch.int32).reshape(B, F)
    idx[::4, 5] = idx[::4, 2]
    fld = torch.randint(0, 10, (B, F), generator=g, dtype=torch.int32)
    fld[::3] = torch.stack([torch.randperm(F, generator=g) for _ in range(B)])[::3].to(torch.int32)
    val = torch.rand(B, F, generator=g) * 3.0 + 0.1
    y = torch.where(torch.rand(B, generator=g) < 0.3, 1.0, -1.0)
    tc = _trainer("cpu", B * F, NFLD, extra=extra)
    tg = _trainer("cuda", B * F, NFLD, extra=extra)
    _copy_state(tc, tg)
    lc, lg = torch.empty(B), torch.empty(B, device="cuda")
    for _ in range(2):
        ffm_step(tc.state, idx, fld, val, y, tc.hyper, loss=lc)
        ffm_step(tg.state, idx.cuda(), fld.cuda(), val.cuda(), y.cuda(), tg.hyper, loss=lg)
    torch.cuda.synchronize()
    np.testing.assert_allclose(lg.cpu().numpy(), lc.numpy(), rtol=max(tol, 1e-4), atol=1e-5 if tol < 1e-3 else 2e-3)
    _assert_state_close(tc, tg, tol)


@pytest.mark.gpu
def test_ffm_gpu_bf16_rows_wider_than_45_features():
    """-bf16_state keeps 12-B {V | G} slots for any row width; rows of more than 45 features
    (beyond the pipelined kernel's LDS image) take the generic kernel on the same layout."""
    g = torch.Generator().manual_seed(8)
    B, F = 96, 46
    idx = torch.arange(B * F, dtype=torch.int32).reshape(B, F)
    val = torch.rand(B, F, generator=g) + 0.5
    y = torch.where(torch.rand(B, generator=g) < 0.3, 1.0, -1.0)
    tc = _trainer("cpu", B * F, F)
    tg = _trainer("cuda", B * F, F, extra=" -bf16_state")
    assert tg.state["G"].stride(1) == 3                 # the 12-B slot layout
    _copy_state(tc, tg)
    lc, lg = torch.empty(B), torch.empty(B, device="cuda")
    for _ in range(2):
        ffm_step(tc.state, idx, None, val, y, tc.hyper, loss=lc)
        ffm_step(tg.state, idx.cuda(), None, val.cuda(), y.cuda(), tg.hyper, loss=lg)
    torch.cuda.synchronize()
    np.testing.assert_allclose(lg.cpu().numpy(), lc.numpy(), rtol=2e-2, atol=2e-3)
    _assert_state_close(tc, tg, 2e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("lin", ["arrays", "records"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_ffm_gpu_tables_of_4gib_and_more(dtype, lin):
    """-feature_hashing 23: the bf16 12-B slot table is 4 GiB and the fp32 block table 7.5 GiB,
    past the 32-bit slot offsets; the pipelined kernels switch to 64-bit offsets.  The rows use
    features at the top of the id range (offsets > 4 GiB) and must match the sequential engine
    run on a small table holding the same rows.  lin "records": the linear state in the feature
    blocks (the learner's layout), where the side-table linear mode applies on 32-bit launches —
    the 64-bit launches keep plain record stores, so no side-table copy may wrap them."""
    g = torch.Generator().manual_seed(9)
    B, F, NF = 256, 39, 1 << 23
    base = NF - B * F
    idx = torch.arange(B * F, dtype=torch.int32).reshape(B, F)
    val = torch.rand(B, F, generator=g) + 0.5
    y = torch.where(torch.rand(B, generator=g) < 0.3, 1.0, -1.0)
    tc = _trainer("cpu", B * F, F)
    tg = FFMTrainer("-classification -factors 4 -seed 3" + (" -bf16_state" if dtype == torch.bfloat16 else ""),
                    device="cuda")
    V, G = new_state_tables(NF, F, 4, dtype, "cuda", packed=True, slot_g=True)
    z = lambda: torch.zeros(NF, dtype=torch.float32, device="cuda")  # noqa: E731
    if lin == "records":
        from hivemall_amd.ops.ffm import lin_record_views
        w, wz, wn = lin_record_views(V, G)
        tg.state = dict(V=V, G=G, w=w, wz=wz, wn=wn, bias=torch.zeros(4, device="cuda"))
    else:
        tg.state = dict(V=V, G=G, w=z(), wz=z(), wn=z(), bias=torch.zeros(4, device="cuda"))
    rows = slice(base, NF)
    _copy_state(tc, tg, rows)
    lc, lg = torch.empty(B), torch.empty(B, device="cuda")
    ffm_step(tc.state, idx, None, val, y, tc.hyper, loss=lc)
    ffm_step(tg.state, (idx + base).cuda(), None, val.cuda(), y.cuda(), tc.hyper, loss=lg)
    torch.cuda.synchronize()
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-4
    np.testing.assert_allclose(lg.cpu().numpy(), lc.numpy(), rtol=1e-4, atol=1e-5)
    _assert_state_close(tc, tg, tol, rows)
    assert float(tg.state["V"][:base].abs().amax()) == 0.0            # nothing else written
    del tg, V, G
    torch.cuda.empty_cache()


def test_ffm_engine_options_grid_and_atomic_rows():
    """train_ffm -grid / -atomic_rows (docs/compat.md: the Hogwild quality / speed knobs) reach the
    learner; the -atomic_rows default is the module's RAMP_ROWS read at construction."""
    from hivemall_amd.models import ffm as ffm_model

    t = FFMTrainer("-c -factors 4 -num_fields 39 -feature_hashing 10 -grid 4 -atomic_rows 1000", device="cpu")
    assert (t.grid, t.atomic_rows) == (4, 1000)
    old = ffm_model.RAMP_ROWS
    try:
        ffm_model.RAMP_ROWS = 12345
        t = FFMTrainer("-c -factors 4 -num_fields 39 -feature_hashing 10", device="cpu")
        assert (t.grid, t.atomic_rows) == (0, 12345)
    finally:
        ffm_model.RAMP_ROWS = old


def test_ffm_step_rejects_retired_variants_and_linear_modes(monkeypatch):
    """A retired or never-assigned kernel variant / linear mode is a ValueError on any device (it
    used to run the default silently), whether it comes from the argument or from the environment's
    module default; the live values run."""
    from hivemall_amd.ops import ffm as ffm_ops

    t = _trainer("cpu", nf=8, nfld=3)
    idx = torch.tensor([[0, 3, 6], [1, 4, 7]], dtype=torch.int32)
    y = torch.tensor([1.0, -1.0])
    for v in (2, 3, 8, 9, 10, 7):
        with pytest.raises(ValueError, match="0, 1, 6, 11"):
            ffm_step(t.state, idx, None, None, y, t.hyper, variant=v)
        monkeypatch.setattr(ffm_ops, "_VARIANT", v)
        with pytest.raises(ValueError, match="0, 1, 6, 11"):
            ffm_step(t.state, idx, None, None, y, t.hyper)
        monkeypatch.setattr(ffm_ops, "_VARIANT", 0)
    for m in (1, 2, 3):
        with pytest.raises(ValueError, match="0, 4"):
            ffm_step(t.state, idx, None, None, y, t.hyper, lin_mode=m)
        monkeypatch.setattr(ffm_ops, "_LIN_ATOMIC", m)
        with pytest.raises(ValueError, match="0, 4"):
            ffm_step(t.state, idx, None, None, y, t.hyper)
        monkeypatch.setattr(ffm_ops, "_LIN_ATOMIC", 4)
    for v in (0, 1, 6, 11):
        ffm_step(t.state, idx, None, None, y, t.hyper, variant=v)
    for m in (0, 4):
        ffm_step(t.state, idx, None, None, y, t.hyper, lin_mode=m)
