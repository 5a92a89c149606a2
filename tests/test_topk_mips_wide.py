"""Fused top-k for k = 65..256 (csrc/kernels/topk_mips_wide.hip through mips_topk,
recommend_topk and topk_similar) against fp64 references: Q.double() @ I.double().T + bias with
a stable argsort, i.e. higher score first and equal scores by lower item index.

Integer operands in -3..3 are exact in bf16 and every partial sum in fp32, so indices and
scores must equal the reference with ==; the fp32 cases add two columns of odd magnitudes
257..1023, which bf16 cannot hold.  The second half of the items repeats the first, so exact
ties cross the threshold.
"""
import functools

import pytest
import torch

from hivemall_amd.ops.topk_mips import exclusion_csr, mips_topk

U24 = 2.0 ** -24
M, N = 131, 517
PRECISIONS = ("bf16", "fp32")


@functools.lru_cache(maxsize=None)
def _int_case(d, precision, n=N):
    g = torch.Generator().manual_seed(2000 + d)
    Q = torch.randint(-3, 4, (M, d), generator=g).float()
    I = torch.randint(-3, 4, (n, d), generator=g).float()
    if precision == "fp32":
        for T in (Q, I):
            mag = 2 * torch.randint(128, 512, (T.shape[0], 2), generator=g) + 1      # odd, 257..1023
            T[:, :2] = (mag * (2 * torch.randint(0, 2, mag.shape, generator=g) - 1)).float()
    bias = torch.randint(-2, 3, (n,), generator=g).float()
    h = (n + 1) // 2
    I[h:], bias[h:] = I[: n - h], bias[: n - h]
    return Q, I, bias, Q.double() @ I.double().T + bias.double()[None, :]


def _expect(S, k):
    """Top-k of an fp64 score matrix in (score desc, index asc) order, -1 / -inf padded."""
    kk = min(k, S.shape[1])
    o = torch.argsort(S, dim=1, descending=True, stable=True)[:, :kk]
    sc = S.gather(1, o)
    ix = torch.full((S.shape[0], k), -1, dtype=torch.int64)
    out = torch.full((S.shape[0], k), -float("inf"), dtype=torch.float64)
    ix[:, :kk] = torch.where(torch.isinf(sc), torch.full_like(o, -1), o)
    out[:, :kk] = sc
    return ix, out


def _assert_exact(got, S, k):
    wi, ws = _expect(S, k)
    assert torch.equal(got[0].cpu(), wi)
    assert torch.equal(got[1].cpu().double(), ws)


def _assert_within_bound(ix, sc, S, Bmat, extra=0.0):
    """Each score within B of the fp64 score of its index; the j-th score within max_n B of the
    j-th largest fp64 score; distinct indices."""
    ix, sc = ix.cpu(), sc.cpu().double()
    k = ix.shape[1]
    at = S.gather(1, ix)
    assert ((sc - at).abs() <= Bmat.gather(1, ix) + extra * at.abs()).all()
    want = torch.topk(S, k, dim=1).values
    assert ((sc - want).abs() <= Bmat.max(1, keepdim=True).values + extra * want.abs()).all()
    assert all(len(set(r)) == k for r in ix.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k", [65, 100, 128, 129, 256])
@pytest.mark.parametrize("d", [3, 64, 256])
def test_gpu_wide_exact_integer_operands(d, k, precision):
    Q, I, bias, S = _int_case(d, precision)
    for splits in (1, 4):
        got = mips_topk(Q.cuda(), I.cuda(), k, item_bias=bias.cuda(), splits=splits, precision=precision)
        _assert_exact(got, S, k)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_gpu_wide_exclusion_and_self_offset(precision):
    Q, I, bias, S = _int_case(40, precision)
    g = torch.Generator().manual_seed(7)
    ex = exclusion_csr(torch.randint(0, M, (3000,), generator=g), torch.randint(0, N, (3000,), generator=g), M)
    S = S.clone()
    for q in range(M):
        S[q, ex[1][ex[0][q]:ex[0][q + 1]].long()] = -float("inf")
        S[q, q + 2] = -float("inf")
    got = mips_topk(Q.cuda(), I.cuda(), 100, item_bias=bias.cuda(), exclude=tuple(t.cuda() for t in ex),
                    exclude_self_offset=2, precision=precision)
    _assert_exact(got, S, 100)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_gpu_wide_fewer_items_than_k(precision):
    Q, I, bias, S = _int_case(10, precision, 100)
    ix, sc = got = mips_topk(Q.cuda(), I.cuda(), 256, item_bias=bias.cuda(), precision=precision)
    _assert_exact(got, S, 256)
    assert (ix[:, 100:] == -1).all().item() and torch.isinf(sc[:, 100:]).all().item()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("descending", [False, True])
def test_gpu_wide_compaction_under_pressure(descending, precision):
    """score(q, n) = c_q n with c_q in 1..3 (items (n // 64, n % 64) against queries (64 c, c),
    all exact in bf16): ascending, every sub-tile beats the threshold and the buffers compact at
    the highest possible rate; descending, nothing is admitted after the first k."""
    n = torch.arange(4096)
    I = torch.stack([n // 64, n % 64], 1).float()
    if descending:
        I = I.flip(0)
    c = 1 + torch.arange(70) % 3
    Q = torch.stack([64 * c, c], 1).float()
    got = mips_topk(Q.cuda(), I.cuda(), 200, precision=precision)
    _assert_exact(got, Q.double() @ I.double().T, 200)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_gpu_wide_random_operands_within_rounding_bound(precision):
    """d products and d + 1 additions rounded once each: B = (d+2) 2^-24 (|Q||I| + |bias|), for
    bf16 on the operand tables rounded to bf16 (their products are exact in fp32)."""
    d = 64
    g = torch.Generator().manual_seed(3)
    Q, I = torch.randn(200, d, generator=g), torch.randn(3000, d, generator=g)
    bias = torch.randn(3000, generator=g) * 0.1
    if precision == "bf16":
        Q, I = Q.bfloat16().float(), I.bfloat16().float()
    ix, sc = mips_topk(Q.cuda(), I.cuda(), 100, item_bias=bias.cuda(), precision=precision)
    S = Q.double() @ I.double().T + bias.double()[None, :]
    B = (d + 2) * U24 * (Q.double().abs() @ I.double().abs().T + bias.double().abs()[None, :])
    _assert_within_bound(ix, sc, S, B)


@pytest.mark.gpu
def test_gpu_wide_recommend_topk_and_topk_similar():
    """k = 100 through the callers; the fp64 reference is formed from the fp32 state tables."""
    from hivemall_amd.knn import topk_similar
    from hivemall_amd.models.mf import BPRMF, MatrixFactorization

    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5)
    us, its = torch.randint(0, 300, (20000,), generator=g), torch.randint(0, 400, (20000,), generator=g)
    r = torch.randint(1, 6, (20000,), generator=g).float()
    m = MatrixFactorization("-factors 16 -iters 2 -update_mean", device=dev).fit(us, its, r)
    st = {n: t.double().cpu() for n, t in m.state.items() if torch.is_tensor(t)}
    P, Qi = st["P"][:, :16], st["Q"][:, :16]
    S = P @ Qi.T + st["Bi"][None, :] + st["Bu"][:, None] + st["mu"][0]
    B = 18 * U24 * (P.abs() @ Qi.abs().T + st["Bi"].abs()[None, :])
    sc, ix = m.recommend_topk(None, k=100, precision="fp32")
    _assert_within_bound(ix, sc, S, B, extra=2.0 ** -23)

    b = BPRMF("-factors 16 -iters 2", device=dev).fit_implicit(us.to(dev), its.to(dev), 300, 400)
    st = {n: t.double().cpu() for n, t in b.state.items() if torch.is_tensor(t)}
    P, Qi = st["P"][:, :16], st["Q"][:, :16]
    sc, ix = b.recommend_topk(None, k=100, precision="fp32")
    _assert_within_bound(ix, sc, P @ Qi.T + st["Bi"][None, :], 18 * U24 * (P.abs() @ Qi.abs().T + st["Bi"].abs()[None, :]))

    X = torch.randn(300, 24, generator=g)
    sc, ix = topk_similar(X.to(dev), k=100, precision="fp32")
    Xn = torch.nn.functional.normalize(X.double(), dim=1)
    S = Xn @ Xn.T
    S.fill_diagonal_(-float("inf"))
    _assert_within_bound(ix, sc, S, torch.full_like(S, 3 * 26 * U24))
    assert not (ix.cpu() == torch.arange(300)[:, None]).any()


# ----------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("k", [100, 256])
def test_cpu_wide_k(k):
    Q, I, bias, S = _int_case(10, "fp32")
    _assert_exact(mips_topk(Q, I, k, item_bias=bias), S, k)


def test_cpu_k_above_256_raises():
    Q, I, _, _ = _int_case(10, "fp32")
    with pytest.raises(ValueError):
        mips_topk(Q, I, 257)
