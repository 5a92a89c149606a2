"""fp32 operand type of the fused top-k (mips_topk(..., precision="fp32"),
csrc/kernels/topk_mips_f32.hip) against fp64 references.

  * integer operands whose every partial sum stays below 2^24: indices and scores must equal
    the fp64 reference with ==, tie order included.  Two columns hold odd integers of magnitude
    257..1023, which bf16 cannot hold, so the bf16 kernel cannot pass;
  * random fp32 operands, not pre-rounded: the order-independent bound of d products and d + 1
    additions rounded once each,  B(q,n) = (d+2) 2^-24 (sum_k |Q_qk I_nk| + |bias_n|).
"""
import functools

import pytest
import torch

from hivemall_amd.ops.topk_mips import exclusion_csr, mips_topk

U24 = 2.0 ** -24
M, N = 131, 517


@functools.lru_cache(maxsize=None)
def _int_case(d, n=N):
    """(Q, I, bias, fp64 scores): the second half of the items repeats the first (exact ties)."""
    g = torch.Generator().manual_seed(1000 + d)
    Q = torch.randint(-3, 4, (M, d), generator=g).float()
    I = torch.randint(-3, 4, (n, d), generator=g).float()
    for T in (Q, I):
        mag = 2 * torch.randint(128, 512, (T.shape[0], 2), generator=g) + 1          # odd, 257..1023
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
    ix, sc = got
    wi, ws = _expect(S, k)
    assert torch.equal(ix.cpu(), wi)
    assert torch.equal(sc.cpu().double(), ws)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 10, 32, 33, 64])
@pytest.mark.parametrize("d", [3, 10, 64, 100, 256])
def test_gpu_fp32_exact_integer_operands(d, k):
    Q, I, bias, S = _int_case(d)
    for splits in (1, 4):
        got = mips_topk(Q.cuda(), I.cuda(), k, item_bias=bias.cuda(), splits=splits, precision="fp32")
        _assert_exact(got, S, k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 40])
def test_gpu_fp32_exclusion_and_self_offset(k):
    Q, I, bias, S = _int_case(40)
    g = torch.Generator().manual_seed(7)
    ex = exclusion_csr(torch.randint(0, M, (3000,), generator=g), torch.randint(0, N, (3000,), generator=g), M)
    S = S.clone()
    for q in range(M):
        S[q, ex[1][ex[0][q]:ex[0][q + 1]].long()] = -float("inf")
        S[q, q + 2] = -float("inf")
    got = mips_topk(Q.cuda(), I.cuda(), k, item_bias=bias.cuda(), exclude=tuple(t.cuda() for t in ex),
                    exclude_self_offset=2, precision="fp32")
    _assert_exact(got, S, k)


@pytest.mark.gpu
def test_gpu_fp32_fewer_items_than_k():
    Q, I, bias, S = _int_case(10, 20)
    ix, sc = got = mips_topk(Q.cuda(), I.cuda(), 40, item_bias=bias.cuda(), precision="fp32")
    _assert_exact(got, S, 40)
    assert (ix[:, 20:] == -1).all().item() and torch.isinf(sc[:, 20:]).all().item()


def _assert_within_bound(ix, sc, S, Bmat, extra=0.0):
    """Each score within B of the fp64 score of its index; the j-th score within max_n B of the
    j-th largest fp64 score; distinct indices."""
    ix, sc = ix.cpu(), sc.cpu().double()
    k = ix.shape[1]
    at = S.gather(1, ix)
    err = (sc - at).abs()
    tol = Bmat.gather(1, ix) + extra * at.abs()
    print("max score error / bound:", (err / tol).max().item())
    assert (err <= tol).all()
    want = torch.topk(S, k, dim=1).values
    rtol = Bmat.max(1, keepdim=True).values + extra * want.abs()
    assert ((sc - want).abs() <= rtol).all()
    assert all(len(set(r)) == k for r in ix.tolist())


@pytest.mark.gpu
def test_gpu_fp32_random_operands_within_rounding_bound():
    d = 64
    g = torch.Generator().manual_seed(3)
    Q, I = torch.randn(200, d, generator=g), torch.randn(3000, d, generator=g)
    bias = torch.randn(3000, generator=g) * 0.1
    ix, sc = mips_topk(Q.cuda(), I.cuda(), 20, item_bias=bias.cuda(), precision="fp32")
    S = Q.double() @ I.double().T + bias.double()[None, :]
    B = (d + 2) * U24 * (Q.double().abs() @ I.double().abs().T + bias.double().abs()[None, :])
    _assert_within_bound(ix, sc, S, B)


@pytest.mark.gpu
def test_gpu_fp32_recommend_topk_and_topk_similar():
    """The fp64 reference is formed from the fp32 state tables: BPRMF.scores() runs a bf16
    GEMM on the GPU, and MatrixFactorization has no scores()."""
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
    sc, ix = m.recommend_topk(None, k=10, precision="fp32")
    _assert_within_bound(ix, sc, S, B, extra=2.0 ** -23)

    b = BPRMF("-factors 16 -iters 2", device=dev).fit_implicit(us.to(dev), its.to(dev), 300, 400)
    st = {n: t.double().cpu() for n, t in b.state.items() if torch.is_tensor(t)}
    P, Qi = st["P"][:, :16], st["Q"][:, :16]
    sc, ix = b.recommend_topk(None, k=10, precision="fp32")
    _assert_within_bound(ix, sc, P @ Qi.T + st["Bi"][None, :], 18 * U24 * (P.abs() @ Qi.abs().T + st["Bi"].abs()[None, :]))

    X = torch.randn(300, 24, generator=g)
    sc, ix = topk_similar(X.to(dev), k=5, precision="fp32")
    Xn = torch.nn.functional.normalize(X.double(), dim=1)
    S = Xn @ Xn.T
    S.fill_diagonal_(-float("inf"))
    _assert_within_bound(ix, sc, S, torch.full_like(S, 3 * 26 * U24))
    assert not (ix.cpu() == torch.arange(300)[:, None]).any()


# ----------------------------------------------------------------------------- CPU
def test_precision_keyword_on_cpu():
    Q, I, bias, S = _int_case(10)
    with pytest.raises(ValueError):
        mips_topk(Q, I, 5, precision="fp16")
    base = mips_topk(Q, I, 12, item_bias=bias)
    for prec in ("fp32", "bf16"):
        ix, sc = mips_topk(Q, I, 12, item_bias=bias, precision=prec)
        assert torch.equal(ix, base[0]) and torch.equal(sc, base[1])
    _assert_exact(base, S, 12)
