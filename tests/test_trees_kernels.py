"""Kernel-level checks of csrc/kernels/trees.hip: every ``hm_*`` entry point that the learner
tests only reach through whole (self-correcting) ensembles is called directly and compared with
a plain fp64 / integer NumPy or torch reference written from the comment above the kernel.

Kernels with a host twin (csrc/host/trees_cpu.cpp) run the same test on both devices, so the
reference and the argument packing are proven without a GPU before a raw pointer reaches one.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from hivemall_amd import _native
from hivemall_amd.models import trees as T
from hivemall_amd.models.trees import CAT_FLAG, DLEFT_FLAG, HistTreeBuilder, Quantized, quantize

gpu = pytest.mark.gpu
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
p = _native.ptr


def _st():
    return _native.stream_of(torch.device("cuda"))


def _sync():
    torch.cuda.synchronize()


def _bits(a):
    """fp32 array -> its bit patterns (bit-for-bit comparisons, -0.0 != +0.0, NaN == NaN)."""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def _ulp32(x):
    """Spacing of fp32 at |x| (>= the smallest normal's, so a zero reference keeps a finite one)."""
    return np.spacing(np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126).astype(np.float32)).astype(np.float64)


# =============================================================== 1. fused statistics
STATS_N = [1, 255, 257, 262144 + 300]     # one thread, a partial block, two blocks, the grid-stride loop
# tolerance constant of the sigmoid error model (see test_fused_stats_match_fp64)
STATS_C = 4.0


def _stats_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    F = torch.randn(n, generator=g) * 3
    planted = [0.0, -0.0, 30.0, -30.0, 100.0, -100.0]
    pos = [(i * max(1, n // 6) + i) % n for i in range(len(planted))]
    if n == 1:
        pos = pos[:1]
    for i, v in zip(pos, planted):
        F[i] = v
    y = (torch.rand(n, generator=g) < 0.5).float()
    mask = (torch.rand(n, generator=g) >= 0.3).to(torch.uint8)
    return F, y, mask


def _run_stats(kind, F, y, mask):
    """Launch hm_gbt_stats / hm_gbt2_stats / hm_xgb_stats; (stats, smax, hh or None) on the host."""
    n = F.numel()
    NS = 3 if kind == "gbt" else 2
    Fd, yd = F.cuda(), y.cuda()
    md = None if mask is None else mask.cuda()
    stats = torch.full((n, NS), float("nan"), device="cuda")
    smax = torch.zeros(NS, device="cuda")
    hh = torch.full((n,), float("nan"), device="cuda") if kind == "gbt2" else None
    lib = _native.hip()
    if kind == "gbt":
        rc = lib.hm_gbt_stats(p(Fd), p(yd), p(md), C.c_int64(n), p(stats), p(smax), _st())
    elif kind == "xgb":
        rc = lib.hm_xgb_stats(p(Fd), p(yd), p(md), C.c_int64(n), p(stats), p(smax), _st())
    else:
        rc = lib.hm_gbt2_stats(p(Fd), p(yd), p(md), C.c_int64(n), p(stats), p(smax), p(hh), _st())
    _native.check(rc, "hm_%s_stats" % kind)
    _sync()
    return stats.cpu().numpy(), smax.cpu().numpy(), None if hh is None else hh.cpu().numpy()


def _stats_ref(kind, F, y, mask):
    """fp64 statistics from the kernel comment, and the error model's per-row scale."""
    F64, y64 = F.double().numpy(), y.double().numpy()
    w = np.ones_like(F64) if mask is None else mask.numpy().astype(np.float64)
    with np.errstate(over="ignore"):
        pr = 1.0 / (1.0 + np.exp(-F64))
    model = 2.0 ** -24 * (1.0 + np.abs(F64) * pr * (1.0 - pr))
    if kind == "xgb":
        cols = [(pr - y64) * w, np.maximum(pr * (1.0 - pr), 1e-16) * w]
        hh = None
    else:
        R = y64 - pr
        h = np.abs(R) * (1.0 - np.abs(R)) * w
        cols = [R * w, h, w] if kind == "gbt" else [R * w, w]
        hh = None if kind == "gbt" else h
    return np.stack(cols, 1), hh, model


def _stats_error_ratio(kind, F, y, mask):
    """Largest observed |kernel - fp64| over the c = 1 error model, over every statistic."""
    st, _, hh = _run_stats(kind, F, y, mask)
    ref, rhh, model = _stats_ref(kind, F, y, mask)
    r = float((np.abs(st.astype(np.float64) - ref) / model[:, None]).max())
    if hh is not None:
        r = max(r, float((np.abs(hh.astype(np.float64) - rhh) / model).max()))
    return r


@gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", STATS_N)
@pytest.mark.parametrize("kind", ["gbt", "gbt2", "xgb"])
def test_fused_stats_exact_properties(kind, n, masked):
    """What must hold bit for bit: masked rows (and their hh) are 0, the count column is the
    mask, smax is the |max| of the kernel's own output, xgb h >= 1e-16 on unmasked rows,
    sigmoid(+-100) is exactly 1 / 0, and nothing is NaN."""
    F, y, mask = _stats_inputs(n, seed=n)
    if not masked:
        mask = None
    st, smax, hh = _run_stats(kind, F, y, mask)
    w = np.ones(n, dtype=np.float32) if mask is None else mask.numpy().astype(np.float32)
    assert not np.isnan(st).any() and not np.isnan(smax).any()
    assert (st[w == 0] == 0).all()
    if hh is not None:
        assert not np.isnan(hh).any() and (hh[w == 0] == 0).all()
    if kind == "gbt":
        np.testing.assert_array_equal(st[:, 2], w)
    elif kind == "gbt2":
        np.testing.assert_array_equal(st[:, 1], w)
    else:
        assert (st[w != 0, 1] >= np.float32(1e-16)).all()
    np.testing.assert_array_equal(_bits(smax), _bits(np.abs(st).max(0)))
    # sigmoid saturates exactly: p(100) = 1, p(-100) = 0
    Fn, yn = F.numpy(), y.numpy()
    for v, pv in ((100.0, 1.0), (-100.0, 0.0)):
        sel = (Fn == v) & (w != 0)
        want = (pv - yn[sel]) if kind == "xgb" else (yn[sel] - pv)
        np.testing.assert_array_equal(st[sel, 0], want.astype(np.float32))


@gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", STATS_N)
@pytest.mark.parametrize("kind", ["gbt", "gbt2", "xgb"])
def test_fused_stats_match_fp64(kind, n, masked):
    """p = 1 / (1 + exp(-F)) in fp64 and the formulas of the kernel comment.

    Error model: |dp| <= c * 2^-24 * (1 + |F| p (1 - p)) -- one rounding each for the scaled
    argument of exp2 (its error is multiplied by |F| and by dp/dF = p (1 - p)), exp2, the add and
    the reciprocal; r = y - p and h = |r| (1 - |r|) (|dh/dr| <= 1) inherit it.  Measured on an
    MI355X over all 24 cases of this test: the largest ratio of the observed error to the model
    with c = 1 is 1.46 (every kind, n = 262,444), so c = 4, the next power of two at least twice
    that.
    """
    F, y, mask = _stats_inputs(n, seed=n)
    ratio = _stats_error_ratio(kind, F, y, mask if masked else None)
    print(f"stats {kind} n={n} masked={masked}: error / model(c=1) = {ratio:.4f}")
    assert ratio <= STATS_C, ratio


# =============================================================== 2. hm_absmax_cols
@gpu
@pytest.mark.parametrize("n", [1, 255, 256 * 1024 + 77])
@pytest.mark.parametrize("NS", list(range(1, 9)))
def test_absmax_cols_exact(NS, n):
    """out[s] = max_r |stats[r, s]| exactly; planted per column (rotated over the columns so every
    NS sees every case): the maximum in row 0, in the last row (the grid-stride tail), as a
    negative number, and a column of all -0.0 whose |max| is +0.0."""
    g = torch.Generator().manual_seed(NS * 131 + n)
    for shift in range(4):
        stats = torch.randn(n, NS, generator=g)
        for s in range(NS):
            kind = (s + shift) % 4
            if kind == 0:
                stats[0, s] = 77.0
            elif kind == 1:
                stats[n - 1, s] = 88.0
            elif kind == 2:
                stats[n // 2, s] = -99.0
            else:
                stats[:, s] = -0.0
        sd = stats.cuda()
        out = torch.zeros(NS, device="cuda")
        _native.check(_native.hip().hm_absmax_cols(p(sd), C.c_int64(n), NS, p(out), _st()), "hm_absmax_cols")
        _sync()
        want = stats.abs().amax(0).numpy()
        np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(want))
        assert not np.signbit(out.cpu().numpy()).any()


# =============================================================== 3. leaf sums and Newton values
def _leaf_ids(n, Tn, node16, g, one_leaf=None):
    """Leaf ids in [0, Tn) with -1 (no leaf) and ids >= Tn (not this tree's: skipped) mixed in."""
    if one_leaf is not None:
        leaf = torch.full((n,), one_leaf, dtype=torch.int64)
    else:
        leaf = torch.randint(0, Tn, (n,), generator=g)
        u = torch.rand(n, generator=g)
        leaf[u < 0.1] = -1
        hi = 32767 if node16 else 2 ** 31 - 1
        big = torch.randint(Tn, min(hi, Tn + 5000) + 1, (n,), generator=g)
        sel = (u >= 0.1) & (u < 0.15)
        leaf[sel] = big[sel]
    return leaf.to(torch.int16 if node16 else torch.int32)


def _run_leaf_sums(leaf, gcol, h, Tn):
    n = leaf.numel()
    st2 = torch.full((n, 2), float("nan"))          # only column 0 is read
    st2[:, 0] = gcol
    sums = torch.zeros((Tn, 2), device="cuda")
    ld, sd, hd = leaf.cuda(), st2.cuda(), h.cuda()
    _native.check(_native.hip().hm_leaf_sums(p(ld), p(sd), p(hd), C.c_int64(n), Tn, p(sums),
                                             int(leaf.dtype == torch.int16), _st()), "hm_leaf_sums")
    _sync()
    return sums.cpu().numpy()


def _leaf_sums_ref(leaf, gcol, h, Tn):
    l = leaf.long().numpy()
    ok = (l >= 0) & (l < Tn)
    ref = np.zeros((Tn, 2))
    np.add.at(ref[:, 0], l[ok], gcol.double().numpy()[ok])
    np.add.at(ref[:, 1], l[ok], h.double().numpy()[ok])
    aabs = np.zeros((Tn, 2))
    np.add.at(aabs[:, 0], l[ok], np.abs(gcol.double().numpy()[ok]))
    np.add.at(aabs[:, 1], l[ok], np.abs(h.double().numpy()[ok]))
    cnt = np.bincount(l[ok], minlength=Tn).astype(np.float64)
    return ref, aabs, cnt


def _exact_gh(n, leaf, g, negative=False):
    """g in [-1, 1], h in [0, 1/4], multiples of 2^-6; odd leaves (every leaf with ``negative``)
    get only negative residuals (the two's-complement path of the 64-bit fixed-point sums);
    saturated rows (g != 0, h = 0) and rows with g = 0 are mixed in."""
    gcol = torch.randint(-64, 65, (n,), generator=g).float() / 64
    h = torch.randint(0, 17, (n,), generator=g).float() / 64
    odd = ((leaf.long() % 2) == 1) | negative
    gcol[odd] = -gcol[odd].abs()
    u = torch.rand(n, generator=g)
    h[u < 0.2] = 0.0
    gcol[(u >= 0.2) & (u < 0.35)] = 0.0
    return gcol, h


LEAF_T = [1, 1024, 1025, 8192]     # 4 LDS copies up to 1024 nodes, 1 above; 8192 = the LDS maximum
LEAF_N = [1, 4095, 4097, 70001]    # one block's chunk is 4096 rows


@gpu
@pytest.mark.parametrize("node16", [0, 1])
@pytest.mark.parametrize("n", LEAF_N)
@pytest.mark.parametrize("Tn", LEAF_T)
def test_leaf_sums_exact(Tn, n, node16):
    """Inputs that are multiples of 2^-6: the 2^24 fixed-point conversion is exact, a block's
    64-bit sums are exact, and every partial sum is a multiple of 2^-6 below 2^17 (23 bits), so
    the fp32 conversions and float atomics are exact in any order: the sums equal the fp64 ones."""
    g = torch.Generator().manual_seed(Tn * 7 + n + node16)
    leaf = _leaf_ids(n, Tn, bool(node16), g)
    gcol, h = _exact_gh(n, leaf, g, negative=Tn == 1 and bool(node16))   # one leaf: its sign by dtype
    if Tn == 1 and not node16:
        gcol = gcol.abs()
    ref, aabs, _ = _leaf_sums_ref(leaf, gcol, h, Tn)
    assert aabs.max() < 2 ** 17
    if n > 1000 and Tn > 1:
        assert (ref[:, 0] < 0).any() and (ref[:, 0] > 0).any()
    elif n > 1000:
        assert (ref[0, 0] < 0) == bool(node16)
    np.testing.assert_array_equal(_run_leaf_sums(leaf, gcol, h, Tn).astype(np.float64), ref)


@gpu
@pytest.mark.parametrize("node16", [0, 1])
@pytest.mark.parametrize("Tn,one", [(1, 0), (1024, 1023), (1025, 7), (8192, 8191)])
def test_leaf_sums_exact_every_row_in_one_leaf(Tn, one, node16):
    """All 70,001 rows in one leaf (every LDS add of a wave on the same two words)."""
    n = 70001
    g = torch.Generator().manual_seed(Tn + node16)
    leaf = _leaf_ids(n, Tn, bool(node16), g, one_leaf=one)
    gcol, h = _exact_gh(n, leaf, g)
    ref, aabs, _ = _leaf_sums_ref(leaf, gcol, h, Tn)
    assert aabs.max() < 2 ** 17
    np.testing.assert_array_equal(_run_leaf_sums(leaf, gcol, h, Tn).astype(np.float64), ref)


@gpu
@pytest.mark.parametrize("node16", [0, 1])
@pytest.mark.parametrize("n", LEAF_N)
@pytest.mark.parametrize("Tn", LEAF_T)
def test_leaf_sums_general_bound(Tn, n, node16):
    """Random fp32 g in [-1, 1] and h in [0, 1/4].  Every row is rounded to a multiple of 2^-24
    (error <= 2^-25 per row, cnt rows per leaf); a block's sum of those is exact (64-bit
    integers); each of the G blocks then contributes one float: its conversion rounds by at most
    2^-24 of the block's partial (together <= 2^-24 sum|x|), and each of the G float atomic adds
    rounds by at most 2^-24 of the running sum (<= sum|x|).  Bound per leaf and column:
    cnt * 2^-25 + (G + 1) * 2^-24 * sum|x|, with G = min(1024, ceil(n / 4096)) blocks."""
    g = torch.Generator().manual_seed(Tn * 3 + n + node16)
    leaf = _leaf_ids(n, Tn, bool(node16), g)
    gcol = torch.rand(n, generator=g) * 2 - 1
    h = torch.rand(n, generator=g) * 0.25
    ref, aabs, cnt = _leaf_sums_ref(leaf, gcol, h, Tn)
    G = min(1024, (n + 4095) // 4096)
    bound = cnt[:, None] * 2.0 ** -25 + (G + 1) * 2.0 ** -24 * aabs
    err = np.abs(_run_leaf_sums(leaf, gcol, h, Tn).astype(np.float64) - ref)
    assert (err <= bound).all(), float((err - bound).max())


@gpu
@pytest.mark.parametrize("Tn", [1, 255, 256, 257])
def test_leaf_newton(Tn):
    """vals[k] = sums[k, 0] / sums[k, 1] (0 when |sums[k, 1]| <= 1e-12) for the leaves (sf < 0)
    only: split nodes keep what was there.  One fp32 division: within 1 ulp of the fp64 ratio."""
    g = torch.Generator().manual_seed(Tn)
    sums = torch.randn(Tn, 2, generator=g)
    sums[:, 1] = sums[:, 1].abs() * 10
    tiny = [0.0, 1e-13, -1e-13, 1e-12, -1e-12, 2e-12, -3.0]
    for i, v in enumerate(tiny):
        sums[(i * 37) % Tn, 1] = v
    sf = torch.where(torch.rand(Tn, generator=g) < 0.4, torch.randint(0, 9, (Tn,), generator=g),
                     torch.full((Tn,), -1)).to(torch.int32)
    sf[:: max(1, Tn // 7)] = -1
    if Tn > 1:
        sf[Tn - 1] = -1
        sf[1] = 0
    vals = torch.full((Tn,), 12345.0, device="cuda")
    sd, fd = sums.cuda(), sf.cuda()
    _native.check(_native.hip().hm_leaf_newton(p(sd), p(fd), Tn, p(vals), _st()), "hm_leaf_newton")
    _sync()
    got = vals.cpu().numpy()
    s = sums.numpy()
    leafm = sf.numpy() < 0
    np.testing.assert_array_equal(got[~leafm], np.float32(12345.0))
    zero = np.abs(s[:, 1]) <= np.float32(1e-12)
    np.testing.assert_array_equal(got[leafm & zero], 0.0)
    sel = leafm & ~zero
    ref = s[sel, 0].astype(np.float64) / s[sel, 1].astype(np.float64)
    assert (np.abs(got[sel].astype(np.float64) - ref) <= _ulp32(ref)).all()


# =============================================================== 4. hm_gbt_apply
@gpu
@pytest.mark.parametrize("node16", [0, 1])
@pytest.mark.parametrize("n", [1, 256 * 2048 + 5])
@pytest.mark.parametrize("ldv", [1, 2])
@pytest.mark.parametrize("ldf,k", [(1, 0), (3, 0), (3, 2)])
def test_gbt_apply_exact(ldf, k, ldv, n, node16):
    """F[r, k] += scale * vals[leaf[r], 0] for leaf[r] >= 0; everything else untouched bit for
    bit.  scale = 1/4, leaf values multiples of 2^-8 and F multiples of 2^-12 below 8: the product
    and the sum are exact, so a fused multiply-add cannot differ from mul + add."""
    g = torch.Generator().manual_seed(ldf * 100 + k * 10 + ldv + n + node16)
    Tn = 300
    F = torch.randint(-2 ** 15, 2 ** 15, (n, ldf), generator=g).float() / 2 ** 12
    vals = torch.full((Tn, ldv), float("nan"))
    vals[:, 0] = torch.randint(-2 ** 10, 2 ** 10, (Tn,), generator=g).float() / 2 ** 8
    leaf = torch.randint(-1, Tn, (n,), generator=g)
    leaf[torch.rand(n, generator=g) < 0.2] = -1
    if n > 1:
        leaf[0], leaf[n - 1] = Tn - 1, 0
    leaf = leaf.to(torch.int16 if node16 else torch.int32)
    Fd, vd, ld = F.cuda(), vals.cuda(), leaf.cuda()
    _native.check(_native.hip().hm_gbt_apply(p(Fd), ldf, k, p(vd), ldv, p(ld), C.c_int64(n), C.c_float(0.25),
                                             node16, _st()), "hm_gbt_apply")
    _sync()
    want = F.double().clone()
    l = leaf.long()
    on = l >= 0
    want[on, k] += 0.25 * vals[l[on], 0].double()
    np.testing.assert_array_equal(_bits(Fd.cpu().numpy()), _bits(want.float().numpy()))
    assert bool((want.float().double() == want).all())        # the reference itself is exact in fp32


# =============================================================== 5. hm_quantize
def _run_quantize(dev, X, edges, dpad):
    n, d = X.shape
    Xd, ed = X.contiguous().to(dev), edges.contiguous().to(dev)
    bins = torch.full((n, dpad), 0xAA, dtype=torch.uint8, device=dev)
    args = (p(Xd), C.c_int64(n), d, dpad, p(ed), edges.shape[1], p(bins))
    if dev == "cuda":
        _native.check(_native.hip().hm_quantize(*args, _st()), "hm_quantize")
        _sync()
    else:
        assert _native.host().hm_quantize_cpu(*args) == 0
    return bins.cpu().numpy()


def _quantize_ref(X, edges):
    """bins[r, f] = number of edges[f] strictly below x (searchsorted, side = left), NaN -> n_edges."""
    Xn, En = X.numpy(), edges.numpy()
    out = np.empty(Xn.shape, dtype=np.int64)
    for f in range(Xn.shape[1]):
        out[:, f] = np.searchsorted(En[f], Xn[:, f], side="left")
    out[np.isnan(Xn)] = En.shape[1]
    return out.astype(np.uint8)


def _quantize_case(n, d, n_edges, seed):
    g = torch.Generator().manual_seed(seed)
    # edges rounded to 1/4: duplicates within a feature
    edges = torch.sort(torch.round(torch.randn(d, n_edges, generator=g) * 8) / 4, 1).values
    X = torch.randn(n, d, generator=g) * 2
    u = torch.rand(n, d, generator=g)
    pick = edges[torch.arange(d)[None, :].expand(n, d), torch.randint(0, n_edges, (n, d), generator=g)]
    X = torch.where(u < 0.3, pick, X)                        # values equal to an edge
    X[(u >= 0.3) & (u < 0.33)] = float("inf")
    X[(u >= 0.33) & (u < 0.36)] = float("-inf")
    X[(u >= 0.36) & (u < 0.40)] = float("nan")
    return X, edges


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("d,dpad", [(1, 16), (9, 16), (28, 32)])
@pytest.mark.parametrize("n_edges", [1, 63, 255])
def test_quantize_matches_searchsorted(n_edges, d, dpad, dev):
    X, edges = _quantize_case(1031, d, n_edges, seed=n_edges + d)
    assert (edges[:, 1:] == edges[:, :-1]).any() or n_edges == 1
    got = _run_quantize(dev, X, edges, dpad)
    np.testing.assert_array_equal(got[:, :d], _quantize_ref(X, edges))
    assert (got[:, d:] == 0xAA).all()                        # row padding is not written


@gpu
def test_quantize_grid_stride_loop():
    """600,000 x 28 values: just above the 65,536 blocks x 256 threads of the capped grid, so the
    last elements are reached by the grid-stride loop (the HIGGS-shaped workload runs through it)."""
    n, d = 600000, 28
    assert n * d > 65536 * 256
    X, edges = _quantize_case(n, d, 63, seed=5)
    got = _run_quantize("cuda", X, edges, 32)
    np.testing.assert_array_equal(got[:, :d], _quantize_ref(X, edges))
    assert (got[:, d:] == 0xAA).all()


# =============================================================== 6. hm_tree_predict
_XV = [0.0, 1.0, 2.0, 3.0, 0.5, -1.5, float("nan")]       # feature values; thresholds come from the same set


def _hand_forest(n_trees, n_out, seed):
    """Trees of uneven depth packed into one node array (roots in reverse order of the trees'
    positions); every kind of split: ordinal, nominal (CAT_FLAG), default-left, both."""
    rng = np.random.default_rng(seed)
    feat, thr, lft, rgt, voff, vals, roots = [], [], [], [], [], [], []

    def leaf():
        k = len(feat)
        feat.append(-1); thr.append(3.4e38); lft.append(0); rgt.append(0)
        voff.append(len(vals))
        vals.extend((rng.integers(-512, 513, n_out) / 256.0).tolist())
        return k

    def grow(depth):
        if depth == 0 or rng.random() < 0.2:
            return leaf()
        k = len(feat)
        f = int(rng.integers(0, 5)) | (CAT_FLAG if rng.random() < 0.35 else 0) | (DLEFT_FLAG if rng.random() < 0.5 else 0)
        feat.append(f); thr.append(float(_XV[int(rng.integers(0, 6))])); lft.append(-1); rgt.append(-1)
        voff.append(0)
        lft[k] = grow(depth - 1)
        rgt[k] = grow(depth - 1)
        return k

    for t in range(n_trees):
        if t == 1:
            roots.append(leaf())                              # a root that is a leaf
        else:
            while True:
                start = len(feat)
                r = grow(2 + t % 4)
                if feat[r] >= 0:
                    break
                del feat[start:], thr[start:], lft[start:], rgt[start:], voff[start:]
            roots.append(r)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)
    return dict(feature=i32(feat), threshold=torch.tensor(thr, dtype=torch.float32), left=i32(lft), right=i32(rgt),
                voff=i32(voff), values=torch.tensor(vals, dtype=torch.float32), roots=i32(roots[::-1]))


def _walk(fl, x, t):
    """Pure-Python traversal: left when x <= threshold (nominal: x == threshold); NaN right unless
    the split has DLEFT_FLAG."""
    k = int(fl["roots"][t])
    while int(fl["feature"][k]) >= 0:
        f = int(fl["feature"][k])
        v = x[f & ~(CAT_FLAG | DLEFT_FLAG)]
        th = float(fl["threshold"][k])
        if math.isnan(v):
            left = bool(f & DLEFT_FLAG)
        else:
            left = (v == th) if f & CAT_FLAG else (v <= th)
        k = int(fl["left"][k]) if left else int(fl["right"][k])
    return k


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("mode", ["per_tree", "sum_weighted", "sum_plain"])
@pytest.mark.parametrize("n_out", [1, 3])
@pytest.mark.parametrize("n_trees", [1, 3, 7])
def test_tree_predict_matches_python_walk(n_trees, n_out, mode, dev):
    fl = _hand_forest(n_trees, n_out, seed=n_trees * 10 + n_out)
    rng = np.random.default_rng(1)
    n, d = 700, 5
    X = torch.tensor(np.asarray(_XV, dtype=np.float32)[rng.integers(0, len(_XV), (n, d))])
    flags = fl["feature"][fl["feature"] >= 0]
    if n_trees > 1:
        assert ((flags & CAT_FLAG) != 0).any() and ((flags & DLEFT_FLAG) != 0).any()
        assert ((flags & DLEFT_FLAG) == 0).any() and ((flags & CAT_FLAG) == 0).any()
    tw = torch.tensor(rng.integers(-8, 9, n_trees) / 4.0, dtype=torch.float32)
    fn = {k: v.numpy() for k, v in fl.items()}
    Xn = X.numpy().tolist()
    leafs = np.array([[_walk(fn, Xn[r], t) for t in range(n_trees)] for r in range(n)])
    V = fn["values"].astype(np.float64)
    per = np.stack([V[fn["voff"][leafs] + o] for o in range(n_out)], -1)          # [n, T, n_out]
    summed = mode != "per_tree"
    if mode == "per_tree":
        want = per
    elif mode == "sum_weighted":
        want = (per * tw.double().numpy()[None, :, None]).sum(1)
    else:
        want = per.sum(1)
    fd = {k: v.to(dev) for k, v in fl.items()}
    Xd = X.to(dev)
    twd = tw.to(dev) if mode == "sum_weighted" else None
    out = torch.zeros((n, n_out) if summed else (n, n_trees, n_out), dtype=torch.float32, device=dev)
    if not summed:
        out.fill_(float("nan"))
    args = (p(Xd), C.c_int64(n), d, p(fd["feature"]), p(fd["threshold"]), p(fd["left"]), p(fd["right"]),
            p(fd["voff"]), p(fd["values"]), p(fd["roots"]), n_trees, n_out, p(out), int(summed), p(twd))
    if dev == "cuda":
        _native.check(_native.hip().hm_tree_predict(*args, _st()), "hm_tree_predict")
        _sync()
    else:
        assert _native.host().hm_tree_predict_cpu(*args) == 0
    # leaf values are multiples of 2^-8, weights of 1/4: every product and partial sum is exact
    np.testing.assert_array_equal(out.cpu().numpy().astype(np.float64), want)


# =============================================================== 7. routing
def _route_ref(bins, node, sf, sb, lc, rc, miss_bin, lo, hi):
    """Rows at a node in [lo, hi) that split move to a child: left when the row's bin of the split
    feature is <= the split bin (nominal: ==), the missing bin follows the default-left flag;
    everything else (leaves of the level, ids below lo, -1) stays."""
    out = node.copy()
    sel = np.nonzero((node >= lo) & (node < hi))[0]
    nd = node[sel]
    f = sf[nd]
    sp = f >= 0
    sel, nd, f = sel[sp], nd[sp], f[sp]
    b = bins[sel, f & ~(CAT_FLAG | DLEFT_FLAG)].astype(np.int64)
    left = np.where(b == miss_bin, (f & DLEFT_FLAG) != 0, np.where((f & CAT_FLAG) != 0, b == sb[nd], b <= sb[nd]))
    out[sel] = np.where(left, lc[nd], rc[nd])
    return out


def _route_case(n, lo, L, n_split, seed, d=9, B=16):
    """A level of L nodes [lo, lo + L) of which n_split split (compact child numbering from
    hi = lo + L), with ordinal, nominal, default-left and both-flag splits; rows spread over the
    level, earlier leaves (ids < lo) and -1."""
    rng = np.random.default_rng(seed)
    hi = lo + L
    sf = np.full(hi, -1, dtype=np.int32)
    sb = rng.integers(0, B, hi).astype(np.int32)
    lc = rng.integers(0, 30000, hi).astype(np.int32)      # garbage wherever no split reads it
    rc = rng.integers(0, 30000, hi).astype(np.int32)
    split_nodes = np.sort(rng.choice(L, n_split, replace=False)) + lo
    flags = np.array([0, CAT_FLAG, DLEFT_FLAG, CAT_FLAG | DLEFT_FLAG], dtype=np.int64)
    sf[split_nodes] = (rng.integers(0, d, n_split) | flags[np.arange(n_split) % 4]).astype(np.int32)
    lc[split_nodes] = hi + 2 * np.arange(n_split)
    rc[split_nodes] = hi + 2 * np.arange(n_split) + 1
    node = rng.integers(lo, hi, n).astype(np.int32)
    u = rng.random(n)
    node[u < 0.1] = -1
    if lo > 0:
        node[(u >= 0.1) & (u < 0.2)] = rng.integers(0, lo, n)[(u >= 0.1) & (u < 0.2)]
    bins = np.full((n, 16), 0xAA, dtype=np.uint8)
    bins[:, :d] = rng.integers(0, B, (n, d))
    return dict(n=n, d=d, B=B, lo=lo, hi=hi, sf=sf, sb=sb, lc=lc, rc=rc, node=node, bins=bins, n_split=n_split)


def _bins_dev(c, dev, feature_major):
    """(bins tensor, col_stride): row-major [n, 16], or the feature-major copy [d, n + 3]."""
    if not feature_major:
        return torch.from_numpy(c["bins"]).to(dev), 0
    bt = np.full((c["d"], c["n"] + 3), 0xAA, dtype=np.uint8)
    bt[:, : c["n"]] = c["bins"][:, : c["d"]].T
    return torch.from_numpy(bt).to(dev), c["n"] + 3


def _run_route_rows(c, dev, node16, feature_major, miss_bin):
    bd, cs = _bins_dev(c, dev, feature_major)
    node = torch.from_numpy(c["node"]).to(torch.int16 if node16 else torch.int32).to(dev)
    sf, sb, lc, rc = (torch.from_numpy(c[k]).to(dev) for k in ("sf", "sb", "lc", "rc"))
    if dev == "cuda":
        _native.check(_native.hip().hm_route_rows(p(bd), C.c_int64(c["n"]), 16, C.c_int64(cs), c["lo"], c["hi"], p(node),
                                                  p(sf), p(sb), p(lc), p(rc), miss_bin, int(node16), _st()),
                      "hm_route_rows")
        _sync()
    else:
        assert not node16 and not feature_major
        assert _native.host().hm_route_rows_cpu(p(bd), C.c_int64(c["n"]), 16, p(node), p(sf), p(sb), p(lc), p(rc),
                                                miss_bin) == 0
    return node.cpu().numpy().astype(np.int32)


def _route_variants(dev):
    return [(0, 0)] if dev == "cpu" else [(0, 0), (0, 1), (1, 0), (1, 1)]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("miss", [False, True])
@pytest.mark.parametrize("n", [1, 4095, 3 * 4096 + 5])
def test_route_rows_matches_reference(n, miss, dev):
    """The host twin takes int32 ids and row-major bins; the kernel is also run with int16 ids
    and with the feature-major bins copy (col_stride = n + 3)."""
    c = _route_case(n, lo=5, L=40, n_split=29, seed=n + miss)
    miss_bin = c["B"] - 1 if miss else -1
    want = _route_ref(c["bins"], c["node"], c["sf"], c["sb"], c["lc"], c["rc"], miss_bin, c["lo"], c["hi"])
    if n > 1000:
        moved = want != c["node"]
        assert moved.any() and (want[c["node"] < c["lo"]] == c["node"][c["node"] < c["lo"]]).all()
        assert ((c["node"] >= c["lo"]) & ~moved).any()       # leaves inside the level
    for node16, fm in _route_variants(dev):
        np.testing.assert_array_equal(_run_route_rows(c, dev, node16, fm, miss_bin), want, err_msg=f"{node16} {fm}")


@gpu
@pytest.mark.parametrize("fm", [0, 1])
def test_route_rows_wide_level_global_table(fm):
    """A level of 1,500 nodes (int32 ids): nodes past the first 1,024 are not in the LDS split
    table and take the global-memory fallback."""
    c = _route_case(3 * 4096 + 5, lo=3, L=1500, n_split=1100, seed=11)
    assert (c["sf"][c["lo"] + 1024:] >= 0).any() and (c["node"] >= c["lo"] + 1024).any()
    for miss_bin in (-1, c["B"] - 1):
        want = _route_ref(c["bins"], c["node"], c["sf"], c["sb"], c["lc"], c["rc"], miss_bin, c["lo"], c["hi"])
        np.testing.assert_array_equal(_run_route_rows(c, "cuda", 0, fm, miss_bin), want)


def _lut_for(nkeys, rng):
    """Compact level: split j's children are 2j, 2j + 1 (relative to nb); one of them (random) is
    the small child with key j, the other is not histogrammed (32767)."""
    sr = rng.integers(0, 2, nkeys)
    lut = np.full(2 * nkeys, 32767, dtype=np.int16)
    lut[2 * np.arange(nkeys) + sr] = np.arange(nkeys, dtype=np.int16)
    return lut


@gpu
@pytest.mark.parametrize("node16", [0, 1])
@pytest.mark.parametrize("nkeys", [1, 16, 17, 300, 1100])
def test_route_count_and_scatter(nkeys, node16):
    """hm_route_count = hm_route_rows + per-(key, block) counts of the rows that land in a small
    child, block b owning rows [b ceil(n / G), (b + 1) ceil(n / G)); hm_partition_scatter(rows =
    NULL) then groups those rows by key.  nkeys <= 16 counts with wave ballots, above with LDS
    atomics; 1,100 keys make the lut (2,200 entries) overflow its 2,048-entry LDS copy and the
    level (1,103 nodes) its 1,024-entry split table."""
    rng = np.random.default_rng(nkeys + node16)
    lut = _lut_for(nkeys, rng)
    lib = _native.hip()
    for n, G, fm, miss in [(3 * 4096 + 5, 1, 0, False), (3 * 4096 + 5, 3, 1, True), (3 * 4096 + 5, 7, 0, True),
                           (4095, 7, 1, False), (4095, 3, 0, True), (1, 1, 0, False), (1, 3, 1, True)]:
        c = _route_case(n, lo=4, L=nkeys + 3, n_split=nkeys, seed=nkeys * 13 + n + G)
        nb = c["hi"]
        miss_bin = c["B"] - 1 if miss else -1
        want = _route_ref(c["bins"], c["node"], c["sf"], c["sb"], c["lc"], c["rc"], miss_bin, c["lo"], nb)
        rel = want.astype(np.int64) - nb
        inr = (rel >= 0) & (rel < 2 * nkeys)
        key = np.where(inr, lut[np.clip(rel, 0, 2 * nkeys - 1)], 32767).astype(np.int64)
        key[key >= nkeys] = -1
        chunk = (n + G - 1) // G
        blk = np.arange(n) // chunk
        want_counts = np.zeros((nkeys, G), dtype=np.int64)
        np.add.at(want_counts, (key[key >= 0], blk[key >= 0]), 1)

        bd, cs = _bins_dev(c, "cuda", fm)
        node = torch.from_numpy(c["node"]).to(torch.int16 if node16 else torch.int32).cuda()
        sf, sb, lc, rc = (torch.from_numpy(c[k]).cuda() for k in ("sf", "sb", "lc", "rc"))
        lutd = torch.from_numpy(lut).cuda()
        counts = torch.full((nkeys * G,), -7, dtype=torch.int64, device="cuda")
        _native.check(lib.hm_route_count(p(bd), C.c_int64(n), 16, C.c_int64(cs), c["lo"], p(node), p(sf), p(sb), p(lc),
                                         p(rc), miss_bin, p(lutd), nb, 2 * nkeys, nkeys, G, p(counts), node16, _st()),
                      "hm_route_count")
        incl = torch.cumsum(counts, 0)
        rows = torch.full((max(1, n),), -1, dtype=torch.int32, device="cuda")
        seg = torch.full((nkeys + 1,), -1, dtype=torch.int64, device="cuda")
        _native.check(lib.hm_partition_scatter(None, C.c_int64(n), p(node), p(lutd), nb, 2 * nkeys, nkeys, G, p(counts),
                                               p(incl), p(rows), p(seg), node16, _st()), "hm_partition_scatter")
        _sync()
        tag = f"n={n} G={G} fm={fm} miss={miss}"
        np.testing.assert_array_equal(counts.cpu().numpy().reshape(nkeys, G), want_counts, err_msg=tag)
        routed = node.cpu().numpy().astype(np.int32)
        np.testing.assert_array_equal(routed, want, err_msg=tag)
        np.testing.assert_array_equal(routed, _run_route_rows(c, "cuda", node16, fm, miss_bin), err_msg=tag)
        segn, rown = seg.cpu().numpy(), rows.cpu().numpy()
        np.testing.assert_array_equal(segn, np.concatenate([[0], np.cumsum(want_counts.sum(1))]), err_msg=tag)
        assert segn[nkeys] == (key >= 0).sum()
        for k in range(nkeys):
            got = np.sort(rown[segn[k]:segn[k + 1]])
            np.testing.assert_array_equal(got, np.nonzero(key == k)[0], err_msg=f"{tag} key {k}")


# =============================================================== 8. sibling histograms
SIB_PER = [4, 1020, 1028, 4 * (256 * 64 + 3)]     # one float4, under / over one block, past the 64-block cap


@gpu
@pytest.mark.parametrize("n_split", [1, 5])
@pytest.mark.parametrize("per", SIB_PER)
def test_hist_sibling_bit_exact(per, n_split):
    """Split i (parent li[i]): child 2i + sr[i] is Hs[i] bit for bit, child 2i + 1 - sr[i] the
    fp32 difference H[li[i]] - Hs[i] (one subtraction: no tolerance); every element is written."""
    g = torch.Generator().manual_seed(per + n_split)
    L = n_split + 3
    H = torch.randn(L, per, generator=g)
    Hs = torch.randn(n_split, per, generator=g)
    li = torch.randperm(L, generator=g)[:n_split]                 # out of order
    sr = (torch.arange(n_split) % 2 == 0).to(torch.uint8) if n_split > 1 else torch.ones(1, dtype=torch.uint8)
    Hn = torch.full((2 * n_split, per), float("nan"), device="cuda")
    Hd, Hsd, lid, srd = H.cuda(), Hs.cuda(), li.cuda(), sr.cuda()
    _native.check(_native.hip().hm_hist_sibling(p(Hd), p(Hsd), p(lid), p(srd), C.c_int64(per), n_split, p(Hn), _st()),
                  "hm_hist_sibling")
    _sync()
    want = torch.empty(2 * n_split, per)
    j2 = 2 * torch.arange(n_split)
    want[j2 + sr.long()] = Hs
    want[j2 + 1 - sr.long()] = H[li] - Hs
    np.testing.assert_array_equal(_bits(Hn.cpu().numpy()), _bits(want.numpy()))


@gpu
@pytest.mark.parametrize("L", [1, 5])
@pytest.mark.parametrize("per", SIB_PER)
def test_hist_sibling_heap_bit_exact(per, L):
    """Heap form: parent l's children are 2l, 2l + 1; parents with split_feat < 0 get exact zeros
    in both, whatever (NaN here) their H and Hs rows hold."""
    g = torch.Generator().manual_seed(per * 3 + L)
    H = torch.randn(L, per, generator=g)
    Hs = torch.randn(L, per, generator=g)
    sf = torch.tensor([7, -1, 0, 3 | CAT_FLAG, -1][:L], dtype=torch.int32)
    sr = torch.tensor([1, 1, 0, 1, 0][:L], dtype=torch.uint8)
    H[sf < 0] = float("nan")
    Hs[sf < 0] = float("nan")
    for split_l0 in ([True, False] if L == 1 else [True]):
        if not split_l0:
            sf = torch.tensor([-1], dtype=torch.int32)
            H[:], Hs[:] = float("nan"), float("nan")
        Hn = torch.full((2 * L, per), float("nan"), device="cuda")
        Hd, Hsd, sfd, srd = H.cuda(), Hs.cuda(), sf.cuda(), sr.cuda()
        _native.check(_native.hip().hm_hist_sibling_heap(p(Hd), p(Hsd), p(sfd), p(srd), C.c_int64(per), L, p(Hn), _st()),
                      "hm_hist_sibling_heap")
        _sync()
        want = torch.zeros(2 * L, per)
        for l in range(L):
            if int(sf[l]) >= 0:
                want[2 * l + int(sr[l])] = Hs[l]
                want[2 * l + 1 - int(sr[l])] = H[l] - Hs[l]
        np.testing.assert_array_equal(_bits(Hn.cpu().numpy()), _bits(want.numpy()))


# =============================================================== 9. hm_level_finalize
def _finalize_ref(b, gain, feat, braw, left, tot, edges, cat, nb, heap=False, last=False):
    """A tree level's bookkeeping as the tensor formulation of HistTreeBuilder.build (its
    non-fused branch, with the builder's own _leaf_values / _weight), on CPU tensors.  ``heap``:
    parent l's children are nb + 2l, nb + 2l + 1 and small_right / lut are indexed by l (32767 in
    both lut slots and small_right 0 for parents that do not split).  ``last``: the children are
    leaves, valued from (left, tot - left) of their parent's split (zeros under unsplit heap
    parents); their records follow the level's at 2 * key, 2 * key + 1."""
    L, NS = tot.shape
    E = edges.shape[1]
    inf = float("inf")
    bb, bdl = braw & 0xFFFF, (braw >> 16) & 1
    vals = b._leaf_values(tot)
    ok = (gain > max(1e-12, b.min_gain)) & torch.isfinite(gain) & (b._weight(tot) >= b.min_split)
    li = torch.nonzero(ok).flatten()
    n_split = li.numel()
    rank = torch.cumsum(ok.int(), 0) - 1
    slot = torch.arange(L, dtype=torch.int32) if heap else rank
    lc = torch.where(ok, nb + 2 * slot, torch.full_like(rank, -1)).to(torch.int32)
    rc = torch.where(ok, lc + 1, lc).to(torch.int32)
    thr = torch.where(bb < E, edges[feat.long(), bb.clamp(max=E - 1).long()], torch.full_like(gain, inf))
    bflag = feat if cat is None else feat | (cat[feat.long()].to(torch.int32) * CAT_FLAG)
    bflag = bflag | (bdl * DLEFT_FLAG)
    left_tot = left[li]
    right_tot = tot[li] - left_tot
    sr = (b._weight(right_tot) < b._weight(left_tot)).long()
    keys = li if heap else torch.arange(n_split)
    nk = L if heap else n_split
    small_right = torch.zeros(nk, dtype=torch.uint8)
    small_right[keys] = sr.to(torch.uint8)
    lut = torch.full((2 * nk,), 32767, dtype=torch.int16)
    lut[2 * keys + sr] = keys.to(torch.int16)
    imp = torch.zeros(b.q.d, dtype=torch.float64).index_add_(0, feat[li].long(), gain[li].double())
    out = dict(n_split=n_split, vals=vals, feats=torch.where(ok, bflag, torch.full_like(feat, -1)),
               thrs=torch.where(ok, thr, torch.full_like(thr, inf)), lc=lc, rc=rc, sb=bb, li=li,
               small_right=small_right, lut=lut, imp=imp)
    if last:
        cv = torch.zeros(2 * nk, vals.shape[1])
        cv[2 * keys] = b._leaf_values(left_tot)
        cv[2 * keys + 1] = b._leaf_values(right_tot)
        out["child_vals"] = cv
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def _exact_tree_data(kind, n, seed, d=9, cat_col=None):
    """Rows whose statistics are exact in fp32 sums: gini = integer class weights {0, 1, 2} of three
    classes, variance = (w y, w) with integer targets and weights.  5 % NaN."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, d, generator=g)
    if cat_col is not None:
        X[:, cat_col] = torch.randint(0, 6, (n,), generator=g).float()
    X[torch.rand(n, d, generator=g) < 0.05] = float("nan")
    z = torch.nan_to_num(X)
    w = torch.randint(0, 3, (n,), generator=g).float()
    t = (z[:, 1] * z[:, 3] > 0) if cat_col is None else (z[:, cat_col] == 3)
    if kind == "gini":
        y = (z[:, 0] > 0.3).long() + t.long()
        stats = torch.nn.functional.one_hot(y, 3).float() * w[:, None]
    else:
        y = torch.round(2 * z[:, 0] + 2 * t.float() + z[:, 4]).clamp(-3, 3)
        stats = torch.stack([w * y, w], 1)
    return X, stats


@pytest.mark.parametrize("kind", ["gini", "variance"])
def test_finalize_reference_reproduces_host_build(kind):
    """Anchor of _finalize_ref: fed the split-search output of every level of a host (CPU) build
    -- missing-value default directions and a nominal column included -- it reproduces that
    level's node records, the children's numbering, the last level's leaf values (``last``: from
    the split statistics; the host build takes them from histograms, identical for exact
    statistics) and the importance."""
    X, stats = _exact_tree_data(kind, 6000, seed=3, d=6, cat_col=2)
    cat = torch.tensor([False, False, True, False, False, False])
    q = quantize(X, 16, categorical=cat, missing=True)
    assert q.missing
    b = HistTreeBuilder(q, kind, max_depth=4, min_samples_split=700, min_samples_leaf=5, seed=1)
    calls, orig = [], b._split_find_raw

    def record(H, base):
        out = orig(H, base)
        calls.append((base, [t.clone() for t in out]))
        return out

    b._split_find_raw = record
    tree = b.build(stats)
    assert len(calls) == 4 and any(tree.cat) and any(tree.dleft) and -1 in tree.feature[:15]
    imp = np.zeros(q.d)
    for i, (base, (gain, feat, braw, left, tot)) in enumerate(calls):
        L = gain.numel()
        nb = base + L
        ref = _finalize_ref(b, gain, feat, braw, left, tot, q.edges, q.cat, nb, last=i == len(calls) - 1)
        imp += ref["imp"]
        sl = slice(base, nb)
        split = ref["feats"] >= 0
        np.testing.assert_array_equal(np.asarray(tree.feature[sl]),
                                      np.where(split, ref["feats"] & ~(CAT_FLAG | DLEFT_FLAG), -1))
        np.testing.assert_array_equal(np.asarray(tree.cat[sl]), split & ((ref["feats"] & CAT_FLAG) != 0))
        np.testing.assert_array_equal(np.asarray(tree.dleft[sl]), split & ((ref["feats"] & DLEFT_FLAG) != 0))
        np.testing.assert_array_equal(np.asarray(tree.threshold[sl]), ref["thrs"].astype(np.float64))
        np.testing.assert_array_equal(np.asarray(tree.left[sl]), ref["lc"])
        np.testing.assert_array_equal(np.asarray(tree.right[sl]), ref["rc"])
        np.testing.assert_array_equal(b.node_values[sl].numpy(), ref["vals"])
        assert i == len(calls) - 1 or calls[i + 1][1][0].numel() == 2 * ref["n_split"]
    np.testing.assert_array_equal(b.node_values[nb:].numpy(), ref["child_vals"])
    assert len(tree.feature) == nb + 2 * ref["n_split"]
    np.testing.assert_allclose(b.importance, imp, rtol=1e-12)


FIN_D, FIN_E = 6, 15
FIN_MIN_SPLIT = 4.0
# what a planted node must exercise; the first six must be refused, the last four must split
FIN_PLANTS = ["gain_ninf", "gain_nan", "gain_pinf", "gain_at_min", "weight_below", "weight_zero",
              "cat_feature", "default_left", "bin_past_edges", "equal_children"]


def _finalize_case(crit, NS, L, seed, min_gain, only=None):
    """Split-search results of a level of L nodes with integer-valued (quarter-valued for
    hessians) statistics, so weights and their comparisons are exact in any summation order."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g)
    gain = torch.rand(L, generator=g) * 10 + 0.75
    feat = ri(0, FIN_D, L).to(torch.int32)
    braw = (ri(0, FIN_E, L) | (ri(0, 2, L) << 16)).to(torch.int32)
    frac = torch.rand(L, generator=g)
    if crit in ("gini", "entropy"):
        tot = ri(0, 21, L, NS).float()
        tot[:, 0] += 4
        left = torch.floor(tot * frac[:, None])
    else:
        w = ri(4, 41, L).float()
        wl = torch.floor(w * frac)
        s0 = ri(-40, 41, L).float() / 2
        l0 = ri(-40, 41, L).float() / 2
        if crit == "gbt":
            h = ri(0, 33, L).float() / 4
            h[ri(0, 5, L) == 0] = 0.0                     # |sum h| <= 1e-12: leaf value 0
            tot = torch.stack([s0, h, w], 1)
            left = torch.stack([l0, torch.floor(h * frac * 4) / 4, wl], 1)
        else:
            tot = torch.stack([s0, w], 1)
            left = torch.stack([l0, wl], 1)
    wcol = None if crit in ("gini", "entropy") else (2 if crit == "gbt" else 1)
    gmin = float(np.float32(max(1e-12, min_gain)))

    def plant(l, kind):
        if kind == "gain_ninf":
            gain[l] = -float("inf")
        elif kind == "gain_nan":
            gain[l] = float("nan")
        elif kind == "gain_pinf":
            gain[l] = float("inf")
        elif kind == "gain_at_min":
            gain[l] = gmin                                  # the test is strict: refused
        elif kind == "weight_below":
            if wcol is None:
                tot[l] = 0.0
                tot[l, 0], tot[l, NS - 1] = 1.75, 2.0
            else:
                tot[l, wcol] = float(np.nextafter(np.float32(FIN_MIN_SPLIT), np.float32(0)))
            left[l] = torch.floor(tot[l] / 2)
        elif kind == "weight_zero":
            tot[l] = 0.0
            left[l] = 0.0
        elif kind == "cat_feature":
            feat[l] = 2
            gain[l] = 3.5
        elif kind == "default_left":
            braw[l] = 3 | (1 << 16)
            gain[l] = 2.5
        elif kind == "bin_past_edges":
            feat[l] = 1
            braw[l] = FIN_E
            gain[l] = 1.5
        elif kind == "equal_children":
            left[l] = torch.floor(tot[l] / 2) + 1
            tot[l] = 2 * left[l]
            gain[l] = 4.5

    if only is not None:
        plant(only[0], only[1])
    elif L >= len(FIN_PLANTS):
        # repeated down the level, so the plants fall into many threads' node chunks
        for j in range(0, L - len(FIN_PLANTS) + 1, 97):
            for i, kind in enumerate(FIN_PLANTS):
                plant(j + i, kind)
    return gain, feat, braw, left, tot


FIN_SENT = 123456


def _run_finalize(b, case, edges, cat, nb, heap, last, n_out):
    gain, feat, braw, left, tot = (t.cuda() for t in case)
    L, NS = tot.shape
    cap = 3 * L
    i32 = lambda n: torch.full((n,), FIN_SENT, dtype=torch.int32, device="cuda")
    vals = torch.full((cap, n_out), float(FIN_SENT), device="cuda")
    feats, lc, rc, sb = i32(cap), i32(cap), i32(cap), i32(cap)
    thrs = torch.full((cap,), float(FIN_SENT), device="cuda")
    li = torch.full((L,), -5, dtype=torch.int64, device="cuda")
    sr = torch.full((L,), 9, dtype=torch.uint8, device="cuda")
    lut = torch.full((2 * L,), -3, dtype=torch.int16, device="cuda")
    nsp = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    imp = torch.zeros(FIN_D, dtype=torch.float64, device="cuda")
    ed = edges.cuda()
    catd = None if cat is None else cat.to(torch.uint8).cuda()
    ip = np.array([L, NS, FIN_D, edges.shape[1], b._CRIT[b.criterion], n_out, nb, int(cat is not None), int(heap),
                   int(last)], dtype=np.int32)
    fp = np.array([b.lam, b.alpha, b.min_gain, float(b.min_split)], dtype=np.float32)
    _native.check(_native.hip().hm_level_finalize(
        ip.ctypes.data, fp.ctypes.data, p(gain), p(feat), p(braw), p(left), p(tot), p(ed), p(catd), p(vals),
        p(feats), p(thrs), p(lc), p(rc), p(sb), p(li), p(sr), p(lut), p(nsp), p(imp), _st()), "hm_level_finalize")
    _sync()
    return {k: v.cpu().numpy() for k, v in dict(vals=vals, feats=feats, thrs=thrs, lc=lc, rc=rc, sb=sb, li=li,
                                                small_right=sr, lut=lut, n_split=nsp, imp=imp).items()}


def _close_ulp(got, ref, ulps, msg):
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    assert (err <= ulps * _ulp32(ref)).all(), msg


def _check_finalize(b, case, edges, cat, nb, heap, last, n_out, tag):
    L = case[0].numel()
    ref = _finalize_ref(b, *case, edges, cat, nb, heap=heap, last=last)
    got = _run_finalize(b, case, edges, cat, nb, heap, last, n_out)
    ns = ref["n_split"]
    assert int(got["n_split"][0]) == ns, tag
    for k in ("feats", "lc", "rc", "sb"):
        np.testing.assert_array_equal(got[k][:L], ref[k], err_msg=f"{tag} {k}")
    np.testing.assert_array_equal(_bits(got["thrs"][:L]), _bits(ref["thrs"]), err_msg=f"{tag} thr")
    _close_ulp(got["vals"][:L], ref["vals"], 2, f"{tag} vals")
    np.testing.assert_array_equal(got["li"][:ns], ref["li"], err_msg=f"{tag} li")
    nk = L if heap else ns
    np.testing.assert_array_equal(got["small_right"][:nk], ref["small_right"], err_msg=f"{tag} small_right")
    np.testing.assert_array_equal(got["lut"][:2 * nk], ref["lut"], err_msg=f"{tag} lut")
    np.testing.assert_allclose(got["imp"], ref["imp"], rtol=1e-12, atol=0, err_msg=f"{tag} imp")
    end = L
    if last:                                   # the children's leaf records follow the level's
        end = L + 2 * nk
        c = slice(L, end)
        np.testing.assert_array_equal(got["feats"][c], -1, err_msg=f"{tag} child feats")
        np.testing.assert_array_equal(got["lc"][c], -1, err_msg=f"{tag} child lc")
        np.testing.assert_array_equal(got["rc"][c], -1, err_msg=f"{tag} child rc")
        np.testing.assert_array_equal(got["sb"][c], 0, err_msg=f"{tag} child sb")
        assert np.isposinf(got["thrs"][c]).all(), tag
        _close_ulp(got["vals"][c], ref["child_vals"], 2, f"{tag} child vals")
    # nothing is written past the records the mode owns
    for k in ("feats", "lc", "rc", "sb"):
        np.testing.assert_array_equal(got[k][end:], FIN_SENT, err_msg=f"{tag} {k} tail")
    np.testing.assert_array_equal(got["vals"][end:], float(FIN_SENT), err_msg=f"{tag} vals tail")
    return ref


FIN_CRITS = [("gini", 3), ("entropy", 2), ("variance", 2), ("gbt", 3), ("xgb", 2), ("gbt2", 2), ("gini", 11),
             ("entropy", 11)]


def _finalize_builder(crit, cat):
    edges = torch.sort(torch.randn(FIN_D, FIN_E, generator=torch.Generator().manual_seed(1)), 1).values
    q = Quantized(torch.zeros(1, 16, dtype=torch.uint8), edges, FIN_D, FIN_E + 1, cat)
    b = HistTreeBuilder(q, crit, lam=0.5 if crit in ("gbt", "xgb", "gbt2") else 0.0,
                        alpha=0.25 if crit == "xgb" else 0.0, min_gain=0.5 if crit in ("gini", "xgb", "gbt") else 0.0)
    b.min_split = FIN_MIN_SPLIT
    return b, edges


@gpu
@pytest.mark.parametrize("heap,last", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("crit,NS", FIN_CRITS)
def test_level_finalize_matches_tensor_formulation(crit, NS, heap, last):
    """hm_level_finalize against _finalize_ref at L = 1 .. 3000 (above 1,024 nodes a thread owns
    two or three and the children's ranks must still follow node order).  Integer outputs and
    thresholds exact, leaf values within 2 ulp (same operations), importance (an fp64 sum of
    fp32 gains in any order) to 1e-12; entries the contract leaves unspecified (li, and in the
    compact layout small_right / lut, past the split count) are not compared."""
    cat = torch.tensor([False, False, True, False, False, True]) if crit not in ("xgb", "gbt2") else None
    b, edges = _finalize_builder(crit, cat)
    n_out = NS if crit in ("gini", "entropy") else 1
    for L in (1, 5, 1023, 1024, 1025, 3000):
        case = _finalize_case(crit, NS, L, seed=L + NS, min_gain=b.min_gain)
        ref = _check_finalize(b, case, edges, cat, 7 + L, heap, last, n_out, f"L={L}")
        if L >= 1023:
            split = ref["feats"] >= 0
            for i, kind in enumerate(FIN_PLANTS):
                assert bool(split[i]) == (i >= 6), kind          # the first six plants are refused
            assert ref["small_right"][ref["li"] if heap else np.arange(ref["n_split"])].any()
            k = int(np.nonzero(ref["li"] == 9)[0][0])            # equal children: small_right = 0
            assert ref["small_right"][9 if heap else k] == 0
            assert np.isposinf(ref["thrs"][8]) and (cat is None or ref["feats"][6] & CAT_FLAG)
            assert ref["feats"][7] & DLEFT_FLAG
    # small levels: each plant on its own, at every node of a 5-node level in turn
    for j, kind in enumerate(FIN_PLANTS):
        for L in (1, 5):
            case = _finalize_case(crit, NS, L, seed=j, min_gain=b.min_gain, only=(j % L, kind))
            _check_finalize(b, case, edges, cat, 3, heap, last, n_out, f"L={L} {kind}")


# =============================================================== 10. every GPU build path grows the same tree
def _compaction(sf, lc, rc):
    """Raw node id -> id in the materialised Tree (the reachable nodes in id order, as
    _tree_from_arrays keeps them)."""
    reach = np.zeros(len(sf), dtype=bool)
    reach[0] = True
    front = np.array([0])
    while front.size:
        sp = front[sf[front] >= 0]
        front = np.concatenate([lc[sp], rc[sp]])
        reach[front] = True
    remap = np.full(len(sf), -1, dtype=np.int64)
    remap[reach] = np.arange(int(reach.sum()))
    return remap


def _grow(monkeypatch, q, kind, stats, heap, route_fused, last_splits, identity=False, max_leaves=None, active=None,
          leaf_h=None, builder=None):
    """(tree, leaf of every row in the tree's numbering, importance) of one build under the given
    switches; ``builder``: a list that receives the HistTreeBuilder."""
    monkeypatch.setattr(T, "HEAP_TREES", heap)
    monkeypatch.setattr(T, "ROUTE_FUSED", route_fused)
    monkeypatch.setattr(T, "LAST_FROM_SPLITS", last_splits)
    n = stats.shape[0]
    b = HistTreeBuilder(q, kind, max_depth=6, min_samples_split=500, max_leaf_nodes=max_leaves, seed=1)
    if builder is not None:
        builder.append(b)
    kw = dict(act_rows=torch.arange(n, dtype=torch.int32, device="cuda"), identity_rows=True) if identity else {}
    out = b.build(stats, active=active, defer=True, leaf_h=leaf_h, **kw)
    raw = b.leaf_of_row.long().cpu().numpy()
    if isinstance(out, T.PendingTree):
        sf, _, lc, rc, _ = (a.cpu().numpy() for a in out.arrays)
        remap = _compaction(sf, lc, rc)
        tree, imp = out.materialize(), b.imp_dev.cpu().numpy()
    else:
        remap = np.arange(len(out.feature))
        tree, imp = out, b.importance
    leaf = np.where(raw >= 0, remap[np.maximum(raw, 0)], -1)
    return tree, leaf, imp


def _same_tree(a, b, tag):
    ta, la, ia = a
    tb, lb, ib = b
    for k in ("feature", "threshold", "left", "right", "value", "cat", "dleft"):
        assert getattr(ta, k) == getattr(tb, k), f"{tag}: {k}"
    np.testing.assert_array_equal(la, lb, err_msg=tag)
    np.testing.assert_allclose(ia, ib, rtol=1e-12, atol=0, err_msg=tag)


@gpu
@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("kind", ["gini", "variance"])
def test_every_gpu_build_path_grows_the_same_tree(monkeypatch, kind, missing):
    """HEAP_TREES x ROUTE_FUSED (with identity rows) x LAST_FROM_SPLITS, the row-list form of
    each layout and a run under an ``active`` mask select different level loops for the same
    mathematical tree.  The statistics are exact in fp32, so every path hands identical
    histograms to the same split kernel: the materialised trees, the leaf of every row (through
    the compaction of _tree_from_arrays) and the importance must equal those of the non-fused
    loop (max_leaves = 2^6 takes it and caps nothing at depth 6)."""
    n = 20000
    X, stats = _exact_tree_data(kind, n, seed=0)
    if missing:
        q = quantize(X.cuda(), 64, missing=True)             # bin 63 = NaN only, learned default directions
    else:                                                     # NaN shares the last bin with the largest values
        qs = torch.linspace(0, 1, 65)[1:-1]
        q = quantize(X.cuda(), 64, edges=torch.nanquantile(X.T.contiguous(), qs, dim=1).T.contiguous().cuda())
    stats = stats.cuda()
    base = _grow(monkeypatch, q, kind, stats, True, True, True, max_leaves=64)
    assert base[0].depth() == 6 and -1 in base[0].feature[:31] and len(base[0].feature) > 30
    assert (base[1] >= 0).all()
    for heap in (False, True):
        for last_splits in (False, True):
            for route_fused in (False, True):
                got = _grow(monkeypatch, q, kind, stats, heap, route_fused, last_splits, identity=True)
                _same_tree(got, base, f"heap={heap} last={last_splits} route_fused={route_fused} identity rows")
            got = _grow(monkeypatch, q, kind, stats, heap, True, last_splits)
            _same_tree(got, base, f"heap={heap} last={last_splits} row list")
    active = torch.rand(n, generator=torch.Generator().manual_seed(4)) < 0.8
    abase = _grow(monkeypatch, q, kind, stats, True, True, True, max_leaves=64, active=active.cuda())
    assert ((abase[1] < 0) == ~active.numpy()).all()
    for heap in (False, True):
        for last_splits in (False, True):
            got = _grow(monkeypatch, q, kind, stats, heap, True, last_splits, active=active.cuda())
            _same_tree(got, abase, f"heap={heap} last={last_splits} active mask")


@gpu
@pytest.mark.parametrize("kind", ["gini", "variance"])
def test_sort_fallback_grows_the_same_tree_on_gpu(monkeypatch, kind):
    """Levels with more keys than the counting-sort partition takes group the small children's
    rows by a stable sort.  With the limit patched to 2 every level from depth 2 on takes it, in
    both fused layouts (the heap level has L = 2^depth keys, the compact one its split count; with
    identity rows the fused route + count pass is bounded alike) and in the tensor loop on CUDA;
    each must grow the tree of the unpatched tensor loop."""
    n = 20000
    X, stats = _exact_tree_data(kind, n, seed=0)
    q = quantize(X.cuda(), 64, missing=True)
    stats = stats.cuda()
    base = _grow(monkeypatch, q, kind, stats, True, True, True, max_leaves=64)
    assert base[0].depth() == 6 and len(base[0].feature) > 30
    monkeypatch.setattr(T, "PARTITION_MAX_KEYS", 2)
    counted = []
    part, route_part = HistTreeBuilder._partition_gpu, HistTreeBuilder._route_partition_gpu

    def spy_part(act_rows, node_of_row, nb, lut, n_keys):
        counted.append(n_keys)
        return part(act_rows, node_of_row, nb, lut, n_keys)

    def spy_route_part(self, n_, node_of_row, nbuf, nb, lut, n_keys, lo):
        counted.append(n_keys)
        return route_part(self, n_, node_of_row, nbuf, nb, lut, n_keys, lo)

    monkeypatch.setattr(HistTreeBuilder, "_partition_gpu", staticmethod(spy_part))
    monkeypatch.setattr(HistTreeBuilder, "_route_partition_gpu", spy_route_part)
    # splitting nodes per level of the tree; the fused layouts group the children of levels 0 .. 4
    # (the last level's come from the split search), the tensor loop those of level 5 too
    splits, level = [], [0]
    while level:
        level = [k for k in level if base[0].feature[k] >= 0]
        splits.append(len(level))
        level = [c for k in level for c in (base[0].left[k], base[0].right[k])]
    assert max(splits[:5]) > 2
    configs = [("heap", dict(heap=True), [1, 2]),
               ("compact", dict(heap=False), [s for s in splits[:5] if 0 < s <= 2]),
               ("max_leaves", dict(heap=True, max_leaves=64), [s for s in splits[:6] if 0 < s <= 2])]
    for name, kw, within in configs:
        for identity in (False, True):
            del counted[:]
            got = _grow(monkeypatch, q, kind, stats, route_fused=True, last_splits=True, identity=identity, **kw)
            _same_tree(got, base, f"{name} identity={identity}")
            # only the levels within the limit reached the counting sort: the others were sorted
            assert counted == within, (name, identity, counted)


@gpu
@pytest.mark.parametrize("identity", [False, True])
def test_leaf_h_newton_leaves_in_both_fused_layouts(monkeypatch, identity):
    """criterion gbt2 on (w y, w) with per-row hessians k / 64: the leaves of a deferred tree hold
    fl32(sum r) / fl32(sum h) over their rows (leaf_newton_kernel's rule; both sums are exact in
    fp32: integers below 2^24 / 64), in the heap and the compact layout, with the last level's
    records from the split search or from histograms; all four materialise the same tree."""
    n = 20000
    X, stats = _exact_tree_data("variance", n, seed=0)
    q = quantize(X.cuda(), 64, missing=True)
    k = torch.randint(1, 65, (n,), generator=torch.Generator().manual_seed(11))
    leaf_h = k.float() / 64
    r64, h64 = stats[:, 0].double().numpy(), leaf_h.double().numpy()
    stats, leaf_h = stats.cuda(), leaf_h.cuda()
    first = None
    for heap in (True, False):
        for last_splits in (False, True):
            tag = f"heap={heap} last={last_splits}"
            bs = []
            got = _grow(monkeypatch, q, "gbt2", stats, heap, True, last_splits, identity=identity, leaf_h=leaf_h,
                        builder=bs)
            b = bs[0]
            assert (b.leaf_of_row.dtype == torch.int16) == heap, tag
            raw = b.leaf_of_row.long().cpu().numpy()
            assert (raw >= 0).all()
            vals = b.node_values.cpu().numpy()
            assert vals.shape[1] == 1
            leaves = np.unique(raw)
            assert len(leaves) > 16, tag
            sum_r = np.bincount(raw, weights=r64, minlength=len(vals))
            sum_h = np.bincount(raw, weights=h64, minlength=len(vals))
            want = np.float32(sum_r[leaves]) / np.float32(sum_h[leaves])
            np.testing.assert_array_equal(vals[leaves, 0], want, err_msg=tag)
            assert got[0].depth() == 6, tag
            if first is None:
                first = got
            else:
                _same_tree(got, first, tag)
