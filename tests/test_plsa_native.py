"""The native pLSA engine (csrc/kernels/plsa.hip, csrc/host/plsa_cpu.cpp, ops/plsa.py and
``train_plsa -engine native``) against an fp64 NumPy oracle of its contracts, one document at a
time.  The CPU twins run on every machine, the kernels under the ``gpu`` mark.

Tolerances are not chosen: the yardstick is the torch engine (``PLSA._doc_em`` and the M-step
lines of ``PLSA.fit``, fp32, on the CPU) on the same inputs against the same oracle.  Its largest
absolute error ``E_abs`` and largest relative error ``E_rel`` are measured per case, and the
kernels and twins, which add in another order (wave trees and LDS partials against
``index_add_``), get ``|x - ref| <= max(4 E_abs, 4 ulp * max|ref|)`` and
``|x - ref| <= max(4 E_rel, 4 ulp) * |ref|`` elementwise, with ulp = 2^-23.  Every quantity
compared is a product, quotient or sum of positive numbers, so the relative error is meaningful
down to small entries.

Measured (torch engine against the oracle; the bounds are four times these, floors aside):
    case (E_abs / E_rel of the torch engine)        pzd                 contrib
    7 iterations, K = 1                             0 / 0               0 / 0
    7 iterations, K = 3                             9.1e-8 / 3.0e-7     7.5e-7 / 5.0e-7
    7 iterations, K = 64 .. 256                     3.5e-8 .. 4.5e-8 /  1.6e-7 .. 3.4e-7 /
                                                    1.0e-6 .. 1.4e-6    1.3e-6 .. 1.6e-6
    one unstaged document, K = 64, 129, 256         5.7e-9 .. 3.3e-8 /  5.9e-8 .. 4.6e-7 /
                                                    8.0e-7 .. 1.4e-6    9.6e-7 .. 1.7e-6
    delta = 0.01 / K, K = 3 .. 256                  1.1e-7 .. 1.6e-7 /  7.9e-7 .. 1.3e-6 /
                                                    5.6e-7 .. 3.2e-6    8.3e-7 .. 3.4e-6
    M-step, K = 1, 65, 256, alpha = 0.5, 1          P(w|z): 1.2e-8 .. 1.8e-7 / 2.3e-8 .. 3.7e-7
                                                    (alpha = 1 with one word: 0 / 0)
    fit, one document per mini-batch, K = 3         P(w|z): 2.0e-8 / 3.4e-7

so the bounds are 1.4e-7 .. 6.3e-7 absolute and 4.8e-7 .. 1.3e-5 relative on ``pzd``, 2.4e-7 ..
5.2e-6 and 4.8e-7 .. 1.4e-5 on ``contrib``, 6.5e-8 .. 7.1e-7 and 4.8e-7 .. 1.5e-6 on P(w|z) (4.8e-7
is the 4 ulp floor).  The kernels' and twins' own errors print with ``pytest -s``; the largest
share of a bound any of them uses is 87 % (M-step, K = 256, one batch word: 1.0e-6 of 1.15e-6
relative, on the CPU and the GPU alike, since both add a column's rows in the same fixed order).
Relative errors are taken on entries of at least 1e-30: after 50 iterations an entry of ``pzd`` can
fall below fp32's normal range, where only the absolute bound means anything.

A test with ``delta > 0`` compares iteration counts exactly, so it first asserts on the oracle
alone that no document's change comes within 1e-3 (relative) of ``delta`` at any iteration (fp32
rounding, ~1e-6 relative on ``ch``, cannot move a stop) and that the counts take at least three
distinct values below the cap.  The seeds of those cases were picked for these two conditions."""
import numpy as np
import pandas as pd
import pytest
import torch

from hivemall_amd.models.topicmodel import PLSA
from hivemall_amd.utils.options import UDFArgumentException

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
ULP = 2.0 ** -23
TINY = 1e-30               # relative errors are taken on entries at least this large
B, V = 33, 97
CAP = 50


def _ops():
    from hivemall_amd.ops import plsa

    return plsa


# ------------------------------------------------------------------------------ fp64 oracle
def _posterior(p, Pw):
    q = p * Pw
    return q / np.maximum(q.sum(1, keepdims=True), 1e-30)


def oracle_doc_em(doc_off, wid, cnt, pwzT, delta, max_iter):
    """The EM contract in fp64: (pzd, contrib, iters, every document's ch per iteration)."""
    pwzT, cnt = pwzT.astype(np.float64), cnt.astype(np.float64)
    nB, K = len(doc_off) - 1, pwzT.shape[1]
    pzd, contrib = np.zeros((nB, K)), np.zeros((len(wid), K))
    iters, chs = np.zeros(nB, dtype=np.int32), [[] for _ in range(nB)]
    for d in range(nB):
        a, b = doc_off[d], doc_off[d + 1]
        if a == b:
            continue
        Pw, c, p = pwzT[wid[a:b]], cnt[a:b, None], np.full(K, 1.0 / K)
        for _ in range(max_iter):
            new = (c * _posterior(p, Pw)).sum(0)
            new /= max(new.sum(), 1e-30)
            chs[d].append(np.abs(new - p).mean())
            p = new
            iters[d] += 1
            if chs[d][-1] < delta:
                break
        pzd[d], contrib[a:b] = p, c * _posterior(p, Pw)
    return pzd, contrib, iters, chs


def oracle_mstep(word_off, perm, uniq, contrib, alpha, pwzT):
    """The M-step contract in fp64."""
    p, contrib = pwzT.astype(np.float64), contrib.astype(np.float64)
    nwz = np.stack([contrib[perm[word_off[u]:word_off[u + 1]]].sum(0) for u in range(len(uniq))])
    p = (1 - alpha) * p
    p[uniq] += alpha * nwz / np.maximum(nwz.sum(0), 1e-30)
    return p / p.sum(0)


# ------------------------------------------------------------------------------ inputs
def _pwzT(rng, K, nV=V, boost=6.0):
    """P(w|z) transposed [V, K] f32: alternate topics favour one half of the vocabulary."""
    P = rng.random((K, nV)) + 0.05
    first = np.arange(nV) < nV // 2
    for k in range(K):
        P[k, first if k % 2 == 0 else ~first] *= boost
    return np.ascontiguousarray((P / P.sum(1, keepdims=True)).T.astype(np.float32))


def _docs(rng, lens, nV=V):
    """CSR non-zeros of documents of the given lengths: distinct words inside a document, words
    shared between documents, non-integer counts."""
    doc_off = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=doc_off[1:])
    wid = np.concatenate([rng.choice(nV, size=n, replace=False) for n in lens] + [np.zeros(0, np.int64)])
    cnt = (rng.random(len(wid)) * 4 + 0.25).astype(np.float32)
    return doc_off, wid.astype(np.int32), cnt


def _lens(rng):
    return [0, 1, 2, 3, 4, 5, 63, 64, 65] + [int(x) for x in rng.integers(2, 91, size=B - 9)]


_CASES: dict = {}


def _em_case(kind, K, seed):
    """One EM problem, its oracle and the torch yardstick, computed once and left unchanged."""
    key = (kind, K, seed)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(seed)
    if kind == "long":                      # one document past the staging limit of the kernel
        n = _ops().EM_STAGE_FLOATS // K + 1
        assert n <= 4 * V
        doc_off, wid, cnt = _docs(rng, [n], nV=4 * V)
        pwzT = _pwzT(rng, K, nV=4 * V)
    else:
        doc_off, wid, cnt = _docs(rng, _lens(rng))
        pwzT = _pwzT(rng, K)
    delta, cap = (0.0, 7) if kind != "stop" else (0.01 / K, CAP)
    ref = oracle_doc_em(doc_off, wid, cnt, pwzT, delta, cap)
    # the torch engine; per document when documents stop alone (one document per call: its
    # batch-mean rule is then the per-document rule)
    m = PLSA(f"-topics {K} -engine torch -delta {delta!r}", device="cpu")
    m.pwz = torch.from_numpy(pwzT.T.copy())
    w_t, c_t = torch.from_numpy(wid.astype(np.int64)), torch.from_numpy(cnt)
    nB = len(doc_off) - 1
    if kind == "stop":
        pz, cb = torch.zeros(nB, K), torch.zeros(len(wid), K)
        for d in range(nB):
            a, b = int(doc_off[d]), int(doc_off[d + 1])
            if a < b:
                p, q = m._doc_em(torch.zeros(b - a, dtype=torch.int64), w_t[a:b], c_t[a:b], 1, cap)
                pz[d], cb[a:b] = p[0], q * c_t[a:b, None]
    else:
        doc = torch.repeat_interleave(torch.arange(nB), torch.from_numpy(np.diff(doc_off).astype(np.int64)))
        pz, q = m._doc_em(doc, w_t, c_t, nB, cap)
        cb = q * c_t[:, None]
    case = dict(doc_off=doc_off, wid=wid, cnt=cnt, pwzT=pwzT, delta=delta, cap=cap, ref=ref,
                bounds=(_bounds(pz.numpy(), ref[0]), _bounds(cb.numpy(), ref[1])))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[key] = case
    return case


def _errors(x, ref):
    err = np.abs(np.asarray(x, dtype=np.float64) - ref)
    pos = ref >= TINY
    return float(err.max(initial=0.0)), float((err[pos] / ref[pos]).max(initial=0.0))


def _bounds(yardstick, ref):
    """(atol, rtol) from the torch engine's error against the oracle: 4x, floored at 4 ulp."""
    e_abs, e_rel = _errors(yardstick, ref)
    return max(4 * e_abs, 4 * ULP * float(np.abs(ref).max(initial=0.0))), max(4 * e_rel, 4 * ULP)


def _assert_within(x, ref, bounds, what):
    atol, rtol = bounds
    x = np.asarray(x, dtype=np.float64)
    err = np.abs(x - ref)
    e_abs, e_rel = _errors(x, ref)
    print(f"{what}: abs err {e_abs:.3g} (bound {atol:.3g}), rel err {e_rel:.3g} (bound {rtol:.3g})")
    assert np.isfinite(x).all(), what
    assert (err <= atol).all(), f"{what}: abs err {e_abs:.3g} > {atol:.3g}"
    assert (err <= rtol * np.abs(ref))[ref >= TINY].all(), f"{what}: rel err {e_rel:.3g} > {rtol:.3g}"


def _run_em(case, device):
    t = lambda a: torch.from_numpy(np.array(a)).to(device)
    pzd, contrib, iters = _ops().plsa_doc_em(t(case["doc_off"]), t(case["wid"]), t(case["cnt"]), t(case["pwzT"]),
                                             case["delta"], case["cap"])
    assert pzd.dtype == contrib.dtype == torch.float32 and iters.dtype == torch.int32
    assert pzd.device.type == contrib.device.type == iters.device.type == device
    return pzd.cpu().numpy(), contrib.cpu().numpy(), iters.cpu().numpy()


# ------------------------------------------------------------------------------ EM
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("K", [1, 3, 64, 65, 128, 129, 256])
def test_em_fixed_iterations_match_oracle(K, device):
    case = _em_case("fixed", K, 500 + K)
    lens = np.diff(case["doc_off"])
    assert {0, 1, 2, 3, 4, 5, 63, 64, 65} <= set(lens.tolist()) and len(lens) == B
    assert np.bincount(case["wid"], minlength=V).max() > 1 and (case["cnt"] % 1 != 0).all()
    pzd, contrib, iters = _run_em(case, device)
    ref_pzd, ref_contrib, ref_iters, _ = case["ref"]
    assert (ref_iters[lens > 0] == 7).all()
    np.testing.assert_array_equal(iters, ref_iters)
    assert iters[0] == 0 and not pzd[0].any()                 # the empty document
    _assert_within(pzd, ref_pzd, case["bounds"][0], f"pzd K={K} {device}")
    _assert_within(contrib, ref_contrib, case["bounds"][1], f"contrib K={K} {device}")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("K", [64, 129, 256])
def test_em_single_document_past_the_staging_limit(K, device):
    P = _ops()
    case = _em_case("long", K, 900 + K)
    assert len(case["doc_off"]) == 2 and int(case["doc_off"][1]) * K > P.EM_STAGE_FLOATS
    if device == "cuda":
        from hivemall_amd import _native

        assert _native.hip().hm_plsa_stage_floats() == P.EM_STAGE_FLOATS
    pzd, contrib, iters = _run_em(case, device)
    assert iters.tolist() == [7]
    _assert_within(pzd, case["ref"][0], case["bounds"][0], f"long pzd K={K} {device}")
    _assert_within(contrib, case["ref"][1], case["bounds"][1], f"long contrib K={K} {device}")


STOP_SEEDS = {3: 1008, 10: 1010, 64: 1076, 65: 1070, 130: 1130, 256: 1256}


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("K", sorted(STOP_SEEDS))
def test_em_documents_stop_on_their_own_change(K, device):
    case = _em_case("stop", K, STOP_SEEDS[K])
    ref_pzd, ref_contrib, ref_iters, chs = case["ref"]
    # on the oracle alone: the stops are spread out and none is a matter of rounding
    assert len({int(i) for i in ref_iters if 0 < i < CAP}) >= 3, sorted(set(ref_iters.tolist()))
    assert all(abs(ch / case["delta"] - 1) >= 1e-3 for doc in chs for ch in doc)
    pzd, contrib, iters = _run_em(case, device)
    np.testing.assert_array_equal(iters, ref_iters)
    _assert_within(pzd, ref_pzd, case["bounds"][0], f"stop pzd K={K} {device}")
    _assert_within(contrib, ref_contrib, case["bounds"][1], f"stop contrib K={K} {device}")
    np.testing.assert_allclose(pzd[1:].sum(1), 1.0, atol=8 * ULP)


@pytest.mark.parametrize("device", DEVICES)
def test_em_zero_iterations_and_empty_batch(device):
    P = _ops()
    case = _em_case("fixed", 3, 503)
    t = lambda a: torch.from_numpy(np.array(a)).to(device)
    pzd, contrib, iters = P.plsa_doc_em(t(case["doc_off"]), t(case["wid"]), t(case["cnt"]), t(case["pwzT"]), 0.0, 0)
    assert not iters.any() and not pzd[0].any()
    np.testing.assert_array_equal(pzd[1:].cpu().numpy(), np.float32(1.0) / np.float32(3))
    ref = oracle_doc_em(case["doc_off"], case["wid"], case["cnt"], case["pwzT"], 0.0, 0)
    np.testing.assert_allclose(contrib.cpu().numpy(), ref[1], rtol=8 * ULP, atol=0)
    none = torch.zeros(1, dtype=torch.int32, device=device)
    empty = torch.zeros(0, dtype=torch.int32, device=device)
    pzd, contrib, iters = P.plsa_doc_em(none, empty, empty.float(), t(case["pwzT"]), 0.0, 5)
    assert pzd.shape == (0, 3) and contrib.shape == (0, 3) and iters.shape == (0,)


# ------------------------------------------------------------------------------ M-step
def _torch_mstep(w, contrib, alpha, pwz):
    """The P(w|z) update of PLSA.fit (``contrib`` = q * cnt), fp32 on the CPU: the yardstick."""
    nwz = torch.zeros_like(pwz).index_add_(1, w, contrib.T)
    upd = nwz / nwz.sum(1, keepdim=True).clamp_min(1e-30)
    pwz = (1 - alpha) * pwz + alpha * upd
    return pwz / pwz.sum(1, keepdim=True)


def _mstep_case(K, alpha, single):
    key = ("m", K, alpha, single)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(7000 + K)
    nV = 600                                # ten row blocks of the kernels, the last partial
    if single:                              # U = 1: every non-zero is the same word
        wid = np.full(5, 11, dtype=np.int32)
    else:                                   # repeated words; most of V absent; one long run
        wid = np.concatenate([rng.choice(100, size=n, replace=False) * 2 for n in (1, 40, 90, 60)]
                             + [np.full(70, 8), np.array([nV - 1, 300, nV - 1])]).astype(np.int32)
    contrib = (rng.random((len(wid), K)) * 3).astype(np.float32)
    pwzT = _pwzT(rng, K, nV=nV)
    perm, word_off, uniq = (t.numpy() for t in _ops().batch_index(torch.from_numpy(wid)))
    ref = oracle_mstep(word_off, perm, uniq, contrib, alpha, pwzT)
    yard = _torch_mstep(torch.from_numpy(wid.astype(np.int64)), torch.from_numpy(contrib), alpha,
                        torch.from_numpy(pwzT.T.copy())).T.numpy()
    case = dict(wid=wid, contrib=contrib, pwzT=pwzT, perm=perm, word_off=word_off, uniq=uniq, ref=ref,
                bounds=_bounds(yard, ref))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[key] = case
    return case


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("single", [False, True], ids=["batch", "U1"])
@pytest.mark.parametrize("alpha", [0.5, 1.0])
@pytest.mark.parametrize("K", [1, 65, 256])
def test_mstep_matches_oracle_and_repeats_bit_for_bit(K, alpha, single, device):
    P = _ops()
    case = _mstep_case(K, alpha, single)
    t = lambda a: torch.from_numpy(np.array(a)).to(device)
    uniq, nV = case["uniq"], case["pwzT"].shape[0]
    assert len(uniq) == (1 if single else len(set(case["wid"].tolist()))) and len(uniq) < nV // 2
    assert single or np.diff(case["word_off"]).max() > 4      # words repeat inside the batch
    outs = []
    for _ in range(2):
        pw = t(case["pwzT"])
        out = P.plsa_mstep(t(case["word_off"]), t(case["perm"]), t(case["uniq"]), t(case["contrib"]), alpha, pw,
                           wid=t(case["wid"]))
        assert out is pw
        outs.append(pw.cpu())
    assert torch.equal(outs[0], outs[1])
    got = outs[0].numpy()
    _assert_within(got, case["ref"], case["bounds"], f"mstep K={K} alpha={alpha} U={len(uniq)} {device}")
    np.testing.assert_allclose(got.astype(np.float64).sum(0), 1.0, atol=nV * ULP)
    absent = np.setdiff1d(np.arange(nV), uniq)
    if alpha == 1.0:
        assert not got[absent].any() and got[uniq].all()
    else:
        assert got[absent].all()
    # a caller's larger scratch is accepted and gives the same bits
    pw = t(case["pwzT"])
    big = P.mstep_scratch(nV, nV, K, device)
    P.plsa_mstep(t(case["word_off"]), t(case["perm"]), t(case["uniq"]), t(case["contrib"]), alpha, pw, big)
    assert torch.equal(pw.cpu(), outs[0])


# ------------------------------------------------------------------------------ learner
def _two_vocab_docs():
    """The corpus of test_plsa_separates_topics."""
    return [["apple", "banana", "cherry", "apple"], ["banana", "cherry", "apple"],
            ["cpu", "gpu", "kernel", "gpu"], ["kernel", "cpu", "gpu"]] * 6


def _tie_docs():
    rng = np.random.default_rng(77)
    words = [f"w{i}" for i in range(23)]
    docs = [[f"{words[i]}:{rng.random() * 3 + 0.5:.3f}" for i in rng.choice(23, size=n, replace=False)]
            for n in (1, 2, 5, 9, 13, 23, 4, 7, 11, 3, 6, 17)]
    return docs


def _oracle_fit(rows, pwz0, alpha, inner, epochs):
    """One document per mini-batch, fixed inner iterations, in fp64 from the oracle functions."""
    pwzT = pwz0.T.astype(np.float64)
    for _ in range(epochs):
        for r in rows:
            wid = np.array([i for i, _ in r], dtype=np.int32)
            cnt = np.array([c for _, c in r], dtype=np.float32)
            _, contrib, _, _ = oracle_doc_em(np.array([0, len(r)]), wid, cnt, pwzT, 0.0, inner)
            order = np.argsort(wid, kind="stable")
            uniq, counts = np.unique(wid, return_counts=True)
            word_off = np.concatenate([[0], np.cumsum(counts)])
            pwzT = oracle_mstep(word_off, order, uniq, contrib, alpha, pwzT)
    return pwzT.T


@pytest.mark.parametrize("device", DEVICES)
def test_fit_native_ties_to_torch_engine_with_one_document_per_batch(device):
    """-mini_batch_size 1: the batch-mean stop and the per-document stop are one rule, so the two
    engines compute the same model up to fp32 summation order."""
    opts = "-topics 3 -mini_batch_size 1 -delta 0 -max_inner_iters 5 -iters 2 -seed 5 -engine "
    docs = _tie_docs()
    ref_m = PLSA(opts + "torch", device="cpu")
    rows = ref_m.vocab.encode(docs, add=True)
    ref_m._grow(len(ref_m.vocab.words))
    start = ref_m.pwz.clone().numpy()
    ref_m.fit(docs)
    oracle = _oracle_fit(rows, start, 0.5, 5, 2)
    native = PLSA(opts + "native", device=device).fit(docs)
    assert native.pwz.shape == ref_m.pwz.shape == (3, 23) and native.pwz.is_contiguous()
    _assert_within(native.pwz.cpu().numpy(), oracle, _bounds(ref_m.pwz.numpy(), oracle), f"fit pwz {device}")


@pytest.mark.parametrize("device", DEVICES)
def test_native_model_separates_topics_and_transforms(device):
    m = PLSA("-topics 2 -iters 5 -engine native", device=device).fit(_two_vocab_docs())
    tab = m.model_table()
    assert list(tab.columns) == ["label", "word", "prob"] and len(tab) == 2 * 6
    top = {k: set(tab[tab.label == k].sort_values("prob", ascending=False).word.head(3)) for k in (0, 1)}
    assert sorted(map(sorted, top.values())) == [["apple", "banana", "cherry"], ["cpu", "gpu", "kernel"]]
    theta = m.transform([["apple", "banana"], ["gpu", "kernel", "cpu"], ["unseen"]])
    np.testing.assert_allclose(theta[:2].sum(1), 1.0, atol=8 * ULP)
    assert theta[0].argmax() != theta[1].argmax() and not theta[2].any()


def test_train_plsa_sql_engine_option():
    from hivemall_amd.sql import Session

    s = Session(device="cpu")
    s.register("docs", pd.DataFrame({"words": _two_vocab_docs()}))
    q = "SELECT train_plsa(words, '-topics 2 -engine {}') AS (label, word, prob) FROM docs"
    tab = s.sql(q.format("native"))
    assert list(tab.columns) == ["label", "word", "prob"] and len(tab) == 2 * 6
    np.testing.assert_allclose(tab.groupby("label")["prob"].sum().to_numpy(), 1.0, atol=1e-5)
    with pytest.raises(UDFArgumentException, match="engine"):
        s.sql(q.format("bogus"))


def test_engine_option_resolution():
    with pytest.raises(UDFArgumentException, match="engine"):
        PLSA("-engine bogus", device="cpu")
    with pytest.raises(UDFArgumentException, match="256"):
        PLSA("-engine native -topics 300", device="cpu")
    docs = _two_vocab_docs()
    wide = PLSA("-engine auto -topics 300 -iters 1", device="cpu")
    assert wide.engine() == "torch" and wide.fit(docs).pwz.shape == (300, 6)
    assert PLSA("", device="cpu").engine() == "torch"
    assert PLSA("-engine native", device="cpu").engine() == "native"
    a = PLSA("-topics 4 -seed 3 -engine auto", device="cpu").fit(docs)
    b = PLSA("-topics 4 -seed 3 -engine torch", device="cpu").fit(docs)
    assert torch.equal(a.pwz, b.pwz)


@pytest.mark.gpu
def test_engine_auto_on_a_gpu():
    assert PLSA("-topics 256", device="cuda").engine() == "native"
    assert PLSA("-topics 257", device="cuda").engine() == "torch"
    with pytest.raises(UDFArgumentException, match="256"):
        PLSA("-engine native -topics 257", device="cuda")


def test_max_inner_iters_caps_both_engines():
    docs = _two_vocab_docs()
    for engine in ("torch", "native"):
        one = PLSA(f"-topics 2 -seed 1 -delta 0 -max_inner_iters 1 -iters 1 -engine {engine}", device="cpu").fit(docs)
        many = PLSA(f"-topics 2 -seed 1 -delta 0 -iters 1 -engine {engine}", device="cpu").fit(docs)
        assert not torch.equal(one.pwz, many.pwz)


# ------------------------------------------------------------------------------ validation
def test_malformed_inputs_raise_before_any_launch():
    """CPU tensors only: nothing malformed is ever handed to a device launch."""
    P = _ops()
    case = _em_case("fixed", 3, 503)
    t = lambda a: torch.from_numpy(np.array(a))
    doc_off, wid, cnt, pwzT = t(case["doc_off"]), t(case["wid"]), t(case["cnt"]), t(case["pwzT"])
    N = wid.numel()
    good = (doc_off, wid, cnt, pwzT, 0.0, 3)
    P.plsa_doc_em(*good)

    def em_bad(i, v, match=None):
        args = list(good)
        args[i] = v
        with pytest.raises(ValueError, match=match):
            P.plsa_doc_em(*args)

    em_bad(0, doc_off.long())
    em_bad(1, wid.long())
    em_bad(2, cnt.double())
    em_bad(3, pwzT.double())
    em_bad(3, pwzT[:, 0])
    em_bad(1, wid.numpy())
    em_bad(2, cnt[:-1])
    em_bad(5, -1, "max_iter")
    em_bad(3, torch.zeros(V, 257), "256")
    em_bad(3, torch.zeros(V, 0))
    shifted = doc_off.clone()
    shifted[0] = 1
    em_bad(0, shifted, "doc_off")
    falling = doc_off.clone()
    falling[3], falling[4] = doc_off[4], doc_off[3]
    em_bad(0, falling, "doc_off")
    em_bad(0, doc_off[:-1], "doc_off")                        # does not end at N
    for v in (-1, V):
        w = wid.clone()
        w[5] = v
        em_bad(1, w, "word ids")
    em_bad(3, pwzT.to("meta"), "is on")                       # devices differ

    perm, word_off, uniq = P.batch_index(wid)
    contrib = torch.rand(N, 3)
    mgood = [word_off, perm, uniq, contrib, 0.5, pwzT.clone()]
    P.plsa_mstep(*mgood, wid=wid)

    def m_bad(i, v, match=None, **kw):
        args = list(mgood)
        args[i] = v
        before = args[5].clone() if isinstance(args[5], torch.Tensor) else None
        with pytest.raises(ValueError, match=match):
            P.plsa_mstep(*args, **kw)
        if before is not None:
            assert torch.equal(args[5], before)               # rejected before anything ran

    m_bad(0, word_off.long())
    m_bad(1, perm.long())
    m_bad(2, uniq.long())
    m_bad(3, contrib.double())
    m_bad(3, contrib[:-1], "contrib")
    m_bad(3, torch.rand(N, 4), "contrib")
    m_bad(5, pwzT.T, "contiguous|topics")
    m_bad(5, pwzT.T.contiguous().T, "contiguous")
    dup = perm.clone()
    dup[0] = perm[1]
    m_bad(1, dup, "permutation")
    out = perm.clone()
    out[0] = N
    m_bad(1, out, "permutation")
    run = int(torch.nonzero(word_off[1:] - word_off[:-1] > 1)[0])
    a = int(word_off[run])
    swapped = perm.clone()
    swapped[a], swapped[a + 1] = perm[a + 1], perm[a]
    m_bad(1, swapped, "ascend")
    moved = perm.clone()                                      # a valid permutation for other words
    moved[0], moved[-1] = perm[-1], perm[0]
    m_bad(1, moved, "ascend|sorted index", wid=wid)
    m_bad(0, word_off[:-1], "word_off")
    short = word_off.clone()
    short[-1] = N - 1
    m_bad(0, short, "word_off")
    desc = uniq.clone()
    desc[0], desc[1] = uniq[1], uniq[0]
    m_bad(2, desc, "ascending")
    far = uniq.clone()
    far[-1] = V
    m_bad(2, far, "ascending")
    with pytest.raises(ValueError, match="scratch"):
        P.plsa_mstep(*mgood, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        P.batch_index(wid.long())
