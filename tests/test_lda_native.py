"""The native LDA engine (csrc/kernels/lda.hip, csrc/host/lda_cpu.cpp, ops/lda.py and ``train_lda
-engine native``) against an fp64 NumPy reference of its contracts.  The CPU twins run on every
machine, the kernels under the ``gpu`` mark.

Tolerances are not chosen.  Every step exists three times with one signature: ``REF`` (fp64), ``YARD``
(the torch formulation of ``LDA.fit`` / ``LDA.e_step`` in fp32 on the CPU) and ``_native(device)``.
``YARD``'s largest absolute and relative error against ``REF`` on the same inputs, times four and
floored at 4 fp32 ulp, bounds the native result elementwise (``_bounds``; the rule of
tests/test_plsa_native.py).  The fp64 ``bound`` output is held to the same rule.  Errors and
bounds print with ``pytest -s``.

The E-step cases run with ``alpha = 1``, but for a one-iteration case at the default ``1 / K``.  An entry of ``gamma`` near ``alpha`` amplifies a relative
perturbation by about ``1 / gamma`` per inner iteration (digamma' ~ 1 / gamma^2); with ``alpha = 1 / K``
every fp32 implementation's error is rounding noise times a large random factor and the ratio of
two implementations' errors (all this rule looks at) is heavy-tailed.  With ``gamma >= 1`` the
factor stays below 1.65 and the comparison measures the arithmetic.  On an MI355X the kernels use
at most 58 % of a bound (batch_eb, K = 1, U = 37: 1.44e-6 of 5.91e-6 relative)."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch
from scipy.special import digamma

from hivemall_amd import _native as _hm
from hivemall_amd.models.topicmodel import LDA
from hivemall_amd.ops import lda as L
from hivemall_amd.utils.options import UDFArgumentException

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
ULP, TINY = 2.0 ** -23, 1e-30
V = 101
LENS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 17, 40)
ALPHA = 1.0
f64 = lambda *xs: [np.asarray(x, dtype=np.float64) for x in xs]
f32t = lambda *xs: [torch.tensor(np.asarray(x), dtype=torch.float32) for x in xs]


def ref_eb(uniq, lamT, T):
    lamT, T = f64(lamT, T)
    return np.exp(digamma(lamT[uniq]) - digamma(T))


def ref_estep(doc_off, wpos, cnt, EbU, gamma, alpha, delta, max_iter):
    cnt, EbU, gamma = f64(cnt, EbU, gamma)
    nB, et = len(doc_off) - 1, lambda x: np.exp(digamma(x) - digamma(x.sum()))
    gamma, contrib, iters, bound = gamma.copy(), np.zeros((len(wpos), EbU.shape[1])), np.zeros(nB, np.int32), np.zeros(nB)
    changes = []                                # every document's mean change, per iteration
    for d in range(nB):
        a, b = doc_off[d], doc_off[d + 1]
        if a == b:
            gamma[d] = alpha
            continue
        E, c, x = EbU[wpos[a:b]], cnt[a:b], gamma[d]
        for _ in range(max_iter):
            Et = et(x)
            new = alpha + Et * ((c / (E @ Et + 1e-30)) @ E)
            changes.append(np.abs(new - x).mean())
            x, iters[d] = new, iters[d] + 1
            if changes[-1] < delta:
                break
        ph = E @ et(x) + 1e-30
        gamma[d], contrib[a:b], bound[d] = x, et(x) * E * (c / ph)[:, None], (c * np.log(ph)).sum()
    return gamma, contrib, iters, bound, changes


def ref_mstep(word_off, perm, uniq, contrib, rho, eta, scale, lamT, T):
    contrib, lamT = f64(contrib, lamT)
    s = np.zeros_like(lamT)
    for u, w in enumerate(uniq):
        s[w] = contrib[perm[word_off[u]:word_off[u + 1]]].sum(0)
    lamT = (1 - rho) * lamT + rho * (eta + scale * s)
    return lamT, lamT.sum(0)


def yard_eb(uniq, lamT, T):
    lamT, T = f32t(lamT, T)
    return torch.exp(torch.digamma(lamT[torch.tensor(uniq).long()]) - torch.digamma(T)).numpy()


def yard_estep(doc_off, wpos, cnt, EbU, gamma, alpha, delta, max_iter):
    c, EbU, gamma = f32t(cnt, EbU, gamma)
    nB, K = gamma.shape
    doc = torch.repeat_interleave(torch.arange(nB), torch.as_tensor(np.diff(doc_off)).long())
    Eb, active = EbU[torch.tensor(wpos).long()], torch.ones(nB, dtype=torch.bool)
    elog = lambda g: torch.digamma(g) - torch.digamma(g.sum(1, keepdim=True))
    for _ in range(max_iter):
        Et = torch.exp(elog(gamma))
        phinorm = (Et[doc] * Eb).sum(1) + 1e-30
        new = torch.full((nB, K), float(alpha)).index_add_(0, doc, Et[doc] * Eb * (c / phinorm)[:, None])
        change = (new - gamma).abs().mean(1)
        gamma = torch.where(active[:, None], new, gamma)
        active &= change >= delta
        if not bool(active.any()):
            break
    if max_iter == 0:
        gamma[torch.as_tensor(np.diff(doc_off) == 0)] = alpha
    Et = torch.exp(elog(gamma))
    phinorm = (Et[doc] * Eb).sum(1) + 1e-30
    bound = torch.zeros(nB).index_add_(0, doc, c * torch.log(phinorm))
    return gamma.numpy(), (Et[doc] * Eb * (c / phinorm)[:, None]).numpy(), None, bound.numpy()


def yard_mstep(word_off, perm, uniq, contrib, rho, eta, scale, lamT, T):
    contrib, lamT = f32t(contrib, lamT)
    w = torch.as_tensor(np.repeat(uniq, np.diff(word_off))).long()
    sstats = torch.zeros_like(lamT).index_add_(0, w, contrib[torch.tensor(perm).long()])
    lamT = (1 - rho) * lamT + rho * (eta + scale * sstats)
    return lamT.numpy(), lamT.sum(0).numpy()


REF, YARD = (ref_eb, ref_estep, ref_mstep), (yard_eb, yard_estep, yard_mstep)


def _native(device):
    t = lambda a: torch.from_numpy(np.array(a)).to(device)
    n = lambda xs: tuple(x.cpu().numpy() for x in xs)
    return (lambda uniq, lamT, T: L.lda_batch_eb(t(uniq), t(lamT), t(T)).cpu().numpy(),
            lambda *a: n(L.lda_doc_estep(*map(t, a[:5]), *a[5:])),
            lambda *a: n(L.lda_mstep(*map(t, a[:4]), *a[4:7], t(a[7]), t(a[8]))))


def _errors(x, ref, rel=True):
    """Largest absolute and relative error; relative on entries of at least TINY and inside ``rel``."""
    err, pos = np.abs(np.asarray(x, dtype=np.float64) - ref), (np.abs(ref) >= TINY) & rel
    return float(err.max(initial=0.0)), float((err[pos] / np.abs(ref[pos])).max(initial=0.0))


def _bounds(yard, ref, rel=True):
    e_abs, e_rel = _errors(yard, ref, rel)
    return max(4 * e_abs, 4 * ULP * float(np.abs(ref).max(initial=0.0))), max(4 * e_rel, 4 * ULP)


def _assert_within(x, yard, ref, what, rel=True):
    (atol, rtol), (e_abs, e_rel) = _bounds(yard, ref, rel), _errors(x, ref, rel)
    print(f"{what}: abs err {e_abs:.3g} (bound {atol:.3g}), rel err {e_rel:.3g} (bound {rtol:.3g})")
    err = np.abs(np.asarray(x, dtype=np.float64) - ref)
    assert np.isfinite(x).all() and (err <= atol).all(), f"{what}: abs err {e_abs:.3g} > {atol:.3g}"
    assert (err <= rtol * np.abs(ref))[(np.abs(ref) >= TINY) & rel].all(), f"{what}: rel err {e_rel:.3g} > {rtol:.3g}"


@functools.lru_cache(maxsize=None)
def _batch(seed, K, lens=LENS, nV=V, wide=False):
    """One mini-batch (words repeat across documents, non-integer counts), its index, gamma0 and a
    table as a fit has it (Gamma(100, 100) draws, alternate topics favouring one half of the
    vocabulary) or, ``wide``, with entries from 1e-3 to 1e3; computed once, read-only."""
    rng = np.random.default_rng(seed)
    doc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    wid = np.concatenate([rng.choice(nV, size=n, replace=n > nV) for n in lens]).astype(np.int32)
    wid[:2] = 0, nV - 1
    perm, word_off, uniq = (x.numpy() for x in L.batch_index(torch.from_numpy(wid)))
    lamT = rng.gamma(100.0, 0.01, size=(nV, K)) * np.where((np.arange(nV)[:, None] < nV // 2) ^ (np.arange(K) % 2 > 0), 6, 1)
    lamT = (10.0 ** rng.uniform(-3, 3, size=(nV, K)) if wide else lamT).astype(np.float32)
    c = dict(doc_off=doc_off, wid=wid, cnt=(rng.random(len(wid)) * 4 + 0.25).astype(np.float32), perm=perm,
             word_off=word_off, uniq=uniq, wpos=L.word_positions(torch.from_numpy(wid), torch.from_numpy(uniq)).numpy(),
             lamT=lamT, T=lamT.sum(0, dtype=np.float64).astype(np.float32),
             gamma=rng.gamma(100.0, 0.01, size=(len(lens), K)).astype(np.float32))
    c["EbU"] = ref_eb(uniq, lamT, c["T"]).astype(np.float32)
    for v in c.values():
        v.setflags(write=False)
    return c


def _check_estep(c, device, alpha, delta, max_iter, what):
    args = (c["doc_off"], c["wpos"], c["cnt"], c["EbU"], c["gamma"], alpha, delta, max_iter)
    ref, yard, got = ref_estep(*args), yard_estep(*args), _native(device)[1](*args)
    # contrib = Et * Eb * cnt / phinorm: where Et or Et * Eb is not a normal fp32 number (a binade of
    # margin for the rounding of exp's argument) the kernel's __expf, arithmetic the E-step keeps, gives 0
    # and the CPU a few bits: only the absolute bound holds there
    et = np.repeat(np.exp(digamma(ref[0]) - digamma(ref[0].sum(1, keepdims=True))), np.diff(c["doc_off"]), axis=0)
    normal = np.minimum(et, et * c["EbU"][c["wpos"]]) >= 2.0 ** -125
    for i, name, rel in ((0, "gamma", True), (1, "contrib", normal), (3, "bound", True)):
        _assert_within(got[i], yard[i], ref[i], f"{what} {name} {device}", rel)
    np.testing.assert_array_equal(got[2], ref[2])
    empty = np.diff(c["doc_off"]) == 0
    assert (got[0][empty] == np.float32(alpha)).all() and not got[3][empty].any() and got[3].dtype == np.float64
    return ref


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("U", [1, 37])
@pytest.mark.parametrize("K", [1, 65, 256])
def test_batch_eb(K, U, device):
    c = _batch(100 + K, K, wide=True)
    uniq = np.array([0] if U == 1 else [0] + list(range(1, V - 1, 2))[:35] + [V - 1], dtype=np.int32)
    assert len(uniq) == U and c["lamT"].min() < 6 < c["lamT"].max()       # both digamma branches
    args = (uniq, c["lamT"], c["T"])
    _assert_within(_native(device)[0](*args), yard_eb(*args), ref_eb(*args), f"eb K={K} U={U} {device}")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("K", [1, 3, 64, 65, 128, 129, 256])
def test_doc_estep_fixed_iterations(K, device):
    c = _batch(200 + K, K)
    assert {0, 1, 2, 3, 4, 5, 63, 64, 65} <= set(np.diff(c["doc_off"]).tolist())
    ref = _check_estep(c, device, ALPHA, 0.0, 5, f"estep K={K}")
    assert (ref[2][np.diff(c["doc_off"]) > 0] == 5).all() and ref[2][0] == 0
    _check_estep(c, device, 1.0 / K, 0.0, 1, f"estep alpha=1/K K={K}")    # the learner's default prior
    if K in (3, 129):                           # no iteration: the input gamma and its statistics
        ref = _check_estep(c, device, ALPHA, 0.0, 0, f"estep0 K={K}")
        assert not ref[2].any() and (ref[0][1:] == c["gamma"][1:]).all()


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("K", [64, 256])
def test_doc_estep_past_the_staging_limit(K, device):
    c = _batch(300 + K, K, lens=(L.STAGE_FLOATS // K + 1,))
    assert int(c["doc_off"][1]) * K > L.STAGE_FLOATS
    assert device != "cuda" or _hm.hip().hm_lda_stage_floats() == L.STAGE_FLOATS
    _check_estep(c, device, ALPHA, 0.0, 5, f"long K={K}")


STOP_SEEDS = {3: 400, 65: 416, 256: 400}      # picked on the reference alone for the two asserts below


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("K", sorted(STOP_SEEDS))
def test_doc_estep_documents_stop_on_their_own_change(K, device):
    c = _batch(STOP_SEEDS[K], K)
    ref = _check_estep(c, device, ALPHA, 1e-3, 100, f"stop K={K}")
    # on the reference alone: no stop is a matter of rounding, and the stops are spread out
    assert all(abs(ch / 1e-3 - 1) >= 0.01 for ch in ref[4])
    assert len({int(i) for i in ref[2] if 0 < i < 100}) >= 3, sorted(set(ref[2].tolist()))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("single", [False, True], ids=["batch", "U1"])
@pytest.mark.parametrize("rho", [1.0, 64 ** -0.7])
@pytest.mark.parametrize("K", [1, 65, 256])
def test_mstep(K, rho, single, device):
    c = _batch(500 + K, K, lens=(1, 40, 90, 60, 70), nV=1031)
    wid = np.full(5, 11, dtype=np.int32) if single else c["wid"]          # U = 1: one word five times
    perm, word_off, uniq = (x.numpy() for x in L.batch_index(torch.from_numpy(wid.copy())))
    contrib = (np.random.default_rng(K).random((len(perm), K)) * 3).astype(np.float32)
    lamT, T, nV, eta, scale = c["lamT"], c["T"], 1031, 1.0 / K, 1000 / 5
    assert len(uniq) == (1 if single else len(uniq)) < nV // 2 and nV % 64 and (single or np.diff(word_off).max() > 1)
    args = (word_off, perm, uniq, contrib, rho, eta, scale, lamT, T)
    ref, yard, got, again = REF[2](*args), YARD[2](*args), _native(device)[2](*args), _native(device)[2](*args)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))          # the same bits twice
    _assert_within(got[0], yard[0], ref[0], f"mstep lamT K={K} rho={rho:.3g} U={len(uniq)} {device}")
    _assert_within(got[1], yard[1], ref[1], f"mstep T K={K} rho={rho:.3g} U={len(uniq)} {device}")
    absent = np.setdiff1d(np.arange(nV), uniq)
    r32, e32 = np.float32(rho), np.float32(eta)                           # the engine's scalars are fp32
    want = np.float64(np.float32(1) - r32) * lamT[absent] + np.float64(r32) * np.float64(e32)
    assert (np.abs(got[0][absent] - want) <= np.spacing(want.astype(np.float32))).all()


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("K", [3, 130])
def test_two_epochs_of_three_mini_batches(K, device):
    batches = [_batch(600 + 10 * K + i, K, lens=(7, 0, 33, 12, 65)[:5 - i]) for i in range(3)]
    alpha, eta = ALPHA, 1.0 / K

    def chain(steps):
        eb, estep, mstep = steps
        lamT, T, t = batches[0]["lamT"], batches[0]["T"], 0
        for _ in range(2):
            for b in batches:
                contrib = estep(b["doc_off"], b["wpos"], b["cnt"], eb(b["uniq"], lamT, T), b["gamma"], alpha, 0.0, 3)[1]
                lamT, T = mstep(b["word_off"], b["perm"], b["uniq"], contrib, (64.0 + t) ** -0.7, eta,
                                50 / (len(b["doc_off"]) - 1), lamT, T)
                t += 1
        return lamT

    _assert_within(chain(_native(device)), chain(YARD), chain(REF), f"chain K={K} {device}")


def _two_topic_docs(n=300):
    """The corpus of tests/test_topic_recommend.py."""
    rng = np.random.default_rng(0)
    A, B = [f"a{i}" for i in range(20)], [f"b{i}" for i in range(20)]
    return [list(rng.choice(A if d % 2 == 0 else B, 30)) for d in range(n)]


@pytest.mark.parametrize("device", DEVICES)
def test_native_model_separates_topics_and_repeats(device):
    docs = _two_topic_docs()
    m = LDA("-topics 2 -iters 5 -seed 7 -engine native", device=device).fit(docs)
    th = m.transform(docs[:10])
    lab = th.argmax(1)
    assert (lab[0::2] == lab[0]).all() and (lab[1::2] != lab[0]).all() and th.max(1).min() > 0.8
    np.testing.assert_allclose(th.sum(1), 1.0, atol=8 * ULP)
    assert len(m.perplexities) >= 2 and m.perplexities[-1] < m.perplexities[0]
    again = LDA("-topics 2 -iters 5 -seed 7 -engine native", device=device).fit(docs)
    assert m.lam.shape == (2, 40) and m.model_table().equals(again.model_table())


@pytest.mark.parametrize("device", DEVICES)
def test_train_lda_sql_engine_native(device):
    from hivemall_amd.sql import Session

    s = Session(device=device)
    s.register("docs", pd.DataFrame({"words": _two_topic_docs(100)}))
    t = s.sql("SELECT train_lda(words, '-topics 2 -iters 3 -engine native') AS (label, word, lambda) FROM docs")
    assert set(t.columns) == {"label", "word", "lambda"} and len(t) == 2 * 40 and (t["lambda"] > 0).all()


def test_engine_option_resolution():
    with pytest.raises(UDFArgumentException, match="engine"):
        LDA("-engine bogus", device="cpu")
    with pytest.raises(UDFArgumentException, match="256"):
        LDA("-topics 257 -engine native", device="cpu")
    for dev in ("cpu", "cuda"):                 # resolving needs no GPU
        assert LDA("", device=dev).engine() == LDA("-engine auto", device=dev).engine() == "torch"
    assert LDA("-engine native", device="cpu").engine() == "native"


BAD = [("eb", 0, lambda c: c["uniq"].astype(np.int64)), ("eb", 1, lambda c: c["lamT"].astype(np.float64)),
       ("eb", 1, lambda c: np.zeros((V, 257), np.float32)), ("eb", 2, lambda c: c["T"][:-1]),
       ("eb", 0, lambda c: np.array([0, V], np.int32)), ("eb", 0, lambda c: np.array([-1], np.int32)),
       ("estep", 0, lambda c: c["doc_off"].astype(np.int64)), ("estep", 0, lambda c: c["doc_off"][::-1]),
       ("estep", 0, lambda c: c["doc_off"][:-1]), ("estep", 1, lambda c: c["wpos"] + len(c["uniq"])),
       ("estep", 2, lambda c: c["cnt"][:-1]), ("estep", 3, lambda c: c["EbU"].astype(np.float64)),
       ("estep", 4, lambda c: c["gamma"][:-1]), ("estep", 4, lambda c: c["gamma"][:, :-1]), ("estep", 7, lambda c: -1),
       ("mstep", 0, lambda c: c["word_off"][:-1]), ("mstep", 1, lambda c: c["perm"][::-1]),
       ("mstep", 2, lambda c: c["uniq"][::-1]), ("mstep", 2, lambda c: c["uniq"] + V),
       ("mstep", 3, lambda c: c["contrib"][:-1]), ("mstep", 7, lambda c: c["lamT"].T), ("mstep", 8, lambda c: c["T"][:-1]),
       ("eb", 1, lambda c: torch.zeros(V, 3, device="meta")), ("estep", 3, lambda c: torch.zeros(V, 3, device="meta")),
       ("mstep", 3, lambda c: torch.zeros(len(c["wid"]), 3, device="meta"))]


@pytest.mark.parametrize("step,i,bad", BAD)
def test_malformed_inputs_raise_before_any_launch(step, i, bad):
    """CPU tensors only: nothing malformed is ever handed to a device launch."""
    c = dict(_batch(203, 3), contrib=np.ones((len(_batch(203, 3)["wid"]), 3), np.float32))
    t = lambda a: torch.from_numpy(np.array(a)) if isinstance(a, np.ndarray) else a
    good = {"eb": (c["uniq"], c["lamT"], c["T"]),
            "estep": (c["doc_off"], c["wpos"], c["cnt"], c["EbU"], c["gamma"], 1 / 3, 0.0, 2),
            "mstep": (c["word_off"], c["perm"], c["uniq"], c["contrib"], 0.5, 1 / 3, 2.0, c["lamT"], c["T"])}[step]
    fn = {"eb": L.lda_batch_eb, "estep": L.lda_doc_estep, "mstep": L.lda_mstep}[step]
    fn(*map(t, good))
    args = list(map(t, good))
    args[i] = t(bad(c))
    with pytest.raises(ValueError):
        fn(*args)
