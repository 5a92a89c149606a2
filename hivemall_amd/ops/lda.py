"""Online-VB LDA's three native steps of one mini-batch (``csrc/kernels/lda.hip``,
``csrc/host/lda_cpu.cpp``), the engine behind ``train_lda -engine native``.

State: ``lamT`` f32 ``[V, K]`` (lambda transposed: a word's topic row contiguous) and ``T`` f32
``[K]`` with ``T[k] = sum_w lamT[w][k]``.  There is no ``[V, K]`` table of ``exp(E[log beta])``.

``lda_batch_eb(uniq, lamT, T)`` returns ``EbU[u][k] = exp(digamma(lamT[uniq[u]][k]) -
digamma(T[k]))`` for the batch's ``U`` distinct words only.

``lda_doc_estep(doc_off, wpos, cnt, EbU, gamma, alpha, delta, max_iter)`` runs every document's
fixed point on ``gamma`` (in place), reading word ``n``'s row as ``EbU[wpos[n]]``:

    Et[k]      = exp(digamma(gamma[k]) - digamma(sum_k gamma[k]))
    phinorm[n] = sum_k Et[k] * EbU[wpos[n]][k] + 1e-30
    gamma'[k]  = alpha + Et[k] * sum_n cnt_n * EbU[wpos[n]][k] / phinorm[n]

until ``mean_k |gamma' - gamma| < delta`` (each document on its own change) or ``max_iter``
iterations; then, with ``Et`` of the final ``gamma``, ``contrib[n][k] = Et[k] * EbU[wpos[n]][k] *
cnt_n / phinorm[n]`` and ``bound[d] = sum_n cnt_n * log(phinorm[n])`` in fp64.  A document without
non-zeros gets ``gamma = alpha``, 0 iterations and ``bound = 0``.

``lda_mstep(word_off, perm, uniq, contrib, rho, eta, scale, lamT, T)`` updates ``lamT`` and ``T`` in
place: ``lam' = (1 - rho) * lam + rho * (eta + scale * s[w])`` for every word, ``s[w]`` the sum of
``contrib[perm[j]]`` over the word's run of ``perm`` in run order (zero outside the batch), then
``T[k] = sum_w lam'[w][k]``.  No float atomics: the same input gives the same bits, on any device
of a kind.  ``ops.plsa.batch_index(wid)`` builds ``(perm, word_off, uniq)`` and
``word_positions(wid, uniq)`` builds ``wpos``.

``cuda`` tensors run the gfx950 kernels (lanes over topics, hence ``K <= KMAX``; a document's rows
of ``EbU`` are staged in LDS when ``nd * K <= STAGE_FLOATS``), CPU tensors the OpenMP twins with the
same contracts and orders of addition.

Reference: core/src/main/java/hivemall/topicmodel/OnlineLDAModel.java.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from .. import _native
from . import _args
from .plsa import batch_index, check_doc_batch, check_word_index  # noqa: F401  (batch_index: re-export)

_P = C.c_void_p
_I64 = _native.c_i64
_F32 = C.c_float
_native.register_hip("hm_lda_batch_eb", [_P, _P, _P, C.c_int, C.c_int, _P, _P])
_native.register_hip("hm_lda_doc_estep", [_P, _P, _P, _P, C.c_int, C.c_int, _F32, _F32, C.c_int, _P, _P, _P, _P, _P])
_native.register_hip("hm_lda_mstep", [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _F32, _F32, _F32, _P, _P, _P, _P])
_native.register_hip("hm_lda_mstep_scratch_words", [C.c_int, C.c_int, C.c_int], restype=_I64)
_native.register_hip("hm_lda_stage_floats", [])
_native.register_host("hm_lda_batch_eb_cpu", [_P, _P, _P, C.c_int, C.c_int, _P])
_native.register_host("hm_lda_doc_estep_cpu", [_P, _P, _P, _P, C.c_int, C.c_int, _F32, _F32, C.c_int, _P, _P, _P, _P])
_native.register_host("hm_lda_mstep_cpu", [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _F32, _F32, _F32, _P, _P, _P])
_native.register_host("hm_lda_mstep_scratch_words_cpu", [C.c_int, C.c_int, C.c_int], restype=_I64)

KMAX = 256                  # topics: lanes of one workgroup span them (4 per lane at most)
STAGE_FLOATS = 12 * 1024    # floats of EbU rows (nd * K) one document stages in LDS (lda.hip)


def _want_table(t, name: str) -> tuple:
    _args.want("lda", t, name, torch.float32, 2)
    rows, K = t.shape
    if K < 1 or K > KMAX:
        raise ValueError(f"lda: {K} topics, the native engine holds 1..{KMAX}")
    if rows > 2**31 - 1:
        raise ValueError(f"lda: {name} has {rows} rows, the native engine holds 2^31 - 1")
    return rows, K


def _want_T(T, K: int, lamT) -> None:
    _args.want("lda", T, "T", torch.float32, 1)
    _args.same_device("lda", (lamT, T), ("lamT", "T"))
    if T.numel() != K:
        raise ValueError(f"lda: T must have {K} entries, got {T.numel()}")


def _finite(x) -> float:
    x = float(x)
    if not math.isfinite(x):
        raise ValueError(f"lda: scalar arguments must be finite, got {x}")
    return x


def word_positions(wid: torch.Tensor, uniq: torch.Tensor) -> torch.Tensor:
    """``wpos`` int32 [N]: the rank of every non-zero's word in ``uniq`` (ascending, as
    ``batch_index`` returns it).  A word that ``uniq`` lacks raises."""
    _args.want("lda", wid, "wid", torch.int32, 1)
    _args.want("lda", uniq, "uniq", torch.int32, 1)
    _args.same_device("lda", (wid, uniq), ("wid", "uniq"))
    if wid.numel() == 0:
        return torch.zeros(0, dtype=torch.int32, device=wid.device)
    if uniq.numel() == 0:
        raise ValueError("lda: wid has entries but uniq no word")
    pos = torch.searchsorted(uniq, wid).clamp_(max=uniq.numel() - 1)
    if not torch.equal(uniq[pos], wid):
        raise ValueError("lda: uniq must be ascending and hold every word of wid")
    return pos.to(torch.int32)


def lda_batch_eb(uniq: torch.Tensor, lamT: torch.Tensor, T: torch.Tensor, *, check: bool = True) -> torch.Tensor:
    """``EbU`` f32 [U, K] for ``uniq`` int32 [U] (word ids, each in ``0..V-1``), ``lamT`` f32 [V, K]
    and ``T`` f32 [K].  ``check=False`` skips the range check of ``uniq``, which reads it back."""
    V, K = _want_table(lamT, "lamT")
    _want_T(T, K, lamT)
    _args.want("lda", uniq, "uniq", torch.int32, 1)
    _args.same_device("lda", (lamT, uniq), ("lamT", "uniq"))
    U = uniq.numel()
    if check and U and (int(uniq.min()) < 0 or int(uniq.max()) >= V):
        raise ValueError(f"lda: word ids must be in 0..{V - 1}")
    EbU = torch.empty((U, K), dtype=torch.float32, device=lamT.device)
    if U == 0:
        return EbU
    uniq, lamT, T = (t.contiguous() for t in (uniq, lamT, T))
    p = _native.ptr
    args = (p(uniq), p(lamT), p(T), U, K, p(EbU))
    if lamT.is_cuda:
        _native.call_hip("hm_lda_batch_eb", lamT.device, *args)
    else:
        _native.call_host("hm_lda_batch_eb", *args)
    return EbU


def lda_doc_estep(doc_off: torch.Tensor, wpos: torch.Tensor, cnt: torch.Tensor, EbU: torch.Tensor,
                  gamma: torch.Tensor, alpha: float, delta: float, max_iter: int, *, check: bool = True):
    """(gamma f32 [B, K], contrib f32 [N, K], iters int32 [B], bound f64 [B]) for ``doc_off`` int32
    [B+1], ``wpos`` int32 [N] (ranks into ``EbU``), ``cnt`` f32 [N], ``EbU`` f32 [U, K] and the
    initial ``gamma`` f32 [B, K], contiguous: it is updated in place and returned.

    ``check=False`` skips the value checks of the CSR triple (they read the tensors back) for a
    caller that has validated the batch once and launches it every epoch."""
    U, K = _want_table(EbU, "EbU")
    max_iter = _args.int_in("lda", max_iter, "max_iter", 0)
    alpha, delta = _finite(alpha), _finite(delta)
    if check:
        B = check_doc_batch(doc_off, wpos, cnt, U, op="lda")
    else:
        _args.want("lda", doc_off, "doc_off", torch.int32, 1)
        _args.want("lda", wpos, "wpos", torch.int32, 1)
        _args.want("lda", cnt, "cnt", torch.float32, 1)
        if doc_off.numel() < 1 or cnt.numel() != wpos.numel():
            raise ValueError("lda: doc_off must have B + 1 entries and wpos / cnt the same length")
        B = doc_off.numel() - 1
    _args.want("lda", gamma, "gamma", torch.float32, 2)
    _args.same_device("lda", (EbU, doc_off, wpos, cnt, gamma), ("EbU", "doc_off", "wpos", "cnt", "gamma"))
    if tuple(gamma.shape) != (B, K) or not gamma.is_contiguous():
        raise ValueError(f"lda: gamma must be a contiguous [{B}, {K}], got {tuple(gamma.shape)}")
    dev, N = EbU.device, wpos.numel()
    contrib = torch.empty((N, K), dtype=torch.float32, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    bound = torch.empty(B, dtype=torch.float64, device=dev)
    if B == 0:
        return gamma, contrib, iters, bound
    doc_off, wpos, cnt, EbU = (t.contiguous() for t in (doc_off, wpos, cnt, EbU))
    p = _native.ptr
    args = (p(doc_off), p(wpos), p(cnt), p(EbU), B, K, alpha, delta, max_iter, p(gamma), p(contrib), p(iters),
            p(bound))
    if EbU.is_cuda:
        _native.call_hip("hm_lda_doc_estep", dev, *args)
    else:
        _native.call_host("hm_lda_doc_estep", *args)
    return gamma, contrib, iters, bound


def mstep_scratch_words(U: int, V: int, K: int, device) -> int:
    """4-byte words of scratch ``lda_mstep`` needs for ``U`` batch words of a ``[V, K]`` table on
    ``device``."""
    if torch.device(device).type == "cuda":
        return int(_native.hip().hm_lda_mstep_scratch_words(int(U), int(V), int(K)))
    return int(_native.host().hm_lda_mstep_scratch_words_cpu(int(U), int(V), int(K)))


def mstep_scratch(U: int, V: int, K: int, device) -> torch.Tensor:
    return torch.empty(max(1, mstep_scratch_words(U, V, K, device)), dtype=torch.int32, device=device)


def lda_mstep(word_off: torch.Tensor, perm: torch.Tensor, uniq: torch.Tensor, contrib: torch.Tensor,
              rho: float, eta: float, scale: float, lamT: torch.Tensor, T: torch.Tensor,
              scratch: torch.Tensor | None = None, *, wid: torch.Tensor | None = None, check: bool = True):
    """Update ``lamT`` f32 [V, K] and ``T`` f32 [K] (both contiguous) in place from ``contrib`` f32
    [N, K] and the batch's word index (``batch_index``); returns ``(lamT, T)``.  ``scale`` is
    ``D / B``.  ``scratch``: an int32 tensor of at least ``mstep_scratch_words(U, V, K, device)``
    entries (allocated when omitted).

    ``check=False`` skips ``check_word_index`` for a caller that has validated the index once."""
    V, K = _want_table(lamT, "lamT")
    _want_T(T, K, lamT)
    if not lamT.is_contiguous() or not T.is_contiguous():
        raise ValueError("lda_mstep: lamT and T are updated in place and must be contiguous")
    rho, eta, scale = _finite(rho), _finite(eta), _finite(scale)
    _args.want("lda", contrib, "contrib", torch.float32, 2)
    if check:
        U = check_word_index(word_off, perm, uniq, V, wid, op="lda")
    else:
        _args.want("lda", word_off, "word_off", torch.int32, 1)
        _args.want("lda", perm, "perm", torch.int32, 1)
        _args.want("lda", uniq, "uniq", torch.int32, 1)
        U = uniq.numel()
        if word_off.numel() != U + 1:
            raise ValueError("lda: word_off must have len(uniq) + 1 entries")
    _args.same_device("lda", (lamT, word_off, perm, uniq, contrib), ("lamT", "word_off", "perm", "uniq", "contrib"))
    if tuple(contrib.shape) != (perm.numel(), K):
        raise ValueError(f"lda: contrib must be [{perm.numel()}, {K}], got {tuple(contrib.shape)}")
    if U > V:
        raise ValueError(f"lda: {U} distinct words for a table of {V}")
    dev = lamT.device
    need = mstep_scratch_words(U, V, K, dev)
    if scratch is None:
        scratch = mstep_scratch(U, V, K, dev)
    else:
        _args.want("lda", scratch, "scratch", torch.int32, 1)
        _args.same_device("lda", (lamT, scratch), ("lamT", "scratch"))
        if scratch.numel() < need or not scratch.is_contiguous():
            raise ValueError(f"lda: scratch must be contiguous with {need} entries, got {scratch.numel()}")
    if V == 0:
        return lamT, T
    word_off, perm, uniq, contrib = (t.contiguous() for t in (word_off, perm, uniq, contrib))
    p = _native.ptr
    args = (p(word_off), p(perm), p(uniq), p(contrib), U, V, K, rho, eta, scale, p(lamT), p(T), p(scratch))
    if lamT.is_cuda:
        _native.call_hip("hm_lda_mstep", dev, *args)
    else:
        _native.call_host("hm_lda_mstep", *args)
    return lamT, T
