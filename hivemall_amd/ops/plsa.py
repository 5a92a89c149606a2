"""pLSA's two native steps (``csrc/kernels/plsa.hip``, ``csrc/host/plsa_cpu.cpp``).

``plsa_doc_em(doc_off, wid, cnt, pwzT, delta, max_iter)`` runs the per-document EM of
``train_plsa`` on a mini-batch given as CSR non-zeros: from ``pzd[k] = 1/K``,

    q[n][k] = pzd[k] * pwzT[w_n][k] / max(sum_k pzd[k] * pwzT[w_n][k], 1e-30)
    new[k]  = sum_n cnt_n * q[n][k];  new /= max(sum_k new, 1e-30)
    ch      = mean_k |new - pzd|;     pzd = new

and a document stops after the iteration with ``ch < delta`` (its own change, as upstream
IncrementalPLSAModel) or after ``max_iter`` iterations.  It returns ``pzd [B, K]``,
``contrib[n][k] = cnt_n * q[n][k]`` with ``q`` from the final ``pzd``, and the iterations each
document ran.  A document without non-zeros gets ``pzd = 0`` and 0 iterations.

``plsa_mstep(word_off, perm, uniq, contrib, alpha, pwzT)`` is the incremental P(w|z) update on
``pwzT`` in place: ``nwz[w] = sum of contrib over the word's run of perm``,
``p' = (1 - alpha) p + alpha nwz / max(S_k, 1e-30)`` with ``S_k = sum_w nwz[w][k]`` (words
outside the batch: ``(1 - alpha) p``), then ``p' / T_k`` with ``T_k = sum_w p'[w][k]``.  No
float atomics: two runs on the same input give the same bits.  ``batch_index(wid)`` builds
``perm``, ``word_off`` and ``uniq`` from a batch's word ids.

Everything is fp32 with ``pwzT`` = P(w|z) transposed to ``[V, K]`` (a word's topic row
contiguous).  ``cuda`` tensors run the gfx950 kernels (one workgroup per document, lanes over
topics, hence ``K <= KMAX``; a document's rows of ``pwzT`` are staged in LDS when
``nd * K <= EM_STAGE_FLOATS`` and read from global memory otherwise), CPU tensors the OpenMP
twins with the same contracts.

Reference: core/src/main/java/hivemall/topicmodel/IncrementalPLSAModel.java.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _native
from . import _args

_P = C.c_void_p
_I64 = _native.c_i64
_F32 = C.c_float
_native.register_hip("hm_plsa_doc_em", [_P, _P, _P, _P, C.c_int, C.c_int, _F32, C.c_int, _P, _P, _P, _P])
_native.register_hip("hm_plsa_mstep", [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _F32, _P, _P, _P])
_native.register_hip("hm_plsa_mstep_scratch_words", [C.c_int, C.c_int, C.c_int], restype=_I64)
_native.register_host("hm_plsa_doc_em_cpu", [_P, _P, _P, _P, C.c_int, C.c_int, _F32, C.c_int, _P, _P, _P])
_native.register_host("hm_plsa_mstep_cpu", [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _F32, _P, _P])
_native.register_host("hm_plsa_mstep_scratch_words_cpu", [C.c_int, C.c_int, C.c_int], restype=_I64)

KMAX = 256                  # topics: lanes of one workgroup span them (4 per lane at most)
EM_STAGE_FLOATS = 12 * 1024   # floats of pwzT rows (nd * K) one document stages in LDS (plsa.hip)


def _want_pwzT(pwzT) -> tuple:
    _args.want("plsa", pwzT, "pwzT", torch.float32, 2)
    V, K = pwzT.shape
    if K < 1 or K > KMAX:
        raise ValueError(f"plsa: {K} topics, the native engine holds 1..{KMAX}")
    return V, K


def _rises(off: torch.Tensor, n: int) -> bool:
    return (off.numel() >= 1 and int(off[0]) == 0 and int(off[-1]) == n
            and not bool((off[1:] < off[:-1]).any()))


def check_doc_batch(doc_off: torch.Tensor, wid: torch.Tensor, cnt: torch.Tensor, V: int) -> int:
    """Validate a mini-batch's CSR triple (dtypes, shapes, devices, ``doc_off`` rising from 0 to
    ``N``, ``0 <= wid < V``); returns the number of documents."""
    _args.want("plsa", doc_off, "doc_off", torch.int32, 1)
    _args.want("plsa", wid, "wid", torch.int32, 1)
    _args.want("plsa", cnt, "cnt", torch.float32, 1)
    _args.same_device("plsa", (doc_off, wid, cnt), ("doc_off", "wid", "cnt"))
    N = wid.numel()
    if cnt.numel() != N:
        raise ValueError(f"plsa: wid has {N} entries, cnt {cnt.numel()}")
    if not _rises(doc_off, N):
        raise ValueError("plsa: doc_off must have B + 1 entries rising from 0 to len(wid)")
    if N and (int(wid.min()) < 0 or int(wid.max()) >= V):
        raise ValueError(f"plsa: word ids must be in 0..{V - 1}")
    return doc_off.numel() - 1


def check_word_index(word_off: torch.Tensor, perm: torch.Tensor, uniq: torch.Tensor, V: int,
                     wid: torch.Tensor | None = None) -> int:
    """Validate a batch's word index: ``uniq`` strictly ascending in ``0..V-1``, ``word_off``
    rising from 0 to ``N`` over ``U + 1`` entries, ``perm`` a permutation of ``0..N-1`` that
    ascends inside every word's run and, when the batch's ``wid`` is given, sorts it into
    ``uniq``'s runs.  Returns ``U``."""
    _args.want("plsa", word_off, "word_off", torch.int32, 1)
    _args.want("plsa", perm, "perm", torch.int32, 1)
    _args.want("plsa", uniq, "uniq", torch.int32, 1)
    _args.same_device("plsa", (word_off, perm, uniq), ("word_off", "perm", "uniq"))
    N, U = perm.numel(), uniq.numel()
    if word_off.numel() != U + 1 or not _rises(word_off, N):
        raise ValueError("plsa: word_off must have len(uniq) + 1 entries rising from 0 to len(perm)")
    if U and (int(uniq[0]) < 0 or int(uniq[-1]) >= V or bool((uniq[1:] <= uniq[:-1]).any())):
        raise ValueError(f"plsa: uniq must be strictly ascending word ids in 0..{V - 1}")
    if N:
        if int(perm.min()) < 0 or int(perm.max()) >= N or \
                not bool((torch.bincount(perm.long(), minlength=N) == 1).all()):
            raise ValueError(f"plsa: perm must be a permutation of 0..{N - 1}")
        if U == 0:
            raise ValueError("plsa: perm has entries but uniq no word")
        run = torch.repeat_interleave(torch.arange(U, device=perm.device), (word_off[1:] - word_off[:-1]).long())
        if N > 1 and bool(((perm[1:] <= perm[:-1]) & (run[1:] == run[:-1])).any()):
            raise ValueError("plsa: perm must ascend inside every word's run (sorted by (word, index))")
        if wid is not None:
            _args.want("plsa", wid, "wid", torch.int32, 1)
            _args.same_device("plsa", (perm, wid), ("perm", "wid"))
            if wid.numel() != N or not torch.equal(wid[perm.long()], uniq[run]):
                raise ValueError("plsa: perm / word_off / uniq are not the sorted index of wid")
    return U


def batch_index(wid: torch.Tensor):
    """``(perm, word_off, uniq)`` of a batch's word ids int32 [N]: a stable sort (non-zero
    indices by (word, index)) and its runs, on ``wid``'s device."""
    _args.want("plsa", wid, "wid", torch.int32, 1)
    srt, perm = torch.sort(wid, stable=True)
    uniq, counts = torch.unique_consecutive(srt, return_counts=True)
    word_off = torch.zeros(uniq.numel() + 1, dtype=torch.int32, device=wid.device)
    word_off[1:] = torch.cumsum(counts, 0).to(torch.int32)
    return perm.to(torch.int32), word_off, uniq


def plsa_doc_em(doc_off: torch.Tensor, wid: torch.Tensor, cnt: torch.Tensor, pwzT: torch.Tensor,
                delta: float, max_iter: int, *, check: bool = True):
    """(pzd f32 [B, K], contrib f32 [N, K], iters int32 [B]) for ``doc_off`` int32 [B+1], ``wid``
    int32 [N], ``cnt`` f32 [N] and ``pwzT`` f32 [V, K].

    ``check=False`` skips ``check_doc_batch`` (value checks that read the tensors back) for a
    caller that has validated the batch once and launches it every epoch."""
    V, K = _want_pwzT(pwzT)
    if int(max_iter) < 0:
        raise ValueError("plsa_doc_em: max_iter must be >= 0")
    if check:
        B = check_doc_batch(doc_off, wid, cnt, V)
    else:
        _args.want("plsa", doc_off, "doc_off", torch.int32, 1)
        _args.want("plsa", wid, "wid", torch.int32, 1)
        _args.want("plsa", cnt, "cnt", torch.float32, 1)
        if doc_off.numel() < 1 or cnt.numel() != wid.numel():
            raise ValueError("plsa: doc_off must have B + 1 entries and wid / cnt the same length")
        B = doc_off.numel() - 1
    _args.same_device("plsa", (pwzT, doc_off, wid, cnt), ("pwzT", "doc_off", "wid", "cnt"))
    dev, N = pwzT.device, wid.numel()
    pzd = torch.empty((B, K), dtype=torch.float32, device=dev)
    contrib = torch.empty((N, K), dtype=torch.float32, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return pzd, contrib, iters
    doc_off, wid, cnt, pwzT = (t.contiguous() for t in (doc_off, wid, cnt, pwzT))
    p = _native.ptr
    args = (p(doc_off), p(wid), p(cnt), p(pwzT), B, K, float(delta), int(max_iter), p(pzd), p(contrib), p(iters))
    if pwzT.is_cuda:
        _native.call_hip("hm_plsa_doc_em", dev, *args)
    else:
        _native.call_host("hm_plsa_doc_em", *args)
    return pzd, contrib, iters


def mstep_scratch_words(U: int, V: int, K: int, device) -> int:
    """4-byte words of scratch ``plsa_mstep`` needs for ``U`` batch words of a ``[V, K]`` table on
    ``device`` (it grows with each of them)."""
    if torch.device(device).type == "cuda":
        return int(_native.hip().hm_plsa_mstep_scratch_words(int(U), int(V), int(K)))
    return int(_native.host().hm_plsa_mstep_scratch_words_cpu(int(U), int(V), int(K)))


def mstep_scratch(U: int, V: int, K: int, device) -> torch.Tensor:
    return torch.empty(max(1, mstep_scratch_words(U, V, K, device)), dtype=torch.int32, device=device)


def plsa_mstep(word_off: torch.Tensor, perm: torch.Tensor, uniq: torch.Tensor, contrib: torch.Tensor,
               alpha: float, pwzT: torch.Tensor, scratch: torch.Tensor | None = None, *,
               wid: torch.Tensor | None = None, check: bool = True) -> torch.Tensor:
    """Update ``pwzT`` f32 [V, K] (contiguous) in place from ``contrib`` f32 [N, K] and the batch's
    word index (``batch_index``); returns it.  ``scratch``: an int32 tensor of at least
    ``mstep_scratch_words(U, V, K, device)`` entries (allocated when omitted).

    ``check=False`` skips ``check_word_index`` for a caller that has validated the index once."""
    V, K = _want_pwzT(pwzT)
    if not pwzT.is_contiguous():
        raise ValueError("plsa_mstep: pwzT is updated in place and must be contiguous")
    _args.want("plsa", contrib, "contrib", torch.float32, 2)
    if check:
        U = check_word_index(word_off, perm, uniq, V, wid)
    else:
        _args.want("plsa", word_off, "word_off", torch.int32, 1)
        _args.want("plsa", perm, "perm", torch.int32, 1)
        _args.want("plsa", uniq, "uniq", torch.int32, 1)
        U = uniq.numel()
        if word_off.numel() != U + 1:
            raise ValueError("plsa: word_off must have len(uniq) + 1 entries")
    _args.same_device("plsa", (pwzT, word_off, perm, uniq, contrib), ("pwzT", "word_off", "perm", "uniq", "contrib"))
    if tuple(contrib.shape) != (perm.numel(), K):
        raise ValueError(f"plsa: contrib must be [{perm.numel()}, {K}], got {tuple(contrib.shape)}")
    if U > V:
        raise ValueError(f"plsa: {U} distinct words for a table of {V}")
    dev = pwzT.device
    need = mstep_scratch_words(U, V, K, dev)
    if scratch is None:
        scratch = mstep_scratch(U, V, K, dev)
    else:
        _args.want("plsa", scratch, "scratch", torch.int32, 1)
        _args.same_device("plsa", (pwzT, scratch), ("pwzT", "scratch"))
        if scratch.numel() < need or not scratch.is_contiguous():
            raise ValueError(f"plsa: scratch must be contiguous with {need} entries, got {scratch.numel()}")
    if V == 0:
        return pwzT
    word_off, perm, uniq, contrib = (t.contiguous() for t in (word_off, perm, uniq, contrib))
    p = _native.ptr
    args = (p(word_off), p(perm), p(uniq), p(contrib), U, V, K, float(alpha), p(pwzT), p(scratch))
    if pwzT.is_cuda:
        _native.call_hip("hm_plsa_mstep", dev, *args)
    else:
        _native.call_host("hm_plsa_mstep", *args)
    return pwzT
