"""train_kpa's native engine (ops.kpa: csrc/kernels/kpa.hip, csrc/host/kpa_cpu.cpp) against the
Python learner, ``KPA('-engine python ...')``, the fp64 sequential definition, on the same rows.

The twin must equal the learner bit for bit.  The kernel adds in another order and is held to
``1e-9 * max(1, |ref|)`` per weight and per score, the bound of the native SLIM descent against its
fp64 reference: a first-order count of the reordering error at these shapes is ~1e-11, a dropped or
doubled pair term moves a weight by a step, 1e-3 or more."""
import functools
import os
import random
import subprocess

import numpy as np
import pandas as pd
import pytest
import torch

from hivemall_amd.models.recommend import KPA
from hivemall_amd.ops import kpa as K
from hivemall_amd.utils.options import UDFArgumentException

HERE = os.path.dirname(os.path.abspath(__file__))
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
GRID = [(it, c, pkc) for it in (1, 3) for c in (0.01, 1.0) for pkc in (0.5, 1.0)]


@functools.lru_cache(maxsize=None)
def make_rows(n, length, names, seed, labels=(0, 1)):
    """``n`` rows of ``length`` distinct names out of ``names`` in random order (so (h, k) and (k, h)
    both occur), mixed-sign values, some without a value, one explicit 0.0."""
    rng = random.Random(seed)
    feats = [[f"f{j}:{rng.uniform(-2, 2)!r}" if rng.random() < 0.8 else f"f{j}"
              for j in rng.sample(range(names), length)] for _ in range(n)]
    feats[1][0] = feats[1][0].split(":")[0] + ":0.0"
    return feats, [rng.choice(labels) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def reference(key, opts):
    feats, y = make_rows(*key)
    return KPA("-engine python " + opts, device="cpu").fit(feats, y)


def assert_same_model(m, ref):
    assert m.w0 == ref.w0
    for got, want in ((m.w1, ref.w1), (m.w2, ref.w2), (m.w3, ref.w3)):
        assert list(got.items()) == list(want.items())
    pd.testing.assert_frame_equal(m.model_table(), ref.model_table(), check_exact=True)


@pytest.mark.parametrize("labels", [(0, 1), (-1, 1)])
@pytest.mark.parametrize("length", [1, 2, 3, 7])
def test_twin_equals_the_learner_bit_for_bit(length, labels):
    key = (64, length, 12, length, labels)
    held_out = make_rows(16, length, 16, 99)[0]
    for it, c, pkc in GRID:
        opts = f"-iters {it} -c {c} -pkc {pkc}"
        ref = reference(key, opts)
        m = KPA("-engine native " + opts, device="cpu").fit(*make_rows(*key))
        scores = m.decision_function(held_out)          # before the dicts exist: the twin's scoring
        assert "w3" not in m.__dict__ and K.STATS["host"] > 0
        assert np.array_equal(scores, ref.decision_function(held_out))
        assert_same_model(m, ref)


def _declined():
    feats, y = make_rows(8, 3, 12, 5)
    swap = lambda row: [row] + feats[1:]                            # noqa: E731
    return {"repeated-name": (swap(["f1:1.0", "f2", "f1:2.0"]), ""),
            "129-entries": (swap([f"g{j}:0.5" for j in range(129)]), ""),
            "nan-value": (swap(["f1:nan", "f2"]), ""),
            "pkc-0": (feats, "-pkc 0")}, y


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("case", ["repeated-name", "129-entries", "nan-value", "pkc-0"])
def test_declines_route_to_python(case, device):
    cases, y = _declined()
    feats, opts = cases[case]
    want = KPA("-engine python " + opts, device="cpu").fit(feats, y)
    before = dict(K.STATS)
    got = KPA("-engine auto " + opts, device=device).fit(feats, y)
    assert K.STATS["python"] == before["python"] + 1
    assert (K.STATS["hip"], K.STATS["host"]) == (before["hip"], before["host"])
    assert got.w0 == want.w0 or (np.isnan(got.w0) and np.isnan(want.w0))
    assert got.model_table().equals(want.model_table())
    with pytest.raises(UDFArgumentException, match="declines"):
        KPA("-engine native " + opts, device=device).fit(feats, y)


@pytest.mark.parametrize("device", DEVICES)
def test_forced_capacity_and_chunks_change_nothing(device):
    """The smallest capacity with a load factor <= 0.5 (long probe chains) and a pair budget that
    splits the 64 rows into >= 3 chunks, against the default-sized build: bit-identical."""
    key, kw = (64, 7, 12, 7), dict(iters=3, c=1.0, pkc=0.5, device=device)
    feats, y = make_rows(*key)
    ref = reference(key, "-iters 3 -c 1.0 -pkc 0.5")
    plain = K.fit(feats, y, **kw)
    cap = 1 << (2 * len(ref.w3) - 1).bit_length()
    forced = K.fit(feats, y, capacity=cap, pair_budget=64 * 21 // 4, **kw)
    assert forced.table.chunks >= 3 and forced.table.keys.numel() == cap < plain.table.keys.numel()
    assert forced.table.slots == len(ref.w3)
    for a, b in zip((forced.w0, forced.w1, forced.w2, forced.w3, forced.table.ckeys, forced.table.occ),
                    (plain.w0, plain.w1, plain.w2, plain.w3, plain.table.ckeys, plain.table.occ)):
        assert torch.equal(a, b)
    assert list(forced.dicts()[2]) == list(ref.w3)
    if device == "cpu":
        assert forced.dicts()[2] == ref.w3
    with pytest.raises(ValueError, match="load factor"):
        K.fit(feats, y, capacity=cap // 2, **kw)


def test_twin_standalone_under_sanitizers(tmp_path):
    """tests/native/kpa_san.cpp: the twin's three entry points on a small fixed input (rows of 0, 1,
    2 and 128 entries, a forced small table, unseen names at scoring) in a program of its own built
    with -fsanitize=address,undefined.  Host only."""
    exe = tmp_path / "kpa_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(HERE, "native", "kpa_san.cpp"),
                           os.path.join(os.path.dirname(HERE), "csrc", "host", "kpa_cpu.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "kpa_san ok" in out.stdout


# ------------------------------------------------------------------ the kernels
TOL = 1e-9


def assert_close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    dev = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"{what}: largest deviation {dev.max() if dev.size else 0.0:.3e}")
    assert got.shape == want.shape and (dev <= TOL).all(), (what, float(dev.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("c,pkc", [(0.01, 0.5), (1.0, 1.0)])
@pytest.mark.parametrize("length", [1, 2, 63, 64, 65, 128])
def test_kernel_against_the_learner(length, c, pkc):
    n = 16 if length == 128 else 48
    key, opts = (n, length, 2 * length + 4, length), f"-iters 2 -c {c} -pkc {pkc}"
    ref = reference(key, opts)
    before = K.STATS["hip"]
    m = KPA("-engine auto " + opts, device="cuda").fit(*make_rows(*key))
    assert K.STATS["hip"] > before
    for feats in (make_rows(*key)[0], make_rows(16, length, 3 * length + 8, 77)[0]):      # seen, held out
        assert_close(m.decision_function(feats), ref.decision_function(feats), "score")
    got, want = m.model_table(), ref.model_table()
    assert got[["h", "hk"]].equals(want[["h", "hk"]])
    assert_close(m.w0, ref.w0, "w0")
    for col in ("w1", "w2", "w3"):
        assert list(getattr(m, col)) == list(getattr(ref, col))
        assert_close(list(getattr(m, col).values()), list(getattr(ref, col).values()), col)


@pytest.mark.gpu
def test_kernel_is_deterministic():
    feats, y = make_rows(48, 65, 134, 65)
    a, b = (K.fit(feats, y, iters=2, c=1.0, pkc=1.0, device="cuda") for _ in range(2))
    for x, z in zip((a.w0, a.w1, a.w2, a.w3, a.table.ckeys), (b.w0, b.w1, b.w2, b.w3, b.table.ckeys)):
        assert torch.equal(x, z)
