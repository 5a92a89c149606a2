"""MurmurHash3_x86_32 against known answers: the widely published vectors of the reference
implementation (the same function as upstream hivemall.utils.hashing.MurmurHash3), through every
route the project hashes by.  They cover tail lengths 0-3, the sign of the top byte and the
project's default seed.  Everything else in the suite compares one of these routes with another;
this is where the tree is tied to absolute values."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from hivemall_amd.utils.hashing import DEFAULT_SEED, mhash_device, murmur3_batch, murmurhash3_x86_32_py

HERE = os.path.dirname(os.path.abspath(__file__))

# (bytes, seed, hash)
VECTORS = [
    (b"", 0, 0x00000000),
    (b"", 1, 0x514E28B7),
    (b"", 0xFFFFFFFF, 0x81F16F39),
    (b"\xff\xff\xff\xff", 0, 0x76293B50),
    (b"\x21\x43\x65\x87", 0, 0xF55B516B),
    (b"\x21\x43\x65", 0, 0x7E4A8634),
    (b"\x21\x43", 0, 0xA0F7B07A),
    (b"\x21", 0, 0x72661CF4),
    (b"\x00\x00\x00\x00", 0, 0x2362F9DE),
    (b"\x00\x00\x00", 0, 0x85F0B427),
    (b"\x00\x00", 0, 0x30F4C306),
    (b"\x00", 0, 0x514E28B7),
    (b"test", 0, 0xBA6BD213),
    (b"test", 0x9747B28C, 0x704B81DC),
    (b"abc", 0, 0xB3DD93FA),
    (b"aaaa", 0x9747B28C, 0x5A97808A),
    (b"Hello, world!", 0, 0xC0363E43),
    (b"Hello, world!", 0x9747B28C, 0x24884CBA),
    (b"The quick brown fox jumps over the lazy dog", 0x9747B28C, 0x2FA826CD),
]
SEEDS = sorted({seed for _, seed, _ in VECTORS})


def _by_seed(seed):
    data = [d for d, s, _ in VECTORS if s == seed]
    want = np.array([h for _, s, h in VECTORS if s == seed], dtype=np.uint32)
    return data, want


def test_vectors_cover_the_cases():
    assert len(VECTORS) == 19
    assert {len(d) & 3 for d, _, _ in VECTORS} == {0, 1, 2, 3}
    assert DEFAULT_SEED in SEEDS


@pytest.mark.parametrize("data,seed,want", VECTORS)
def test_python_restatement(data, seed, want):
    assert murmurhash3_x86_32_py(data, seed) == want


@pytest.mark.parametrize("seed", SEEDS)
def test_host_library(seed):
    data, want = _by_seed(seed)
    got = murmur3_batch(data, seed).view(np.uint32)
    assert got.tolist() == want.tolist()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shared_header_compiled_for_the_host(tmp_path):
    """csrc/kernels/murmur3.h on its own: the byte-loader template, the host pointer version and
    the three steps composed by hand (tests/native/murmur3_kat.cpp)."""
    exe = tmp_path / "murmur3_kat"
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(HERE, "native", "murmur3_kat.cpp"),
                           "-o", str(exe)])
    args = []
    for data, seed, want in VECTORS:
        args += [data.hex() or "-", f"{seed:x}", f"{want:x}"]
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"checked {len(VECTORS)} bad 0" in r.stdout


@pytest.mark.gpu
def test_device_kernel():
    """hm_mhash with num_features = 0 returns the raw hash: one launch per distinct seed."""
    for seed in SEEDS:
        data, want = _by_seed(seed)
        got = mhash_device(data, num_features=0, seed=seed).cpu().numpy().view(np.uint32)
        assert got.tolist() == want.tolist(), f"seed {seed:#x}"
