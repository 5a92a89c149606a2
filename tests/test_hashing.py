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


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_string_front_end_compiled_for_the_host(tmp_path):
    """The word loaders and mm3 of csrc/kernels/strspan.h (tests/native/strspan_kat.cpp): every
    start position 0..15 x length 0..40 x 4 seeds against murmur3_bytes, then the vectors."""
    exe = tmp_path / "strspan_kat"
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(HERE, "native", "strspan_kat.cpp"),
                           "-o", str(exe)])
    args = []
    for data, seed, want in VECTORS:
        args += [data.hex() or "-", f"{seed:x}", f"{want:x}"]
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"grid {16 * 41 * 4} vectors {len(VECTORS)} bad 0" in r.stdout


# ------------------------------------------------------------------ hm_mhash over its own window
MHASH_STRINGS, MHASH_BYTES = 256, 16384          # HASH_STRINGS, HASH_LDS of csrc/kernels/hashing.hip


def _window_cases() -> dict:
    S, W = MHASH_STRINGS, MHASH_BYTES
    each = W // S
    cases = {
        "edge_lengths": [b"q" * n for n in (*range(10), 31, 32, 33)],
        "utf8": [s.encode() for s in ("日本語", "特徴量", "😀", "😀😀x", "é", "aé😀日", "\u0000", "a\u0000b")],
        "beyond_window": [b"", b"s0", b"L" * (W + 100), b"s1", b"", b"N" * (W + 1), b"", b"s2", b""],
        "five_windows": [b"", b"M" * (5 * W + 3), b""],
    }
    # a first full step before the run: 256 two-byte strings (512 bytes), and 256 strings of 2-4
    # bytes (914 bytes) so that the second step's span does not start at a multiple of 16
    two = [b"%02x" % i for i in range(S)]
    odd = [b"p%d" % i for i in range(S)]
    assert sum(map(len, two)) % 16 == 0 and sum(map(len, odd)) % 16 == 2
    for d in (-1, 0, 1):
        cases[f"count{d:+d}"] = [b"c%d" % i for i in range(S + d)]
        run = [(b"%04d" % i).ljust(each, b"r") for i in range(S - 1)] + [(b"%04d" % S).ljust(each + d, b"e")]
        assert len(run) == S and sum(map(len, run)) == W + d
        cases[f"bytes{d:+d}"] = run
        cases[f"bytes{d:+d}_after_two_byte_step"] = two + run + [b"after", b""]
        cases[f"bytes{d:+d}_after_odd_step"] = odd + run + [b"after", b""]
    return cases


WINDOW = _window_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(WINDOW))
def test_device_kernel_window(case):
    """hm_mhash at the edges of its tiling: raw hashes against murmur3_batch, mhash against
    mhash_batch; the buffer as uploaded and as a misaligned view that launch() has to re-pad."""
    import torch

    from hivemall_amd.ops._packed import mhash_packed
    from hivemall_amd.utils.hashing import mhash_batch, pack_strings

    words = WINDOW[case]
    raw, off = pack_strings(words)
    buf = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()
    big = torch.full((buf.numel() + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    view = big[3:3 + buf.numel()]
    view.copy_(buf)
    assert view.data_ptr() % 16 == 3
    off = torch.from_numpy(off).cuda()
    for seed in SEEDS:
        for nf, want in ((0, murmur3_batch(words, seed)), (1 << 24, mhash_batch(words, 1 << 24, seed))):
            for b in (buf, view):
                got = mhash_packed(b, off, nf, seed).cpu().numpy()
                assert np.array_equal(got, want), f"seed {seed:#x} num_features {nf}"


@pytest.mark.gpu
def test_device_kernel():
    """hm_mhash with num_features = 0 returns the raw hash: one launch per distinct seed."""
    for seed in SEEDS:
        data, want = _by_seed(seed)
        got = mhash_device(data, num_features=0, seed=seed).cpu().numpy().view(np.uint32)
        assert got.tolist() == want.tolist(), f"seed {seed:#x}"
