"""The host side of a packed string column (hivemall_amd/ops/_packed.py, io.ingest.string_buffers):
the offset check, the launch wrapper, the column normalisation and the two packers built on them.
No GPU."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest
import torch

from hivemall_amd import _native
from hivemall_amd.io import ingest
from hivemall_amd.ops import _packed, minhash as mh, sketch as sk


# ------------------------------------------------------------------ check_offsets
def test_check_offsets():
    t = lambda *v: torch.tensor(v, dtype=torch.int64)                       # noqa: E731
    buf = torch.zeros(6, dtype=torch.uint8)
    _packed.check_offsets("minhash", t(0), "rowptr")
    _packed.check_offsets("sketch", t(0, 0, 4, 6), "off", buf)
    _packed.check_offsets("sketch", t(0, 9), "off")                         # no buf: the end is not checked
    for op, name in (("minhash", "off"), ("minhash", "rowptr"), ("sketch", "off")):
        for off, text in ((t(), f"{op}: {name} must hold at least one offset"),
                          (t(1, 2), f"{op}: {name} must start at 0, got 1"),
                          (t(0, 5, 4, 6), f"{op}: {name} must be non-decreasing"),
                          (t(0, 3, 7), f"{op}: {name} ends at 7, buf holds 6 bytes")):
            with pytest.raises(ValueError) as e:
                _packed.check_offsets(op, off, name, buf)
            assert str(e.value) == text


def test_engines_refuse_bad_offsets():
    """The same texts through the engines' entries, each with its own prefix."""
    buf, off, nlen, rowptr = mh.pack_feature_column([["ab:1", "c"], [], ["d"]])
    gid = torch.zeros(3, dtype=torch.int32)
    for bad, text in ((off + 1, "off must start at 0, got 1"),
                      (torch.tensor([0, 5, 4, 6]), "off must be non-decreasing")):
        with pytest.raises(ValueError, match=f"minhash: {text}"):
            mh.minhash_signatures(buf, bad, nlen, rowptr, 4)
        with pytest.raises(ValueError, match=f"sketch: {text}"):
            sk.hll_registers(buf, bad, gid, 1, 11)
    with pytest.raises(ValueError, match="minhash: rowptr must start at 0, got 1"):
        mh.minhash_signatures(buf, off, nlen, rowptr + 1, 4)
    with pytest.raises(ValueError, match="minhash: off ends at 6, buf holds 5 bytes"):
        mh.minhash_signatures(buf[:-1], off, nlen, rowptr, 4)
    with pytest.raises(ValueError, match="sketch: off ends at 6, buf holds 5 bytes"):
        sk.bloom_bits(buf[:-1], off, gid, 1)
    with pytest.raises(ValueError, match="sketch: off must hold at least one offset"):
        sk.hll_registers(buf, off[:0], gid[:0], 1, 11, check=False)
    with pytest.raises(ValueError, match="minhash: off and rowptr must hold at least one offset"):
        mh.minhash_signatures(buf, off[:0], nlen[:0], rowptr, 4, check=False)


# ------------------------------------------------------------------ pad16 / launch
def test_pad16_copies_only_what_it_must():
    base = torch.arange(80, dtype=torch.uint8)
    assert base.data_ptr() % 16 == 0
    for ok in (base, base[:16], base[16:48]):
        assert _packed.pad16(ok) is ok
    for n, view in ((77, base[3:]), (13, base[16:29]), (16, base[3:19]), (0, base[:0]), (1, base[79:])):
        out = _packed.pad16(view)
        assert out is not view and out.data_ptr() % 16 == 0 and out.numel() == max(16, (n + 15) // 16 * 16)
        assert torch.equal(out[:n], view) and not out[n:].any()


def test_launch_on_the_cpu(monkeypatch):
    seen = []
    monkeypatch.setattr(_native, "call_host", lambda name, *a: seen.append((name, a)))
    monkeypatch.setattr(_native, "call_hip", lambda *a: pytest.fail("a CPU buffer went to the GPU"))
    buf = torch.arange(5, dtype=torch.uint8)
    _packed.launch("hm_x", buf, 1, 2)
    _packed.launch("hm_x", buf[::2], 3)                   # not contiguous: copied
    _packed.launch("hm_x", buf[:0], 4)                    # empty: still an address to take
    assert [(n, a[1:]) for n, a in seen] == [("hm_x", (1, 2)), ("hm_x", (3,)), ("hm_x", (4,))]
    assert seen[0][1][0] == buf.data_ptr()
    assert seen[1][1][0] not in (0, buf.data_ptr()) and seen[2][1][0] != 0


def test_mhash_packed_checks_its_arguments():
    buf, off = torch.zeros(4, dtype=torch.uint8), torch.tensor([0, 4])
    for args, text in (((buf.numpy(), off, 0, 0), "buf must be a torch tensor"),
                       ((buf.int(), off, 0, 0), "buf must be torch.uint8"),
                       ((buf, off.int(), 0, 0), "off must be torch.int64"),
                       ((buf, off, 0, 0), "buf must be on a cuda device"),
                       ):
        with pytest.raises(ValueError, match=f"mhash: {text}"):
            _packed.mhash_packed(*args)


# ------------------------------------------------------------------ as_arrow / string_buffers
def _refuse(col):
    return None


def test_as_arrow():
    ident = lambda c: c                                                     # noqa: E731
    a = pa.array(["x", None, "yz"])
    assert _packed.as_arrow(a, pa.string(), _refuse) is a                   # Arrow never meets the hook
    assert _packed.as_arrow(a.slice(1), pa.string(), _refuse).to_pylist() == [None, "yz"]
    ser = pd.Series(a, dtype=pd.ArrowDtype(pa.string()))
    assert _packed.as_arrow(ser, pa.string(), _refuse).to_pylist() == ["x", None, "yz"]
    ch = pa.chunked_array([a.slice(0, 1), a.slice(1)])
    got = _packed.as_arrow(ch, pa.string(), _refuse)
    assert isinstance(got, pa.Array) and got.to_pylist() == ["x", None, "yz"]
    assert _packed.as_arrow(pa.chunked_array([a]), pa.string(), _refuse).equals(a)
    none = _packed.as_arrow(pa.chunked_array([], type=pa.large_string()), pa.string(), _refuse)
    assert isinstance(none, pa.Array) and len(none) == 0 and none.type == pa.large_string()
    # not Arrow yet: the hook decides, pyarrow infers, an empty column takes the caller's type
    assert _packed.as_arrow(["a", None], pa.string(), ident).type == pa.string()
    assert _packed.as_arrow(("a", "b"), pa.string(), ident).to_pylist() == ["a", "b"]
    for empty in (pa.string(), pa.list_(pa.string())):
        got = _packed.as_arrow([], empty, ident)
        assert len(got) == 0 and got.type == empty
    assert _packed.as_arrow(["a"], pa.string(), lambda c: pa.array([1, 2])).to_pylist() == [1, 2]
    assert _packed.as_arrow(["a"], pa.string(), _refuse) is None
    for bad in (["a", 1], [1, "a"], ["\ud800"], [2**70], 7, "abc", {"a": 1}):
        assert _packed.as_arrow(bad, pa.string(), ident) is None, bad
    assert _packed.as_arrow([b"ab", "c"], pa.string(), ident).type == pa.binary()   # the caller's to refuse

    def raises(col):
        raise pa.ArrowInvalid("from the hook")
    assert _packed.as_arrow(["a"], pa.string(), raises) is None


@pytest.mark.parametrize("ty", [pa.string(), pa.large_string()])
def test_string_buffers(ty):
    texts = ["zz", "ab", "", "日本", "c"]
    joined = lambda ts: "".join(ts).encode()                                # noqa: E731
    ends = lambda ts: np.cumsum([0] + [len(t.encode()) for t in ts]).tolist()   # noqa: E731
    arr = pa.array(texts, type=ty)
    for a, ts in ((arr, texts), (arr.slice(1), texts[1:]), (arr.slice(1, 3), texts[1:4]), (arr.slice(2, 0), []),
                  (pa.array([], type=ty), []), (pa.chunked_array([arr.slice(0, 2), arr.slice(2)]).combine_chunks(),
                                                texts)):
        data, so = ingest.string_buffers(a)
        assert so.dtype == np.int64 and so.tolist() == ends(ts)
        assert data.dtype == np.uint8 and bytes(data) == joined(ts)
    data, so = ingest.string_buffers(arr.slice(1), wide=False)
    assert so.dtype == (np.int64 if ty == pa.large_string() else np.int32) and so.tolist() == ends(texts[1:])
    # the values of a list column go the same way
    lists = pa.array([["zz"], ["ab", ""], ["日本", "c"]], type=pa.list_(ty)).slice(1)
    data, so, lo = ingest.arrow_buffers(lists)
    assert bytes(data) == joined(texts[1:]) and so.tolist() == ends(texts[1:]) and lo.tolist() == [0, 2, 4]


# ------------------------------------------------------------------ the two packers
def _model_values(values):
    """What pack_value_column returns for a column of str / int / None, restated."""
    keep = [i for i, v in enumerate(values) if v is not None]
    enc = [str(values[i]).encode() for i in keep]
    return b"".join(enc), np.cumsum([0] + [len(e) for e in enc]).tolist(), keep


@pytest.mark.parametrize("values", [["a", None, "", "日本", None], ["x", None, "yz"], [], [None, None], [0, -1, 2**62],
                                    [7, None, -12345678901], ["only"]])
def test_pack_value_column_forms(values):
    data, off, keep = _model_values(values)
    forms = [values, tuple(values), pd.Series(values, dtype=object), np.array(values, dtype=object)]
    if all(v is None or isinstance(v, str) for v in values):
        for ty in (pa.string(), pa.large_string()):
            a = pa.array(values, type=ty)
            forms += [a, pa.array(["pad"] + values, type=ty).slice(1), pa.chunked_array([a.slice(0, 1), a.slice(1)]),
                      pd.Series(a, dtype=pd.ArrowDtype(ty))]
    elif values and None not in values:
        forms += [np.array(values, dtype=np.int64), pd.Series(values, dtype="int64"), pa.array(values)]
    else:
        forms += [pd.Series(values, dtype="Int64")]
    for col in forms:
        got = sk.pack_value_column(col)
        assert got is not None, type(col)
        assert [t.dtype for t in got] == [torch.uint8, torch.int64, torch.int64]
        assert (bytes(got[0].numpy()), got[1].tolist(), got[2].tolist()) == (data, off, keep), type(col)


def test_pack_value_column_refusals():
    for col in ([1.5, 2.0], pd.Series([1.0, 2.0]), [True, False], pd.Series([True, False]), ["a", 1], [1, "a"],
                [b"ab"], [["a"], ["b"]], [{"a": 1}], [1, 2.5], ["a", float("nan")], 7, "abc",
                np.array(["a", "b"]), np.array([[1, 2]]), np.array([1.5]), pd.Series(["a"], dtype="string"),
                pa.array([1.5]), pa.array([[1]])):
        assert sk.pack_value_column(col) is None, col


def test_pack_feature_column_forms():
    rows = [["ab:1", "c"], None, [], [":2", "日:3"]]
    want = (b"ab:1c:2\xe6\x97\xa5:3", [0, 4, 5, 7, 12], [2, 1, 0, 3], [0, 2, 2, 2, 4])
    ty = pa.list_(pa.string())
    for col in (rows, tuple(rows), np.array(rows + [7], dtype=object)[:4], pd.Series(rows, dtype=object),
                pa.array(rows, type=ty), pa.chunked_array([pa.array(rows[:2], type=ty), pa.array(rows[2:], type=ty)]),
                pa.array([["zz"]] + rows, type=pa.list_(pa.large_string())).slice(1),
                pa.array(rows, type=pa.large_list(pa.string())),
                pd.Series(pa.array(rows, type=ty), dtype=pd.ArrowDtype(ty))):
        got = mh.pack_feature_column(col)
        assert got is not None, type(col)
        assert [t.dtype for t in got] == [torch.uint8, torch.int64, torch.int32, torch.int64]
        assert (bytes(got[0].numpy()), *(t.tolist() for t in got[1:])) == want, type(col)
    assert [t.numel() for t in mh.pack_feature_column([])] == [0, 1, 0, 1]
    assert [t.numel() for t in mh.pack_feature_column(pa.array([], type=ty))] == [0, 1, 0, 1]
    two_d = mh.pack_feature_column(np.array([["a", "b"], ["c:1", "d"]]))      # a 2-D array reads as rows
    assert bytes(two_d[0].numpy()) == b"abc:1d" and two_d[3].tolist() == [0, 2, 4]
    for bad in ([[1, 2, 3]], [{"a": 1.0}], [np.array([0.5, 1.5])], [["a:x"]], [["a:"]], [["a: 1"]], [["a:1", None]],
                [["a", 3]], ["abc"], 7, [["a:inf"]], [["a:1_0"]], pd.Series([1, 2]), pd.Series(["a"]),
                np.array([1, 2]), pa.array(["a"]), pa.array([[1]]), [[None]]):
        assert mh.pack_feature_column(bad) is None, bad
