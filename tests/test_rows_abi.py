"""CPU checks of the documents entry points (wp_linear_encode_rows / wp_linear_encode_padded): what they answer without
a device — empty inputs, argument errors — and that anything else fails loudly without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import wordpiece_amd as W


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(W.LIB_PATH):
        from wordpiece_amd import build
        build.build()


VOCAB = ["[UNK]", "a", "##b", "b"]


def test_join_docs_round_trip():
    docs = ["ab", b"", "c d\ne", "é中"]
    text, off = W.join_docs(docs)
    assert text == "ab\n\nc d\ne\né中\n".encode() and off.dtype == np.int64 and off[0] == 0 and off[-1] == len(text)
    assert [text[off[i]:off[i + 1] - 1] for i in range(len(docs))] == [W._bytes(d) for d in docs]
    assert all(text[o - 1:o] == b"\n" for o in off[1:])
    text, off = W.join_docs([])
    assert text == b"" and off.tolist() == [0]


def test_empty_inputs_need_no_device():
    v = W.Vocab(VOCAB)
    for offsets in (None, "byte", "char"):
        for kw, rows in ((dict(docs=[]), 0), (dict(text=b""), 0), (dict(docs=["", "", ""]), 3),
                         (dict(text=b"\n\n", doc_offsets=[0, 1, 2]), 2)):
            out = v.encode_rows(offsets=offsets, **kw)
            assert len(out) == (2 if offsets is None else 3)
            assert out[0].dtype == np.int32 and len(out[0]) == 0
            assert out[1].dtype == np.int64 and out[1].tolist() == [0] * (rows + 1)
            if offsets:
                assert out[2].shape == (0, 2) and out[2].dtype == np.uint32
    ids, lens = v.encode_padded(docs=["", ""], max_len=5, cls_id=101, sep_id=102, pad_id=7)
    assert ids.dtype == np.int32 and ids.tolist() == [[101, 102, 7, 7, 7]] * 2 and lens.tolist() == [2, 2]
    ids, lens = v.encode_padded(docs=[""], max_len=3, sep_id=102)
    assert ids.tolist() == [[102, 0, 0]] and lens.tolist() == [1]
    ids, lens = v.encode_padded(docs=["", ""], max_len=2)
    assert ids.tolist() == [[0, 0]] * 2 and lens.tolist() == [0, 0]
    ids, lens = v.encode_padded(text=b"", max_len=4, cls_id=1)
    assert ids.shape == (0, 4) and lens.shape == (0,)


def test_argument_errors_come_before_the_device():
    v = W.Vocab(VOCAB)
    text = b"ab\na\n"
    for bad in ([0, 3, 3, 5], [0, 5, 3], [0, 3], [0, 3, 6], [1, 3, 5], [0, 2, 5], [0, 3, 4], [0, -1, 5], [0, 9, 5]):
        with pytest.raises(W.WordPieceError, match="document offsets"):
            v.encode_rows(text=text, doc_offsets=bad)
        with pytest.raises(W.WordPieceError, match="document offsets"):
            v.encode_padded(text=text, doc_offsets=bad, max_len=8)
    L = W.lib()
    off = np.array([0, 3, 5], dtype=np.int64)
    ids, splits, offs = C.POINTER(C.c_int32)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_uint32)()
    n, rows = C.c_size_t(), C.c_size_t()
    for unit in (2, -2, 7):
        rc = L.wp_linear_encode_rows(v._h, text, len(text), off.ctypes.data_as(C.POINTER(C.c_int64)), 2, unit, C.byref(ids),
                                     C.byref(splits), C.byref(offs), C.byref(n), C.byref(rows))
        assert rc == 6 and b"unit" in L.wp_last_error()  # WP_ERR_ARG
    with pytest.raises(W.WordPieceError, match="unit"):
        v.encode_rows(docs=["ab"], offsets="word")
    for kw in (dict(max_len=1, cls_id=1, sep_id=2), dict(max_len=0), dict(max_len=-3), dict(max_len=0, cls_id=1)):
        with pytest.raises(W.WordPieceError, match="max_len"):
            v.encode_padded(docs=["ab"], **kw)
        with pytest.raises(W.WordPieceError, match="max_len"):
            v.encode_padded(docs=[""], **kw)
    with pytest.raises(W.WordPieceError, match="docs or text"):
        v.encode_rows()
    with pytest.raises(W.WordPieceError, match="docs or text"):
        v.encode_rows(docs=["a"], text=b"a\n")


def test_no_cpu_fallback_for_documents():
    if W.lib().wp_device_count() > 0:
        pytest.skip("GPU present")
    v = W.Vocab(VOCAB)
    for call in (lambda: v.encode_rows(docs=["ab", ""]), lambda: v.encode_rows(text=b"ab\nb", offsets="char"),
                 lambda: v.encode_rows(text=b"\n"), lambda: v.encode_padded(docs=["ab"], max_len=4),
                 lambda: v.encode_padded(text=b"ab\na\n", doc_offsets=[0, 3, 5], max_len=4, cls_id=1, sep_id=2)):
        with pytest.raises(W.WordPieceError, match="no HIP device"):
            call()


def test_stats_mirror_has_the_documents_fields():
    names = [f[0] for f in W.Stats._fields_]
    assert names[-3:] == ["n_rows", "rows_truncated", "rows_route"]
